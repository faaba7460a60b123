// Stand-alone driver of the host weight packers (pytorch-openpose_amd/csrc/x6_pack.cpp) for
// tests/test_x6_pack.py:  x6_pack_main <plain|pairs|wino> cout cin ks Mpad weights.f32 out.u16
// reads cout*cin*ks*ks floats, writes the packed bf16 units and prints nK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "x6_pack.h"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int cout = atoi(argv[2]), cin = atoi(argv[3]), ks = atoi(argv[4]), Mpad = atoi(argv[5]);
    std::vector<float> w((size_t)cout * cin * ks * ks);
    FILE* f = fopen(argv[6], "rb");
    if (!f || fread(w.data(), sizeof(float), w.size(), f) != w.size()) return 3;
    fclose(f);
    std::vector<uint16_t> out;
    int nK = 0;
    if (!strcmp(argv[1], "plain")) opose::x6_pack_weights(w.data(), cout, cin, ks, Mpad, &nK, out);
    else if (!strcmp(argv[1], "pairs")) opose::x6_pack_weights_pairs(w.data(), cout, cin, ks, Mpad, &nK, out);
    else if (!strcmp(argv[1], "wino") && ks == 3) opose::x6_pack_weights_wino(w.data(), cout, cin, Mpad, &nK, out);
    else return 2;
    f = fopen(argv[7], "wb");
    if (!f || fwrite(out.data(), sizeof(uint16_t), out.size(), f) != out.size()) return 4;
    fclose(f);
    printf("%d\n", nK);
    return 0;
}
