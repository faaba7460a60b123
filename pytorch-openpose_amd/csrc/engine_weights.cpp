// engine_weights.cpp — network topology, state_dict order and weight packing of libopose.
#include "engine.h"

namespace opose {

// ---------------------------------------------------------------- topology (src/model.py)
std::vector<Spec> vgg_body() {
    return {{"conv1_1", 3, 64, 3, 1},     {"conv1_2", 64, 64, 3, 1},     {"conv2_1", 64, 128, 3, 1},
            {"conv2_2", 128, 128, 3, 1},  {"conv3_1", 128, 256, 3, 1},   {"conv3_2", 256, 256, 3, 1},
            {"conv3_3", 256, 256, 3, 1},  {"conv3_4", 256, 256, 3, 1},   {"conv4_1", 256, 512, 3, 1},
            {"conv4_2", 512, 512, 3, 1},  {"conv4_3_CPM", 512, 256, 3, 1}, {"conv4_4_CPM", 256, 128, 3, 1}};
}
std::vector<Spec> vgg_hand() {
    return {{"conv1_1", 3, 64, 3, 1},    {"conv1_2", 64, 64, 3, 1},    {"conv2_1", 64, 128, 3, 1},
            {"conv2_2", 128, 128, 3, 1}, {"conv3_1", 128, 256, 3, 1},  {"conv3_2", 256, 256, 3, 1},
            {"conv3_3", 256, 256, 3, 1}, {"conv3_4", 256, 256, 3, 1},  {"conv4_1", 256, 512, 3, 1},
            {"conv4_2", 512, 512, 3, 1}, {"conv4_3", 512, 512, 3, 1},  {"conv4_4", 512, 512, 3, 1},
            {"conv5_1", 512, 512, 3, 1}, {"conv5_2", 512, 512, 3, 1},  {"conv5_3_CPM", 512, 128, 3, 1}};
}
static std::vector<Spec> body_branch(int stage, int br) {
    const int out = br == 1 ? 38 : 19;
    const std::string L = "_L" + std::to_string(br);
    if (stage == 1)
        return {{"conv5_1_CPM" + L, 128, 128, 3, 1}, {"conv5_2_CPM" + L, 128, 128, 3, 1},
                {"conv5_3_CPM" + L, 128, 128, 3, 1}, {"conv5_4_CPM" + L, 128, 512, 1, 0},
                {"conv5_5_CPM" + L, 512, out, 1, 0}};
    const std::string sfx = "_stage" + std::to_string(stage) + L;
    std::vector<Spec> v = {{"Mconv1" + sfx, 185, 128, 7, 3}};
    for (int i = 2; i <= 5; ++i) v.push_back({"Mconv" + std::to_string(i) + sfx, 128, 128, 7, 3});
    v.push_back({"Mconv6" + sfx, 128, 128, 1, 0});
    v.push_back({"Mconv7" + sfx, 128, out, 1, 0});
    return v;
}
static std::vector<Spec> hand_stage(int stage) {
    if (stage == 1) return {{"conv6_1_CPM", 128, 512, 1, 0}, {"conv6_2_CPM", 512, 22, 1, 0}};
    const std::string sfx = "_stage" + std::to_string(stage);
    std::vector<Spec> v = {{"Mconv1" + sfx, 150, 128, 7, 3}};
    for (int i = 2; i <= 5; ++i) v.push_back({"Mconv" + std::to_string(i) + sfx, 128, 128, 7, 3});
    v.push_back({"Mconv6" + sfx, 128, 128, 1, 0});
    v.push_back({"Mconv7" + sfx, 128, 22, 1, 0});
    return v;
}
static std::vector<Spec> state_dict_order(int net) {
    std::vector<Spec> all;
    if (net == OPOSE_NET_BODY) {
        all = vgg_body();
        for (int br = 1; br <= 2; ++br)
            for (int s = 1; s <= 6; ++s) {
                auto b = body_branch(s, br);
                all.insert(all.end(), b.begin(), b.end());
            }
    } else {
        all = vgg_hand();
        for (int s = 1; s <= 6; ++s) {
            auto b = hand_stage(s);
            all.insert(all.end(), b.begin(), b.end());
        }
    }
    return all;
}

DevConv* find_conv(opose_ctx* h, int net, const std::string& name) {
    auto it = h->convs[net].find(name);
    if (it == h->convs[net].end()) throw std::runtime_error("missing layer " + name);
    return it->second.get();
}

void upload_conv(opose_ctx* h, int net, const std::string& key, const std::vector<const Spec*>& parts,
                 const std::vector<const float*>& w, const std::vector<const float*>& b, const std::vector<int>& cmap) {
    auto dc = std::make_unique<DevConv>();
    const Spec& s0 = *parts[0];
    dc->name = key;
    dc->net = net;
    dc->lvl = key.rfind("conv1_", 0) == 0 ? 0 : key.rfind("conv2_", 0) == 0 ? 1 : key.rfind("conv3_", 0) == 0 ? 2 : 3;
    dc->pair = key.size() > 3 && (key.compare(key.size() - 3, 3, "_L1") == 0 || key.compare(key.size() - 3, 3, "_L2") == 0);
    dc->cin = s0.cin;
    dc->ks = s0.ks;
    dc->pad = s0.pad;
    dc->K = s0.cin * s0.ks * s0.ks;
    dc->tap_major = s0.cin >= 32;
    const int cin_pad = round_up(s0.cin, 32);
    dc->Kpad = dc->tap_major ? s0.ks * s0.ks * cin_pad : round_up(dc->K, 32);
    int cout = 0;
    for (auto* p : parts) cout += p->cout;
    dc->cout = cout;
    dc->Mpad = cout <= 64 ? 64 : round_up(cout, 128);
    std::vector<float> wt((size_t)dc->Kpad * dc->Mpad, 0.f), bias(cout, 0.f);
    int m0 = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        for (int m = 0; m < parts[i]->cout; ++m) {
            for (int k = 0; k < dc->K; ++k) {
                // reference layout OIHW: k = c * ks*ks + tap
                const int c = k / (s0.ks * s0.ks), tap = k % (s0.ks * s0.ks);
                // blocked layout: K = (32-channel block, tap, channel in block) -- a workgroup
                // walks all taps of one channel block before the next, so the im2col rows it
                // gathers are re-read from L2 while still resident (see conv.hip)
                const int kk = dc->tap_major ? ((c / 32) * (s0.ks * s0.ks) + tap) * 32 + (c % 32) : k;
                wt[(size_t)kk * dc->Mpad + m0 + m] = w[i][(size_t)m * dc->K + k];
            }
            bias[m0 + m] = b[i][m];
        }
        m0 += parts[i]->cout;
    }
    std::vector<int> ktab(dc->Kpad, 0);  // padding rows: any in-range tap (weights are 0)
    for (int k = 0; k < dc->K; ++k) {
        int c = k / (dc->ks * dc->ks), r = k % (dc->ks * dc->ks);
        ktab[k] = (c << 8) | ((r / dc->ks) << 4) | (r % dc->ks);
    }
    // X6 weights: input channel c of the reference layer sits at physical channel cmap[c]
    {
        const int cin_phys = cmap.empty() ? s0.cin : cmap.back() + 1;
        const int taps = s0.ks * s0.ks;
        std::vector<float> wp((size_t)cout * cin_phys * taps, 0.f);
        int mm = 0;
        for (size_t i = 0; i < parts.size(); ++i)
            for (int m = 0; m < parts[i]->cout; ++m, ++mm)
                for (int c = 0; c < s0.cin; ++c) {
                    const int pc = cmap.empty() ? c : cmap[c];
                    for (int t = 0; t < taps; ++t)
                        wp[((size_t)mm * cin_phys + pc) * taps + t] = w[i][((size_t)m * s0.cin + c) * taps + t];
                }
        std::vector<uint16_t> wx;
        x6_pack_weights(wp.data(), cout, cin_phys, s0.ks, dc->Mpad, &dc->nK6, wx);
        dc->cin_g = (cin_phys + 7) / 8;
        dc->small6 = dc->cin_g == 1;
        OPOSE_HIP_CHECK(hipMalloc(&dc->wx6, wx.size() * 2));
        OPOSE_HIP_CHECK(hipMemcpy(dc->wx6, wx.data(), wx.size() * 2, hipMemcpyHostToDevice));
        if ((s0.ks == 7 || s0.ks == 3) && dc->Mpad % 128 == 0 && cin_phys > 8) {
            x6_pack_weights_pairs(wp.data(), cout, cin_phys, s0.ks, dc->Mpad, &dc->nK6p, wx);
            OPOSE_HIP_CHECK(hipMalloc(&dc->wx6p, wx.size() * 2));
            OPOSE_HIP_CHECK(hipMemcpy(dc->wx6p, wx.data(), wx.size() * 2, hipMemcpyHostToDevice));
        }
        if (s0.ks == 3 && dc->Mpad % 128 == 0 && cin_phys > 8) {
            x6_pack_weights_wino(wp.data(), cout, cin_phys, dc->Mpad, &dc->nKw, wx);
            OPOSE_HIP_CHECK(hipMalloc(&dc->wwino, wx.size() * 2));
            OPOSE_HIP_CHECK(hipMemcpy(dc->wwino, wx.data(), wx.size() * 2, hipMemcpyHostToDevice));
        }
    }
    OPOSE_HIP_CHECK(hipMalloc(&dc->wt, wt.size() * 4));
    OPOSE_HIP_CHECK(hipMalloc(&dc->bias, bias.size() * 4));
    OPOSE_HIP_CHECK(hipMalloc(&dc->ktab, ktab.size() * 4));
    g_alloc_epoch.fetch_add(1);  // captured graphs may hold the replaced layer's pointers
    OPOSE_HIP_CHECK(hipMemcpy(dc->wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    OPOSE_HIP_CHECK(hipMemcpy(dc->bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    OPOSE_HIP_CHECK(hipMemcpy(dc->ktab, ktab.data(), ktab.size() * 4, hipMemcpyHostToDevice));
    h->convs[net][key] = std::move(dc);
}

}  // namespace opose

using namespace opose;

int opose_load_weights(opose_t* h, int net, const float* const* tensors, const int64_t* shapes, int n) {
    if (!h || !tensors || !shapes || (net != OPOSE_NET_BODY && net != OPOSE_NET_HAND)) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const std::vector<Spec> order = state_dict_order(net);
        if ((size_t)n != 2 * order.size()) {
            h->err = "expected " + std::to_string(2 * order.size()) + " tensors, got " + std::to_string(n);
            return OPOSE_E_WEIGHTS;
        }
        std::map<std::string, std::pair<const float*, const float*>> byname;
        for (size_t i = 0; i < order.size(); ++i) {
            const Spec& s = order[i];
            const int64_t* ws = shapes + 8 * i;
            const int64_t* bs = shapes + 8 * i + 4;
            if (ws[0] != s.cout || ws[1] != s.cin || ws[2] != s.ks || ws[3] != s.ks || bs[0] != s.cout) {
                h->err = "shape mismatch for " + s.name;
                return OPOSE_E_WEIGHTS;
            }
            byname[s.name] = {tensors[2 * i], tensors[2 * i + 1]};
        }
        h->convs[net].clear();
        // physical channel order of the X6 stage-input concat (8-channel groups): body
        // [L1 38 | pad 2 | L2 19 | pad 5 | trunk 128], hand [L 22 | pad 2 | trunk 128]
        std::vector<int> cmap;
        if (net == OPOSE_NET_BODY)
            for (int c = 0; c < 185; ++c) cmap.push_back(c < 38 ? c : (c < 57 ? c + 2 : c + 7));
        else
            for (int c = 0; c < 150; ++c) cmap.push_back(c < 22 ? c : c + 2);
        for (const Spec& s : order)
            upload_conv(h, net, s.name, {&s}, {byname[s.name].first}, {byname[s.name].second},
                        s.name.rfind("Mconv1_", 0) == 0 ? cmap : std::vector<int>{});
        if (net == OPOSE_NET_BODY) {
            // branch-pair layers sharing an input become one GEMM with M = 256
            std::vector<std::string> shared = {"conv5_1_CPM"};
            for (int st = 2; st <= 6; ++st) shared.push_back("Mconv1_stage" + std::to_string(st));
            for (const auto& base : shared) {
                const std::string l1 = base + "_L1", l2 = base + "_L2";
                const Spec *s1 = nullptr, *s2 = nullptr;
                for (const Spec& s : order) {
                    if (s.name == l1) s1 = &s;
                    if (s.name == l2) s2 = &s;
                }
                upload_conv(h, net, base + "_L1+L2", {s1, s2}, {byname[l1].first, byname[l2].first},
                            {byname[l1].second, byname[l2].second},
                            base.rfind("Mconv1_", 0) == 0 ? cmap : std::vector<int>{});
            }
        }
        h->loaded[net] = true;
    });
    return OPOSE_OK;
}
