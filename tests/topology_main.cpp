// Prints the network descriptions of csrc/topology.cpp for tests/test_topology.py: per network the
// X6 group counts, the state_dict order, the trunk's levels and pools, the shared pairs, the cmap.
#include <cstdio>

#include "topology.h"

int main() {
    for (int net = 0; net < 2; ++net) {
        const opose::NetDesc& d = opose::net_desc(net);
        std::printf("net %s\ngroups %d %d %d\n", d.what, d.SG, d.TG, d.UG);
        for (const opose::Layer& L : d.order)
            std::printf("layer %s %d %d %d %d\n", L.s.name.c_str(), L.s.cin, L.s.cout, L.s.ks, L.s.pad);
        for (const opose::Layer& L : d.trunk) std::printf("trunk %s %d %d\n", L.s.name.c_str(), L.lvl, L.pool ? 1 : 0);
        for (const opose::SharedPair& p : d.shared)
            std::printf("shared %s %s %s\n", p.key.c_str(), d.order[p.l1].s.name.c_str(), d.order[p.l2].s.name.c_str());
        std::printf("cmap");
        for (int c : d.cmap) std::printf(" %d", c);
        std::printf("\n");
    }
    return 0;
}
