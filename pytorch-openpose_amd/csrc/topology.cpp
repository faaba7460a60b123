// topology.cpp — builds the two NetDesc (topology.h) from what differs between the networks:
// the trunk's last layers, the branches' output channels and the 3x3 layers of stage 1.
#include "topology.h"

#include <initializer_list>

namespace opose {

namespace {

struct TrunkRow {
    const char* name;
    int cout;
    bool pool;  // MaxPool2d(2, 2) follows
};

// VGG trunk: 3x3 convs, each on the previous one's output; VGG-19's first ten, then `tail`
std::vector<Layer> trunk_layers(std::initializer_list<TrunkRow> tail) {
    std::vector<TrunkRow> rows = {{"conv1_1", 64, false},  {"conv1_2", 64, true},   {"conv2_1", 128, false},
                                  {"conv2_2", 128, true},  {"conv3_1", 256, false}, {"conv3_2", 256, false},
                                  {"conv3_3", 256, false}, {"conv3_4", 256, true},  {"conv4_1", 512, false},
                                  {"conv4_2", 512, false}};
    rows.insert(rows.end(), tail);
    std::vector<Layer> v;
    int cin = 3, lvl = 0;
    for (const TrunkRow& r : rows) {
        v.push_back(Layer{Spec{r.name, cin, r.cout, 3, 1}, lvl, r.pool});
        cin = r.cout;
        lvl += r.pool ? 1 : 0;
    }
    return v;
}

// stage1: "conv5_" / "conv6_"; relu_quirk: the reference's no_relu list names Mconv7_stage6_L1
// only, so the last stage's L2 output takes a ReLU (src/model.py:30-33)
NetDesc describe(const char* what, std::vector<Layer> trunk, std::initializer_list<int> bout, int n3x3,
                 const std::string& stage1, bool relu_quirk) {
    NetDesc d;
    d.what = what;
    d.trunk = std::move(trunk);
    const int B = d.branches = (int)bout.size();
    // swept on the bench, same box: conv4_1 2,101, stage2 2,100, stage3 2,105, stage4 2,107 frames/s
    // against 2,110 with no gate (a round-4 A/B, kept in git history)
    d.gate = "conv3_1";
    for (size_t i = 0; i < d.trunk.size(); ++i)
        if (d.trunk[i].s.name == d.gate) d.gate_trunk = (int)i;
    if (d.gate.rfind("stage", 0) == 0) d.gate_stage = std::stoi(d.gate.substr(5));

    // buffer layouts: the branches' outputs, then the trunk
    for (int b = 0; b < B; ++b) {
        d.bout[b] = bout.begin()[b];
        d.s_off[b] = d.trunk_off;
        d.s_goff[b] = d.trunk_goff;
        d.trunk_off += d.bout[b];
        d.trunk_goff += (d.bout[b] + 7) / 8;  // every slice starts a group
        for (int c = 0; c < d.bout[b]; ++c) d.cmap.push_back(8 * d.s_goff[b] + c);
    }
    for (int c = 0; c < kTrunkOut; ++c) d.cmap.push_back(8 * d.trunk_goff + c);
    d.Sc = d.trunk_off + kTrunkOut;
    d.SG = d.trunk_goff + kTrunkOut / 8;
    d.Tc = B * kMid;
    d.TG = d.Tc / 8;
    d.Uc = B * kHidden;
    d.UG = d.Uc / 8;

    // the CPM stages (src/model.py:52-90, :163-190)
    for (int st = 1; st <= kStages; ++st) {
        StageDesc& sd = d.stages[st - 1];
        std::vector<Spec> base;  // names without the branch suffix; the last one's cout: per branch
        if (st == 1) {
            for (int k = 1; k <= n3x3; ++k) base.push_back({stage1 + std::to_string(k) + "_CPM", kTrunkOut, kMid, 3, 1});
            base.push_back({stage1 + std::to_string(n3x3 + 1) + "_CPM", n3x3 ? kMid : kTrunkOut, kHidden, 1, 0});
            base.push_back({stage1 + std::to_string(n3x3 + 2) + "_CPM", kHidden, 0, 1, 0});
        } else {
            const std::string s = "_stage" + std::to_string(st);
            base.push_back({"Mconv1" + s, d.Sc, kMid, 7, 3});
            for (int k = 2; k <= 5; ++k) base.push_back({"Mconv" + std::to_string(k) + s, kMid, kMid, 7, 3});
            base.push_back({"Mconv6" + s, kMid, kMid, 1, 0});
            base.push_back({"Mconv7" + s, kMid, 0, 1, 0});
        }
        sd.has_open = st > 1 || n3x3 > 0;
        if (sd.has_open) sd.open_key = base[0].name + (B == 2 ? "_L1+L2" : "");
        for (int b = 0; b < B; ++b) {
            for (Spec s : base) {
                if (B == 2) s.name += b ? "_L2" : "_L1";
                sd.layers[b].push_back(s);
            }
            sd.layers[b].back().cout = d.bout[b];
            sd.relu2[b] = relu_quirk && st == kStages && b == 1;
        }
    }

    // state_dict order: the trunk, then branch by branch every stage (src/model.py:92-104); two
    // branches' opening layers are also loaded as one conv
    d.order = d.trunk;
    int open_at[2][kStages] = {};
    for (int b = 0; b < B; ++b)
        for (int st = 0; st < kStages; ++st) {
            open_at[b][st] = (int)d.order.size();
            for (size_t i = 0; i < d.stages[st].layers[b].size(); ++i)
                d.order.push_back(Layer{d.stages[st].layers[b][i], 3, false, B == 2, st > 0 && i == 0});
        }
    for (int st = 0; st < kStages && B == 2; ++st)
        if (d.stages[st].has_open) d.shared.push_back({d.stages[st].open_key, open_at[0][st], open_at[1][st]});
    return d;
}

}  // namespace

const NetDesc& net_desc(int net) {
    // bodypose_model (src/model.py:7-133): branches L1 (38 PAF channels) and L2 (19 heat maps),
    // stage 1 = three 3x3 layers and the 1x1 pair
    static const NetDesc body =
        describe("body", trunk_layers({{"conv4_3_CPM", 256, false}, {"conv4_4_CPM", 128, false}}), {38, 19}, 3, "conv5_", true);
    // handpose_model (src/model.py:136-214): one branch of 22 heat maps, stage 1 = the 1x1 pair
    static const NetDesc hand = describe(
        "hand", trunk_layers({{"conv4_3", 512, false}, {"conv4_4", 512, false}, {"conv5_1", 512, false},
                              {"conv5_2", 512, false}, {"conv5_3_CPM", 128, false}}), {22}, 0, "conv6_", false);
    return net == 0 ? body : hand;
}

}  // namespace opose
