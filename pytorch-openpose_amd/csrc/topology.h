// topology.h — the body and the hand network, each described once (src/model.py): layers in
// state_dict order, the trunk's pools and resolution levels, the CPM stages' structure, the widths
// of the fp32 stage buffers and the group layout of the X6 ones.  The loader and the forwards of
// the host runtime read it; standard C++, no HIP (tests/test_topology.py compiles it alone).
#pragma once
#include <string>
#include <vector>

namespace opose {

struct Spec {
    std::string name;
    int cin, cout, ks, pad;
};

// A state_dict layer with what the launch planner asks about it: lvl, the resolution level of its
// input (0: H .. 3: H/8); pair, one branch of a two-branch launch.  pool: MaxPool2d(2, 2) follows
// (trunk only).  concat_in: it reads a stage-input concat, so its X6 weights follow NetDesc::cmap.
struct Layer {
    Spec s;
    int lvl = 3;
    bool pool = false, pair = false, concat_in = false;
};

// Two branches' layers (NetDesc::order indices) on one input, loaded also as one conv under `key`
struct SharedPair {
    std::string key;
    int l1, l2;
};

// One CPM stage.  Per branch its layers in state_dict order: the opening layer on the stage input
// when has_open (3x3 on the trunk in stage 1, 7x7 on the concat after; open_key: the name it is
// run under, the SharedPair's with two branches), the middle layers (3x3 / 7x7), and the closing
// 1x1 pair, whose second conv takes a ReLU only where relu2 says so.
struct StageDesc {
    std::vector<Spec> layers[2];
    bool has_open = false;
    std::string open_key;
    bool relu2[2] = {false, false};
};

constexpr int kStages = 6;
constexpr int kTrunkOut = 128;  // channels of the trunk's last layer, the stages' shared input
constexpr int kMid = 128;       // channels of a branch's middle layers
constexpr int kHidden = 512;    // channels of stage 1's first closing 1x1

struct NetDesc {
    const char* what = "";  // "body" / "hand"
    int branches = 1, bout[2] = {0, 0};  // and their output channels
    std::vector<Layer> trunk;
    StageDesc stages[kStages];
    // OPOSE_PIPELINE_DEFER gate: the layer before which the next network records it, a trunk
    // layer's name (gate_trunk: its index, else -1) or "stageN" (gate_stage: N >= 2, else 0)
    std::string gate;
    int gate_trunk = -1, gate_stage = 0;
    // Stage buffers: S = [branch outputs | trunk] (the stage input), T = the branches' activations
    // side by side (kMid each), U = stage 1's hidden 1x1 outputs (kHidden each).  fp32: channels
    // per pixel and the first channel of S's slices; X6: 8-channel groups, each slice on its own.
    int Sc = 0, Tc = 0, Uc = 0, trunk_off = 0, s_off[2] = {0, 0};
    int SG = 0, TG = 0, UG = 0, trunk_goff = 0, s_goff[2] = {0, 0};
    std::vector<int> cmap;  // physical channel (X6 S buffer) of channel c of the reference's concat
    std::vector<Layer> order;  // state_dict order
    std::vector<SharedPair> shared;
};

const NetDesc& net_desc(int net);  // OPOSE_NET_BODY (0) / OPOSE_NET_HAND (1)

}  // namespace opose
