// engine_weights.cpp — weight packing and upload of libopose, and the per-network table of the
// layers a forward runs (the networks themselves: topology.h).
#include "engine.h"

namespace opose {

static DevConv* find_conv(opose_ctx* h, int net, const std::string& name) {
    auto it = h->convs[net].find(name);
    if (it == h->convs[net].end()) throw std::runtime_error("missing layer " + name);
    return it->second.get();
}

void upload_conv(opose_ctx* h, int net, const std::string& key, const std::vector<const Spec*>& parts,
                 const std::vector<const float*>& w, const std::vector<const float*>& b, int lvl, bool pair,
                 const std::vector<int>& cmap) {
    auto dc = std::make_unique<DevConv>();
    const Spec& s0 = *parts[0];
    dc->name = key;
    dc->net = net;
    dc->lvl = lvl;
    dc->pair = pair;
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
        const NetDesc& d = net_desc(net);
        if ((size_t)n != 2 * d.order.size()) {
            h->err = "expected " + std::to_string(2 * d.order.size()) + " tensors, got " + std::to_string(n);
            return OPOSE_E_WEIGHTS;
        }
        for (size_t i = 0; i < d.order.size(); ++i) {
            const Spec& s = d.order[i].s;
            const int64_t* ws = shapes + 8 * i;
            const int64_t* bs = shapes + 8 * i + 4;
            if (ws[0] != s.cout || ws[1] != s.cin || ws[2] != s.ks || ws[3] != s.ks || bs[0] != s.cout) {
                h->err = "shape mismatch for " + s.name;
                return OPOSE_E_WEIGHTS;
            }
        }
        // the table points into convs[net]: gone before the layers it names, back once complete
        h->loaded[net] = false;
        h->table[net] = NetTable{};
        h->convs[net].clear();
        const std::vector<int> none;
        for (size_t i = 0; i < d.order.size(); ++i) {
            const Layer& L = d.order[i];
            upload_conv(h, net, L.s.name, {&L.s}, {tensors[2 * i]}, {tensors[2 * i + 1]}, L.lvl, L.pair,
                        L.concat_in ? d.cmap : none);
        }
        // branch-pair layers sharing an input become one GEMM with M = 256
        for (const SharedPair& p : d.shared)
            upload_conv(h, net, p.key, {&d.order[p.l1].s, &d.order[p.l2].s}, {tensors[2 * p.l1], tensors[2 * p.l2]},
                        {tensors[2 * p.l1 + 1], tensors[2 * p.l2 + 1]}, 3, false, d.order[p.l1].concat_in ? d.cmap : none);
        NetTable t;
        for (const Layer& L : d.trunk) t.trunk.push_back(find_conv(h, net, L.s.name));
        for (int st = 0; st < kStages; ++st) {
            const StageDesc& sd = d.stages[st];
            if (sd.has_open) t.stages[st].open = find_conv(h, net, sd.open_key);
            for (int b = 0; b < d.branches; ++b) {
                const std::vector<Spec>& ls = sd.layers[b];
                const size_t m0 = sd.has_open ? 1 : 0, m1 = ls.size() - 2;
                for (size_t i = m0; i < m1; ++i) t.stages[st].mid[b].push_back(find_conv(h, net, ls[i].name));
                t.stages[st].close[b][0] = find_conv(h, net, ls[m1].name);
                t.stages[st].close[b][1] = find_conv(h, net, ls[m1 + 1].name);
            }
        }
        h->table[net] = std::move(t);
        h->loaded[net] = true;
    });
    return OPOSE_OK;
}
