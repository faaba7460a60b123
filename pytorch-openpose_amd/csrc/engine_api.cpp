// engine_api.cpp — the inference entry points of libopose and what drives them: input staging, the
// launch-sequence (hipGraph) cache, the scales of a pyramid, cross-call pipelining.
#include "engine.h"

namespace opose {

// bytes a strided uint8 [N][H][W][3] host view spans: the last row ends 3*W bytes after its start,
// so a view cut from the bottom-right of a larger buffer is never read past its end
static size_t host_span(int N, int H, int W, int64_t row_stride, int64_t frame_stride) {
    return (size_t)(N - 1) * (size_t)frame_stride + (size_t)(H - 1) * (size_t)row_stride + (size_t)W * 3;
}

// a strided uint8 [N][H][W][3] view of the frames on the device: the caller's pointer
// (OPOSE_IN_DEVICE), or the copy of the host frames in h->frames
const uint8_t* stage_frames(opose_ctx* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                                   int64_t frame_stride, int flags) {
    if (flags & OPOSE_IN_DEVICE) return bgr;
    uint8_t* buf = h->frames.ensure<uint8_t>((size_t)frame_stride * N, h->stream);
    OPOSE_HIP_CHECK(hipMemcpyAsync(buf, bgr, host_span(N, H, W, row_stride, frame_stride), hipMemcpyHostToDevice,
                                   h->stream));
    return buf;
}

// n floats of network maps on the device: the caller's pointer (OPOSE_IN_DEVICE), or the copy of
// the host maps in h->maps_in.  One buffer: a multi-scale entry point consumes a scale's maps on
// the handle's stream before it stages the next scale's.
static const float* stage_maps(opose_ctx* h, const float* maps, size_t n, int flags) {
    if (flags & OPOSE_IN_DEVICE) return maps;
    float* buf = h->maps_in.ensure<float>(n, h->stream);
    OPOSE_HIP_CHECK(hipMemcpyAsync(buf, maps, n * 4, hipMemcpyHostToDevice, h->stream));
    return buf;
}

// cv2.resize + pad + normalise of N frames into the network input x of scale g (imgproc.hip)
void preprocess_scale(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                      const ScaleGeom& g, const opose_params& p, float* x, hipStream_t stream) {
    launch_preprocess(frames, frame_stride, row_stride, N, H, W, g.Hs, g.Ws, 1.0 / g.mult, 1.0 / g.mult, g.Hp, g.Wp,
                      (float)p.pad_value / 256.f - 0.5f, x, stream);
}

// preprocess_scale's arguments as one segment's row of a preprocess table (kernels.h PrepSeg)
PrepSeg prep_seg(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                 const ScaleGeom& g, float* x) {
    PrepSeg s{};
    s.src = frames;
    s.out = x;
    s.frame_stride = frame_stride;
    s.row_stride = row_stride;
    s.sy = s.sx = 1.0 / g.mult;
    s.N = N;
    s.H = H;
    s.W = W;
    s.Hs = g.Hs;
    s.Ws = g.Ws;
    s.Hp = g.Hp;
    s.Wp = g.Wp;
    return s;
}

// preprocess_scale of every segment of the table in one launch, through the handle's device table
void preprocess_segs(opose_ctx* h, PrepTable& t, int nseg, const opose_params& p) {
    PrepSeg* dev = h->prep_table.ensure<PrepSeg>(kPrepSegs, h->stream);
    ProfEntry pe;
    double bytes = 0;
    for (int k = 0; k < nseg; ++k) bytes += (double)t.s[k].N * (3.0 * t.s[k].H * t.s[k].W + 12.0 * t.s[k].Hp * t.s[k].Wp);
    h->prof_begin(pe, "preprocess", 0, bytes);
    launch_preprocess_segs(t, nseg, (float)p.pad_value / 256.f - 0.5f, dev, h->stream);
    h->prof_end(pe);
}

// Batch_body.calculate_size_pad (srcmx/Batch_model.py:302-307): int() truncation
BatchGeom batch_geom(const opose_params& p, int H, int W) {
    BatchGeom g;
    g.scale = p.boxsize * p.scales[0] / H;
    g.nh = (int)(H * g.scale);
    g.nw = (int)(W * g.scale);
    if (g.nh <= 0 || g.nw <= 0) throw std::invalid_argument("scale produces an empty image");
    g.Hp = round_up(g.nh, p.stride);
    g.Wp = round_up(g.nw, p.stride);
    return g;
}

// the fast mode's network input x [N][3][Hp][Wp] of N frames (srcmx/Batch_model.py:147-150)
void batch_preprocess(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                      const BatchGeom& g, float* x, hipStream_t stream) {
    const float sc = (float)(1.0 / g.scale);  // torch: float(1 / scale_factor)
    launch_preprocess_torch(frames, frame_stride, row_stride, N, H, W, g.nh, g.nw, sc, sc, g.Hp, g.Wp, x, stream);
}

static opose_params fill_params(const opose_params* p, int net) {
    opose_params q;
    if (p) q = *p;
    else opose_default_params(net, &q);
    if (q.n_scales < 1 || q.n_scales > OPOSE_MAX_SCALES || q.stride != 8 || q.boxsize <= 0)
        throw std::invalid_argument("bad opose_params");
    return q;
}

// Run `work` (device work only: kernels, device memsets/copies on h->stream, no host sync,
// no allocation once warm) through the launch-sequence cache keyed by `key`.  Captures stay on
// the one stream (h->capturing: run_scales_concurrently runs its scales one after another), and
// a captured graph that is not a single chain of nodes is refused (linear_graph).  Cause: in a
// torch process the library runs on torch's bundled HIP runtime (libamdhip64 7.0.2, SONAME
// libamdhip64.so.7, loaded before ours), whose hipGraphLaunch segfaults on a freshly instantiated
// forked graph after other forked executables were destroyed.  scripts/graph_fork_repro.hip
// reproduces it without libopose: the same program crashes under 7.0.2 and runs clean
// under /opt/rocm's 7.2, with no fork in captures, or with no executable destroyed.
// a chain: one root, nodes - 1 edges, and no node with more than one successor (a tree with
// nodes - 1 edges and one root may still branch)
static bool linear_graph(hipGraph_t g) {
    size_t nodes = 0, edges = 0, roots = 0;
    OPOSE_HIP_CHECK(hipGraphGetNodes(g, nullptr, &nodes));
    OPOSE_HIP_CHECK(hipGraphGetEdges(g, nullptr, nullptr, &edges));
    OPOSE_HIP_CHECK(hipGraphGetRootNodes(g, nullptr, &roots));
    if (nodes == 0) return true;
    if (roots != 1 || edges != nodes - 1) return false;
    std::vector<hipGraphNode_t> all(nodes);
    OPOSE_HIP_CHECK(hipGraphGetNodes(g, all.data(), &nodes));
    for (hipGraphNode_t n : all) {
        size_t succ = 0;
        OPOSE_HIP_CHECK(hipGraphNodeGetDependentNodes(n, nullptr, &succ));
        if (succ > 1) return false;
    }
    return true;
}

template <class F>
static void run_graphed(opose_ctx* h, const std::string& key, F&& work) {
    if (!h->use_graphs || h->prof || !h->stream) {
        work();
        return;
    }
    const uint64_t epoch = g_alloc_epoch.load();
    auto it = h->graphs.find(key);
    if (it != h->graphs.end() && it->second.eager) {  // refused once: never captured again
        work();
        return;
    }
    if (it != h->graphs.end() && it->second.exec && it->second.epoch == epoch) {
        OPOSE_HIP_CHECK(hipGraphLaunch(it->second.exec, h->stream));
        return;
    }
    if (it == h->graphs.end() || it->second.epoch != epoch) {  // first sighting: eager, allocates
        if (it != h->graphs.end() && it->second.exec) OPOSE_HIP_CHECK(hipGraphExecDestroy(it->second.exec));
        work();
        h->graphs[key] = GraphEntry{nullptr, g_alloc_epoch.load()};
        return;
    }
    // second sighting with nothing reallocated since: capture, instantiate, launch
    OPOSE_HIP_CHECK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    try {
        Redirect<bool> capturing(h->capturing, true);
        work();
    } catch (...) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(h->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    hipGraph_t g = nullptr;
    OPOSE_HIP_CHECK(hipStreamEndCapture(h->stream, &g));
    if (!linear_graph(g)) {
        // a fork inside a capture (see above): never instantiated.  The captured work did not run,
        // so run it eagerly now, and keep this signature eager (no capture on every later call)
        (void)hipGraphDestroy(g);
        it->second.eager = true;
        work();
        return;
    }
    if (g_alloc_epoch.load() != epoch) {  // something allocated inside the capture: not replayable
        (void)hipGraphDestroy(g);
        h->graphs.erase(key);
        work();
        return;
    }
    hipGraphExec_t ex = nullptr;
    const hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    OPOSE_HIP_CHECK(e);
    it->second.exec = ex;
    OPOSE_HIP_CHECK(hipGraphLaunch(ex, h->stream));
}

static std::string call_key(const char* what, int N, int H, int W, int64_t rs, int64_t fs, const opose_params& p,
                            const void* in_dev, const void* out_dev, int ppp, int maxp) {
    std::string k(what);
    char tmp[256];
    std::snprintf(tmp, sizeof tmp, "|%d|%d|%d|%lld|%lld|%p|%p|%d|%d|", N, H, W, (long long)rs, (long long)fs, in_dev,
                  out_dev, ppp, maxp);
    k += tmp;
    k.append(reinterpret_cast<const char*>(&p), sizeof p);
    return k;
}

// the deferred post-network part (OPOSE_PIPELINE_DEFER) on the handle's stream, after `after`
static void enqueue_deferred_post(opose_ctx* h, hipEvent_t after) {
    opose_ctx::DeferredPost& d = h->dpost;
    if (!d.pending) return;
    d.pending = false;
    OPOSE_HIP_CHECK(hipStreamWaitEvent(h->stream, after, 0));
    {
        Redirect<int> mid_set(h->mid_set, d.set);
        body_post_common(h, d.N, d.H, d.W, d.gs, d.p, d.rec);
    }
    OPOSE_HIP_CHECK(hipEventRecord(h->ev_post[d.set], h->stream));
    h->post_pending[d.set] = true;
}

// enqueue a deferred post-network part now (after its whole network)
void flush_post(opose_ctx* h) {
    if (h->dpost.pending) enqueue_deferred_post(h, h->ev_net);
}

// every entry point that enqueues work on the handle's stream (other than the pipelined body
// path): select the device, and make the next pipelined network wait for that stream
void enter_main(opose_ctx* h) {
    OPOSE_HIP_CHECK(hipSetDevice(h->device));
    flush_post(h);
    h->main_dirty = true;
}

// fn(s) for every scale s, scale s on stream s (0: the handle's stream, others its scale
// streams), each with workspace slot s; the handle's stream continues after all of them
static void run_scales_concurrently(opose_ctx* h, int ns, const std::function<void(int)>& fn) {
    Redirect<int> slot(h->slot);
    if (h->capturing) {  // one stream while capturing (run_graphed): same work, same slots
        for (int s = ns - 1; s >= 0; --s) {
            h->slot = s;
            fn(s);
        }
        return;
    }
    const hipStream_t main = h->stream;
    if (!h->ev_fork) OPOSE_HIP_CHECK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    OPOSE_HIP_CHECK(hipEventRecord(h->ev_fork, main));
    for (int s = 1; s < ns; ++s) {
        if (!h->sstream[s]) {
            OPOSE_HIP_CHECK(pooled_stream(&h->sstream[s], 0));
            OPOSE_HIP_CHECK(hipEventCreateWithFlags(&h->ev_join[s], hipEventDisableTiming));
        }
        OPOSE_HIP_CHECK(hipStreamWaitEvent(h->sstream[s], h->ev_fork, 0));
    }
    // largest scale first: it is the critical path
    {
        Redirect<hipStream_t> stream(h->stream);
        for (int s = ns - 1; s >= 0; --s) {
            h->stream = s ? h->sstream[s] : main;
            h->slot = s;
            fn(s);
            if (s) OPOSE_HIP_CHECK(hipEventRecord(h->ev_join[s], h->sstream[s]));
        }
    }
    for (int s = 1; s < ns; ++s) OPOSE_HIP_CHECK(hipStreamWaitEvent(main, h->ev_join[s], 0));
}

// One scale's frames preprocessed into the network input of workspace set `slot`
static float* preprocess_into(opose_ctx* h, int slot, const uint8_t* fd, int64_t frame_stride, int64_t row_stride, int N,
                              int H, int W, const ScaleGeom& g, const opose_params& p) {
    float* x = h->ws[slot].x.ensure<float>((size_t)N * 3 * g.Hp * g.Wp, h->stream);
    ProfEntry pe;
    h->prof_begin(pe, "preprocess", 0, (double)N * (3.0 * H * W + 12.0 * g.Hp * g.Wp));
    preprocess_scale(fd, frame_stride, row_stride, N, H, W, g, p, x, h->stream);
    h->prof_end(pe);
    return x;
}

// Every scale's network in lockstep on the handle's stream (split-bf16 path): per scale the
// preprocess into its slot's input, one conv launch per layer for all scales (net_forward_x6
// segments), per scale the x8 upsample of its C heat / PAF channels into mid(s).
static void run_scales_lockstep(opose_ctx* h, int net, const uint8_t* fd, int64_t frame_stride, int64_t row_stride,
                                int N, int H, int W, const std::vector<ScaleGeom>& gs, const opose_params& p) {
    if (!h->loaded[net]) throw std::runtime_error(net == OPOSE_NET_BODY ? "body weights not loaded" : "hand weights not loaded");
    std::vector<NetSeg> segs;
    for (size_t s = 0; s < gs.size(); ++s) {
        float* x = preprocess_into(h, (int)s, fd, frame_stride, row_stride, N, H, W, gs[s], p);
        segs.push_back(NetSeg{x, N, gs[s].Hp, gs[s].Wp, (int)s});
    }
    const std::vector<float*> outs = net_forward_x6(h, net, segs);
    for (size_t s = 0; s < gs.size(); ++s)
        if (net == OPOSE_NET_BODY)
            body_to_mid(h, (int)s, outs[s], 185, N, gs[s]);
        else
            upsample_to_mid(h, (int)s, outs[s], 150, N, gs[s], 21);
}

static void pipelined_body(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs,
                           const opose_params& p, uint8_t* rec, const std::function<void()>& net_part,
                           bool defer) {
    if (h->dpost.pending && !(h->dpost.N == N && h->dpost.H == H && h->dpost.W == W)) flush_post(h);
    if (!h->nstream) {
        int lo = 0, hi = 0;
        OPOSE_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // the network stream gets the higher priority: its conv grids should not wait for
        // post-network workgroups that can run on whatever CUs are left (network high / post
        // high / both default measured the same)
        OPOSE_HIP_CHECK(pooled_stream(&h->nstream, hi));
        h->nstream_prio = hi;
        for (hipEvent_t* e : {&h->ev_net, &h->ev_main, &h->ev_post[0], &h->ev_post[1], &h->ev_gate})
            OPOSE_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    const int set = h->next_set;
    h->next_set ^= 1;
    if (h->post_pending[set]) OPOSE_HIP_CHECK(hipStreamWaitEvent(h->nstream, h->ev_post[set], 0));
    if (h->main_dirty) {
        OPOSE_HIP_CHECK(hipEventRecord(h->ev_main, h->stream));
        OPOSE_HIP_CHECK(hipStreamWaitEvent(h->nstream, h->ev_main, 0));
        h->main_dirty = false;
    }
    hipStream_t main = h->stream;
    const bool gate = h->dpost.pending;  // the previous call's post waits for this network's gate
    {
        Redirect<int> mid_set(h->mid_set, set);
        Redirect<hipStream_t> stream(h->stream, h->nstream);
        Redirect<hipEvent_t> gate_ev(h->gate_ev, gate ? h->ev_gate : nullptr);
        h->gate_done = false;
        net_part();
        if (gate && !h->gate_done) OPOSE_HIP_CHECK(hipEventRecord(h->ev_gate, h->nstream));
    }
    // ev_net is re-recorded every call: take the gate first (the deferred post's network ran
    // before this one on nstream, so the gate implies it)
    if (gate) enqueue_deferred_post(h, h->ev_gate);
    OPOSE_HIP_CHECK(hipEventRecord(h->ev_net, h->nstream));
    if (defer) {
        opose_ctx::DeferredPost& d = h->dpost;
        d.pending = true;
        d.N = N;
        d.H = H;
        d.W = W;
        d.set = set;
        d.gs = gs;
        d.p = p;
        d.rec = rec;
        return;
    }
    OPOSE_HIP_CHECK(hipStreamWaitEvent(main, h->ev_net, 0));
    Redirect<int> mid_set(h->mid_set, set);
    body_post_common(h, N, H, W, gs, p, rec);
    OPOSE_HIP_CHECK(hipEventRecord(h->ev_post[set], main));
    h->post_pending[set] = true;
}

// bytes of one direction of a band's halo exchange at wl columns: 3 pieces x 32 groups (the
// widest stage tensor, 256 channels) x 3 rows x P units x 16 B
static size_t band_halo_bytes(int wl) { return (size_t)3 * 32 * 3 * x6p_pitch(wl) * 16; }

}  // namespace opose

using namespace opose;

static int forward_to_caller(opose_t* h, int net, const float* x, int N, int Hp, int Wp, float* o1, float* o2, int flags) {
    if (!h || !x || N <= 0 || Hp < 8 || Wp < 8 || Hp % 8 || Wp % 8) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t in_n = (size_t)N * 3 * Hp * Wp;
        const float* xd = x;
        if (!(flags & OPOSE_IN_DEVICE)) {
            float* buf = h->w().x.ensure<float>(in_n, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(buf, x, in_n * 4, hipMemcpyHostToDevice, h->stream));
            xd = buf;
        }
        const int hl = Hp / 8, wl = Wp / 8;
        const size_t plane = (size_t)hl * wl;
        const hipMemcpyKind kind = (flags & OPOSE_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        // S: [N][Sc][hl][wl], branch b's maps from channel s_off[b] (body: paf, heat; hand: heat)
        const NetDesc& d = net_desc(net);
        float* S = net_forward(h, net, xd, N, Hp, Wp);
        float* const outs[2] = {o1, o2};
        for (int b = 0; b < d.branches; ++b)
            OPOSE_HIP_CHECK(hipMemcpy2DAsync(outs[b], d.bout[b] * plane * 4, S + d.s_off[b] * plane, d.Sc * plane * 4,
                                             d.bout[b] * plane * 4, N, kind, h->stream));
        if (!(flags & OPOSE_OUT_DEVICE)) OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_hand_forward_pyramid(opose_t* h, int n, const float* const* xs, const int* N, const int* Hp, const int* Wp,
                               float* const* heats, int flags) {
    if (!h || !xs || !N || !Hp || !Wp || !heats || n < 1 || n > OPOSE_MAX_SCALES) return OPOSE_E_ARG;
    for (int i = 0; i < n; ++i)
        if (!xs[i] || !heats[i] || N[i] <= 0 || Hp[i] < 8 || Wp[i] < 8 || Hp[i] % 8 || Wp[i] % 8) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        if (!h->loaded[OPOSE_NET_HAND]) throw std::runtime_error("hand weights not loaded");
        const hipMemcpyKind kind = (flags & OPOSE_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        std::vector<NetSeg> segs;
        for (int i = 0; i < n; ++i) {
            const size_t in_n = (size_t)N[i] * 3 * Hp[i] * Wp[i];
            const float* xd = xs[i];
            if (!(flags & OPOSE_IN_DEVICE)) {
                float* buf = h->ws[i].x.ensure<float>(in_n, h->stream);
                OPOSE_HIP_CHECK(hipMemcpyAsync(buf, xs[i], in_n * 4, hipMemcpyHostToDevice, h->stream));
                xd = buf;
            }
            segs.push_back(NetSeg{xd, N[i], Hp[i], Wp[i], i});
        }
        std::vector<float*> outs;
        if (h->x6) {
            outs = net_forward_x6(h, OPOSE_NET_HAND, segs);
        } else {
            Redirect<int> slot(h->slot);
            for (int i = 0; i < n; ++i) {
                h->slot = i;
                outs.push_back(net_forward(h, OPOSE_NET_HAND, segs[i].x, N[i], Hp[i], Wp[i]));
            }
        }
        for (int i = 0; i < n; ++i) {
            const size_t plane = (size_t)(Hp[i] / 8) * (Wp[i] / 8);
            OPOSE_HIP_CHECK(hipMemcpy2DAsync(heats[i], 22 * plane * 4, outs[i], 150 * plane * 4, 22 * plane * 4, N[i],
                                             kind, h->stream));
        }
        if (!(flags & OPOSE_OUT_DEVICE)) OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_body_forward(opose_t* h, const float* x, int N, int Hp, int Wp, float* paf, float* heat, int flags) {
    if (!paf || !heat) return OPOSE_E_ARG;
    return forward_to_caller(h, OPOSE_NET_BODY, x, N, Hp, Wp, paf, heat, flags);
}

int opose_hand_forward(opose_t* h, const float* x, int N, int Hp, int Wp, float* heat, int flags) {
    if (!heat) return OPOSE_E_ARG;
    return forward_to_caller(h, OPOSE_NET_HAND, x, N, Hp, Wp, heat, nullptr, flags);
}

int opose_body_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride, int64_t frame_stride,
                     const opose_params* pp, void* records, int flags) {
    if (!h || !bgr || !records || N <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));  // pipelined or not: decided below
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
        std::vector<ScaleGeom> gs;
        for (int s = 0; s < p.n_scales; ++s) gs.push_back(geom(p.scales[s], p, H, W));
        uint8_t* rec = records_dest(h, N, records, flags);
        auto scale_net = [&](int s) {
            const ScaleGeom& g = gs[s];
            float* x = preprocess_into(h, h->slot, fd, frame_stride, row_stride, N, H, W, g, p);
            float* S = net_forward(h, OPOSE_NET_BODY, x, N, g.Hp, g.Wp);
            body_to_mid(h, s, S, 185, N, g);
        };
        const bool lockstep = h->x6 && h->lockstep && p.n_scales > 1;
        auto net_part = [&] {
            if (lockstep)
                run_scales_lockstep(h, OPOSE_NET_BODY, fd, frame_stride, row_stride, N, H, W, gs, p);
            else if (h->scale_streams && p.n_scales > 1)  // (pipelined: forked from and joined into nstream)
                run_scales_concurrently(h, p.n_scales, scale_net);
            else
                for (int s = 0; s < p.n_scales; ++s) scale_net(s);
        };
        if ((flags & OPOSE_PIPELINE) && (flags & OPOSE_IN_DEVICE) && (flags & OPOSE_OUT_DEVICE)) {
            pipelined_body(h, N, H, W, gs, p, rec, net_part, (flags & OPOSE_PIPELINE_DEFER) != 0);
        } else if (!lockstep && h->scale_streams && p.n_scales > 1) {  // multi-scale pyramid (C5): scales concurrently
            enter_main(h);
            h->mid_set = 0;
            run_scales_concurrently(h, p.n_scales, scale_net);
            body_post_common(h, N, H, W, gs, p, rec);
        } else {
            enter_main(h);
            h->mid_set = 0;
            const std::string key = call_key("body", N, H, W, row_stride, frame_stride, p, fd, rec, h->ppp, h->maxp);
            run_graphed(h, key, [&] {
                net_part();
                body_post_common(h, N, H, W, gs, p, rec);
            });
        }
        return finish_records(h, N, records, rec, flags);
    });
}

int opose_body_infer_groups(opose_t* h, int n_groups, const uint8_t* const* bgr, const int* N, const int* H,
                            const int* W, const int64_t* row_stride, const int64_t* frame_stride,
                            const opose_params* pp, void* const* records, int flags) {
    if (!h || !bgr || !N || !H || !W || !row_stride || !frame_stride || !records) return OPOSE_E_ARG;
    if (n_groups < 1 || n_groups > OPOSE_MAX_SCALES || (flags & (OPOSE_PIPELINE | OPOSE_PIPELINE_DEFER)))
        return OPOSE_E_ARG;
    for (int g = 0; g < n_groups; ++g) {
        if (!bgr[g] || !records[g] || N[g] <= 0 || H[g] <= 0 || W[g] <= 0) return OPOSE_E_ARG;
        if (row_stride[g] < (int64_t)W[g] * 3 || frame_stride[g] < row_stride[g] * H[g]) return OPOSE_E_ARG;
    }
    if (pp && pp->n_scales >= 1 && (int64_t)n_groups * pp->n_scales > OPOSE_MAX_SCALES) return OPOSE_E_ARG;
    if (!(h->x6 && h->lockstep)) {
        // no lockstep (fp32 path, OPOSE_LOCKSTEP=0): the groups one after another, each as its own call
        int worst = OPOSE_OK;
        for (int g = 0; g < n_groups; ++g) {
            const int rc = opose_body_infer(h, bgr[g], N[g], H[g], W[g], row_stride[g], frame_stride[g], pp, records[g],
                                            flags);
            if (rc != OPOSE_OK && rc != OPOSE_E_CAPACITY && rc != OPOSE_E_ASSEMBLY) return rc;
            worst = std::min(worst, rc);
        }
        return worst;
    }
    OPOSE_TRY(h, {
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        const int ns = p.n_scales, nseg = n_groups * ns;
        enter_main(h);
        h->mid_set = 0;
        if (!h->loaded[OPOSE_NET_BODY]) throw std::runtime_error("body weights not loaded");
        const bool id = flags & OPOSE_IN_DEVICE, od = flags & OPOSE_OUT_DEVICE;
        const size_t rbytes = make_record_layout(h->ppp, h->maxp).bytes;
        std::vector<std::vector<ScaleGeom>> gs(n_groups);
        for (int g = 0; g < n_groups; ++g)
            for (int s = 0; s < ns; ++s) gs[g].push_back(geom(p.scales[s], p, H[g], W[g]));
        // Every buffer of the call at its full size before anything is enqueued: a buffer that grew
        // between two groups would synchronise the device and drop what the earlier groups left.
        // Segment (g, s) has workspace and mid set g * ns + s.
        std::vector<size_t> foff(n_groups + 1, 0), roff(n_groups + 1, 0);
        for (int g = 0; g < n_groups; ++g) {
            foff[g + 1] = foff[g] + (size_t)frame_stride[g] * N[g];
            roff[g + 1] = roff[g] + rbytes * N[g];
        }
        uint8_t* fbuf = id ? nullptr : h->frames.ensure<uint8_t>(foff[n_groups], h->stream);
        uint8_t* rbuf = od ? nullptr : h->records.ensure<uint8_t>(roff[n_groups], h->stream);
        h->prep_table.ensure<PrepSeg>(kPrepSegs, h->stream);
        PrepTable table{};
        std::vector<NetSeg> segs;
        std::vector<const uint8_t*> fd(n_groups);
        std::vector<uint8_t*> rec(n_groups);
        for (int g = 0; g < n_groups; ++g) {
            fd[g] = id ? bgr[g] : fbuf + foff[g];
            rec[g] = od ? static_cast<uint8_t*>(records[g]) : rbuf + roff[g];
            body_post_reserve(h, N[g], H[g], W[g], gs[g], g * ns);
            for (int s = 0; s < ns; ++s) {
                const ScaleGeom& sg = gs[g][s];
                float* x = h->ws[g * ns + s].x.ensure<float>((size_t)N[g] * 3 * sg.Hp * sg.Wp, h->stream);
                table.s[g * ns + s] = prep_seg(fd[g], frame_stride[g], row_stride[g], N[g], H[g], W[g], sg, x);
                segs.push_back(NetSeg{x, N[g], sg.Hp, sg.Wp, g * ns + s});
            }
        }
        std::string key;
        for (int g = 0; g < n_groups; ++g) {
            if (!id)
                OPOSE_HIP_CHECK(hipMemcpyAsync(fbuf + foff[g], bgr[g], host_span(N[g], H[g], W[g], row_stride[g], frame_stride[g]),
                                               hipMemcpyHostToDevice, h->stream));
            key += call_key(g ? "" : "body_groups", N[g], H[g], W[g], row_stride[g], frame_stride[g], p, fd[g], rec[g],
                            h->ppp, h->maxp);
        }
        run_graphed(h, key, [&] {
            preprocess_segs(h, table, nseg, p);
            const std::vector<float*> outs = net_forward_x6(h, OPOSE_NET_BODY, segs);
            for (int g = 0; g < n_groups; ++g)
                for (int s = 0; s < ns; ++s) body_to_mid(h, g * ns + s, outs[g * ns + s], 185, N[g], gs[g][s]);
            for (int g = 0; g < n_groups; ++g) body_post_common(h, N[g], H[g], W[g], gs[g], p, rec[g], g * ns);
        });
        return finish_records_groups(h, n_groups, N, records, rec.data(), flags);
    });
}

int opose_body_post(opose_t* h, const float* maps, int N, int hl, int wl, int pad_down, int pad_right, int H, int W,
                    const opose_params* pp, void* records, int flags) {
    if (!h || !maps || !records || N <= 0 || hl <= 0 || wl <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (pad_down < 0 || pad_right < 0 || pad_down >= 8 * hl || pad_right >= 8 * wl) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        opose_params p = fill_params(pp, OPOSE_NET_BODY);
        p.n_scales = 1;
        const float* md = stage_maps(h, maps, (size_t)N * 57 * hl * wl, flags);
        const ScaleGeom g = geom_from_pads(hl, wl, pad_down, pad_right, H, W);
        body_to_mid(h, 0, md, 57, N, g);
        uint8_t* rec = records_dest(h, N, records, flags);
        body_post_common(h, N, H, W, {g}, p, rec);
        return finish_records(h, N, records, rec, flags);
    });
}

// ---- scale-sharded single-frame latency ---------------------------------
int opose_body_scale_geom(int H, int W, const opose_params* pp, int s, int* out4) {
    if (!out4 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    try {
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        if (s < 0 || s >= p.n_scales) return OPOSE_E_ARG;
        const ScaleGeom g = geom(p.scales[s], p, H, W);
        out4[0] = g.hl;
        out4[1] = g.wl;
        out4[2] = g.Hp - g.Hs;
        out4[3] = g.Wp - g.Ws;
        return OPOSE_OK;
    } catch (const std::exception&) {
        return OPOSE_E_SHAPE;
    }
}

int opose_body_scale_maps(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                          int64_t frame_stride, const opose_params* pp, int s, float* maps, int flags) {
    if (!h || !bgr || !maps || N <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        if (s < 0 || s >= p.n_scales) return OPOSE_E_ARG;
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
        const ScaleGeom g = geom(p.scales[s], p, H, W);
        float* x = h->w().x.ensure<float>((size_t)N * 3 * g.Hp * g.Wp, h->stream);
        preprocess_scale(fd, frame_stride, row_stride, N, H, W, g, p, x, h->stream);
        const float* S = net_forward(h, OPOSE_NET_BODY, x, N, g.Hp, g.Wp);
        // channels 0..56 of the stage-6 concat buffer [N][185][hl*wl] -> [N][57][hl*wl]
        const size_t plane = (size_t)g.hl * g.wl * 4;
        OPOSE_HIP_CHECK(hipMemcpy2DAsync(maps, 57 * plane, S, 185 * plane, 57 * plane, N,
                                         (flags & OPOSE_OUT_DEVICE) ? hipMemcpyDeviceToDevice
                                                                    : hipMemcpyDeviceToHost,
                                         h->stream));
        if (!(flags & OPOSE_OUT_DEVICE)) OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        return OPOSE_OK;
    });
}

size_t opose_body_band_halo_bytes(int wl) { return wl > 0 ? band_halo_bytes(wl) : 0; }

int opose_body_band_maps(opose_t* h, const uint8_t* bgr, int H, int W, int64_t row_stride, const opose_params* pp,
                         int s, int r0, int r1, float* maps, opose_halo_fn fn, void* user, void* xbuf,
                         size_t xbuf_bytes, int flags) {
    if (!h || !bgr || !maps || !xbuf || H <= 0 || W <= 0 || row_stride < (int64_t)W * 3) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        if (s < 0 || s >= p.n_scales) return OPOSE_E_ARG;
        const ScaleGeom g = geom(p.scales[s], p, H, W);
        if (r0 < 0 || r1 > g.hl || r1 - r0 < 3) return OPOSE_E_ARG;
        if (!fn && ((r0 > 0 && (!h->comm || h->band_up < 0)) || (r1 < g.hl && (!h->comm || h->band_dn < 0))))
            return OPOSE_E_ARG;  // the library's exchange needs opose_rccl_init + opose_set_band_peers
        if (xbuf_bytes < 4 * band_halo_bytes(g.wl)) return OPOSE_E_ARG;
        if (!h->x6) throw std::invalid_argument("row bands need the split-bf16 path (OPOSE_CONV=f32 is set)");
        if (!h->loaded[OPOSE_NET_BODY]) throw std::runtime_error("body weights not loaded");
        const uint8_t* fd = stage_frames(h, bgr, 1, H, W, row_stride, row_stride * H, flags);
        const int hb = r1 - r0;
        float* out = (flags & OPOSE_OUT_DEVICE) ? maps : h->maps_in.ensure<float>((size_t)57 * hb * g.wl, h->stream);
        float* x = h->w().x.ensure<float>((size_t)3 * g.Hp * g.Wp, h->stream);
        preprocess_scale(fd, row_stride * H, row_stride, 1, H, W, g, p, x, h->stream);
        const size_t cap = xbuf_bytes / 4;
        const Band band{r0, r1, out, fn, user, static_cast<uint8_t*>(xbuf), cap};
        net_forward_x6(h, OPOSE_NET_BODY, {NetSeg{x, 1, g.Hp, g.Wp, h->slot}}, &band);
        if (!(flags & OPOSE_OUT_DEVICE)) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(maps, out, (size_t)57 * hb * g.wl * 4, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        return OPOSE_OK;
    });
}

int opose_body_post_scales(opose_t* h, const float* const* maps, const int* hl, const int* wl, const int* pad_down,
                           const int* pad_right, int n_scales, int N, int H, int W, const opose_params* pp,
                           void* records, int flags) {
    if (!h || !maps || !hl || !wl || !pad_down || !pad_right || !records || N <= 0 || H <= 0 || W <= 0 ||
        n_scales < 1 || n_scales > OPOSE_MAX_SCALES)
        return OPOSE_E_ARG;
    for (int s = 0; s < n_scales; ++s)
        if (!maps[s] || hl[s] <= 0 || wl[s] <= 0 || pad_down[s] < 0 || pad_right[s] < 0 ||
            pad_down[s] >= 8 * hl[s] || pad_right[s] >= 8 * wl[s])
            return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        opose_params p = fill_params(pp, OPOSE_NET_BODY);
        std::vector<ScaleGeom> gs;
        for (int s = 0; s < n_scales; ++s) {
            const ScaleGeom g = geom_from_pads(hl[s], wl[s], pad_down[s], pad_right[s], H, W);
            const float* md = stage_maps(h, maps[s], (size_t)N * 57 * g.hl * g.wl, flags);
            body_to_mid(h, s, md, 57, N, g);
            gs.push_back(g);
        }
        uint8_t* rec = records_dest(h, N, records, flags);
        body_post_common(h, N, H, W, gs, p, rec);
        return finish_records(h, N, records, rec, flags);
    });
}

// The fast mode's launch sequence from the caller's frames to the records at rec_of() on the device
// (opose_batch_body_infer, opose_batch_body_extract): rec_of() names the destination once the
// frames are staged.  Returns it.
template <class F>
static uint8_t* run_batch_body(opose_ctx* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                               int64_t frame_stride, const opose_params& p, int flags, F&& rec_of) {
    const BatchGeom g = batch_geom(p, H, W);
    const int nh = g.nh, nw = g.nw, Hp = g.Hp, Wp = g.Wp;
    const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
    uint8_t* rec = rec_of();
    const std::string key = call_key("batch_body", N, H, W, row_stride, frame_stride, p, fd, rec, h->ppp, h->maxp);
    run_graphed(h, key, [&] {
        float* x = h->w().x.ensure<float>((size_t)N * 3 * Hp * Wp, h->stream);
        ProfEntry pe;
        h->prof_begin(pe, "preprocess", 0, (double)N * (3.0 * H * W + 12.0 * Hp * Wp));
        batch_preprocess(fd, frame_stride, row_stride, N, H, W, g, x, h->stream);
        h->prof_end(pe);
        float* S = net_forward(h, OPOSE_NET_BODY, x, N, Hp, Wp);
        batch_post_common(h, N, H, W, S, 185, Hp / 8, Wp / 8, nh, nw, p, rec);
    });
    return rec;
}

int opose_batch_body_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const opose_params* pp, void* records, int flags) {
    if (!h || !bgr || !records || N <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        uint8_t* rec = run_batch_body(h, bgr, N, H, W, row_stride, frame_stride, p, flags,
                                      [&] { return records_dest(h, N, records, flags); });
        return finish_records(h, N, records, rec, flags);
    });
}

int opose_batch_body_post(opose_t* h, const float* maps, int N, int hl, int wl, int nh, int nw, int H, int W,
                          const opose_params* pp, void* records, int flags) {
    if (!h || !maps || !records || N <= 0 || hl <= 0 || wl <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (nh <= 0 || nw <= 0 || nh > 8 * hl || nw > 8 * wl) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        const float* md = stage_maps(h, maps, (size_t)N * 57 * hl * wl, flags);
        uint8_t* rec = records_dest(h, N, records, flags);
        batch_post_common(h, N, H, W, md, 57, hl, wl, nh, nw, p, rec);
        return finish_records(h, N, records, rec, flags);
    });
}

int opose_hand_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride, int64_t frame_stride,
                     const opose_params* pp, double* peaks, int32_t* found, int flags) {
    if (!h || !bgr || !peaks || !found || N <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_HAND);
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
        std::vector<ScaleGeom> gs;
        for (int s = 0; s < p.n_scales; ++s) gs.push_back(geom(p.scales[s], p, H, W));
        const bool od = flags & OPOSE_OUT_DEVICE;
        char fk[32];
        std::snprintf(fk, sizeof fk, "%p", od ? (const void*)found : nullptr);
        const std::string key =
            call_key("hand", N, H, W, row_stride, frame_stride, p, fd, od ? (const void*)peaks : nullptr, 0, 0) + fk;
        auto scale_net = [&](int s) {
            const ScaleGeom& g = gs[s];
            float* x = preprocess_into(h, h->slot, fd, frame_stride, row_stride, N, H, W, g, p);
            float* Sb = net_forward(h, OPOSE_NET_HAND, x, N, g.Hp, g.Wp);
            upsample_to_mid(h, s, Sb, 150, N, g, 21);
        };
        if (h->x6 && h->lockstep && p.n_scales > 1) {
            run_graphed(h, key, [&] {
                run_scales_lockstep(h, OPOSE_NET_HAND, fd, frame_stride, row_stride, N, H, W, gs, p);
                hand_post_common(h, N, H, W, gs, p, peaks, found, flags & OPOSE_OUT_DEVICE);
            });
        } else if (h->scale_streams && p.n_scales > 1) {
            // the scales' networks are independent until the heat average: each on its own stream
            // with its own workspace (a single crop's layers fill a fraction of the chip each)
            run_scales_concurrently(h, p.n_scales, scale_net);
            hand_post_common(h, N, H, W, gs, p, peaks, found, flags & OPOSE_OUT_DEVICE);
        } else {
            run_graphed(h, key, [&] {
                for (int s = 0; s < p.n_scales; ++s) scale_net(s);
                hand_post_common(h, N, H, W, gs, p, peaks, found, flags & OPOSE_OUT_DEVICE);
            });
        }
        hand_finish(h, N, peaks, found, flags & OPOSE_OUT_DEVICE);
    });
    return OPOSE_OK;
}

int opose_batch_hand_post(opose_t* h, const float* maps, int N, int hl, int wl, const opose_params* pp, double* peaks,
                          int32_t* found, int flags) {
    if (!h || !maps || !peaks || !found || N <= 0 || hl <= 0 || wl <= 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_HAND);
        const float* md = stage_maps(h, maps, (size_t)N * 22 * hl * wl, flags);
        batch_hand_post_common(h, N, 8 * hl, 8 * wl, md, 22, p, peaks, found, flags);
    });
    return OPOSE_OK;
}

int opose_batch_hand_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const opose_params* pp, double* peaks, int32_t* found, int flags) {
    if (!h || !bgr || !peaks || !found || N <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_HAND);
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
        // ToTensor - 0.5 at scale 1 (torch bicubic at scale 1 is the identity)
        float* x = h->w().x.ensure<float>((size_t)N * 3 * H * W, h->stream);
        ProfEntry pe;
        h->prof_begin(pe, "preprocess", 0, (double)N * 15.0 * H * W);
        launch_preprocess_torch(fd, frame_stride, row_stride, N, H, W, H, W, 1.f, 1.f, H, W, x, h->stream);
        h->prof_end(pe);
        float* Sb = net_forward(h, OPOSE_NET_HAND, x, N, H, W);
        batch_hand_post_common(h, N, H, W, Sb, 150, p, peaks, found, flags);
    });
    return OPOSE_OK;
}

// ---- fast-mode hand extraction (srcmx/Batch_model.py:55-104, srcmx/utilmx.py:267-327,
// srcmx/Batch_motion_Estimation.py:19-65) -------------------------------------------------------
// grid z runs over the 2N slots of a batch
bool opose::extract_batch_ok(int N, int boxsize) { return N > 0 && N <= 32767 && boxsize > 0 && boxsize % 8 == 0; }

// n values of T on the device: the caller's pointer (in_device), or the copy of the host values in buf
template <class T>
static const T* stage_values(opose_ctx* h, DevBuf& buf, const T* v, size_t n, bool in_device) {
    if (in_device) return v;
    T* d = buf.ensure<T>(n, h->stream);
    OPOSE_HIP_CHECK(hipMemcpyAsync(d, v, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return d;
}

// the worst of n per-slot statuses on the device, once the handle's stream has passed them
static int worst_slot_status(opose_ctx* h, const int32_t* status_dev, int n, int32_t* status_out) {
    std::vector<int32_t> st(n);
    OPOSE_HIP_CHECK(hipMemcpyAsync(st.data(), status_dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (status_out) std::memcpy(status_out, st.data(), sizeof(int32_t) * n);
    return *std::min_element(st.begin(), st.end());
}

static void run_hand_boxes(opose_ctx* h, const double* motion_dev, int N, int H, int W, int32_t* boxes_dev) {
    ProfEntry pe;
    h->prof_begin(pe, "hand_boxes", 0, (double)N * (18 * 24 + 32));
    launch_hand_boxes(motion_dev, N, H, W, boxes_dev, h->stream);
    h->prof_end(pe);
}

void opose::run_hand_crops(opose_ctx* h, const uint8_t* fd, int64_t frame_stride, int64_t row_stride, int N,
                           int H, int W, const int32_t* boxes_dev, int bs, float* x, uint8_t* crops,
                           int32_t* status_dev) {
    ProfEntry pe;
    h->prof_begin(pe, "hand_crops", 0, 2.0 * N * bs * bs * ((x ? 12.0 : 0.0) + (crops ? 3.0 : 0.0)));
    launch_hand_crops(fd, frame_stride, row_stride, N, H, W, boxes_dev, bs, x, crops, status_dev, h->stream);
    h->prof_end(pe);
}

int opose_batch_hand_boxes(opose_t* h, const double* motion, int N, int H, int W, int32_t* boxes, int flags) {
    if (!h || !motion || !boxes || H <= 0 || W <= 0 || !extract_batch_ok(N, 8)) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const double* md = stage_values(h, h->hx_motion, motion, (size_t)N * 54, flags & OPOSE_IN_DEVICE);
        const bool od = flags & OPOSE_OUT_DEVICE;
        int32_t* bd = od ? boxes : h->hx_boxes.ensure<int32_t>((size_t)N * 8, h->stream);
        run_hand_boxes(h, md, N, H, W, bd);
        if (!od) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(boxes, bd, sizeof(int32_t) * N * 8, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_batch_hand_crops(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const int32_t* boxes, int boxsize, uint8_t* crops, int flags) {
    if (!h || !bgr || !boxes || !crops || H <= 0 || W <= 0 || !extract_batch_ok(N, boxsize)) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
        const int32_t* bd = stage_values(h, h->hx_boxes, boxes, (size_t)N * 8, flags & OPOSE_IN_DEVICE);
        const bool od = flags & OPOSE_OUT_DEVICE;
        const size_t bytes = (size_t)2 * N * boxsize * boxsize * 3;
        uint8_t* cd = od ? crops : h->hx_crops.ensure<uint8_t>(bytes, h->stream);
        int32_t* sd = h->hx_status.ensure<int32_t>((size_t)2 * N, h->stream);
        run_hand_crops(h, fd, frame_stride, row_stride, N, H, W, bd, boxsize, nullptr, cd, sd);
        if (od) {
            h->prof_drain();
            return OPOSE_OK;
        }
        OPOSE_HIP_CHECK(hipMemcpyAsync(crops, cd, bytes, hipMemcpyDeviceToHost, h->stream));
        const int worst = worst_slot_status(h, sd, 2 * N, nullptr);
        h->prof_drain();
        if (worst != OPOSE_OK) h->err = "a present hand box is empty or leaves the frame";
        return worst;
    });
}

int opose_batch_hand_extract(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                             int64_t frame_stride, const double* motion, int boxsize, const opose_params* pp,
                             double* handmat, int32_t* status, int flags) {
    if (!h || !bgr || !motion || !handmat || !status || H <= 0 || W <= 0 || !extract_batch_ok(N, boxsize))
        return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_HAND);
        const int bs = boxsize, slots = 2 * N;
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
        const double* md = stage_values(h, h->hx_motion, motion, (size_t)N * 54, flags & OPOSE_IN_DEVICE);
        const bool od = flags & OPOSE_OUT_DEVICE;
        // every buffer that outlives a chunk is sized here, before the first chunk: a reallocation
        // later would drop the results of the crops already done.  (The network's and the
        // post-processing's workspace is sized by the first chunk, the largest.)
        int32_t* bd = h->hx_boxes.ensure<int32_t>((size_t)slots * 4, h->stream);
        int32_t* sd = od ? status : h->hx_status.ensure<int32_t>((size_t)slots, h->stream);
        double* hm = od ? handmat : h->hx_handmat.ensure<double>((size_t)N * 126, h->stream);
        double* peaks = h->hpeaks.ensure<double>((size_t)slots * 63, h->stream);
        int32_t* found = h->hfound.ensure<int>((size_t)slots * 21, h->stream);
        const size_t per_crop = (size_t)3 * bs * bs;
        float* x = h->w().x.ensure<float>((size_t)slots * per_crop, h->stream);
        run_hand_boxes(h, md, N, H, W, bd);
        run_hand_crops(h, fd, frame_stride, row_stride, N, H, W, bd, bs, x, nullptr, sd);
        // chunks as opose_hand_infer_crops cuts them: the largest activation (64 channels at full
        // resolution, X6: 3 x 128 B per pixel) stays below the 2 GiB the conv kernels address
        // with 32-bit offsets
        const int fit = (int)std::max<size_t>(1, (((size_t)1 << 31) - 1) / ((size_t)3 * 128 * bs * bs));
        const int chunk = h->extract_chunk > 0 ? std::min(h->extract_chunk, fit) : fit;
        for (int c0 = 0; c0 < slots; c0 += chunk) {
            const int nc = std::min(chunk, slots - c0);
            float* Sb = net_forward(h, OPOSE_NET_HAND, x + (size_t)c0 * per_crop, nc, bs, bs);
            batch_hand_post_common(h, nc, bs, bs, Sb, 150, p, peaks + (size_t)c0 * 63, found + (size_t)c0 * 21,
                                   OPOSE_OUT_DEVICE);
        }
        ProfEntry pe;
        h->prof_begin(pe, "hand_backmap", 0, (double)slots * 21 * 52);
        launch_hand_backmap(peaks, found, bd, N, bs, hm, h->stream);
        h->prof_end(pe);
        if (od) {
            h->prof_drain();
            return OPOSE_OK;
        }
        OPOSE_HIP_CHECK(hipMemcpyAsync(handmat, hm, sizeof(double) * N * 126, hipMemcpyDeviceToHost, h->stream));
        const int worst = worst_slot_status(h, sd, slots, status);
        h->prof_drain();
        if (worst != OPOSE_OK) h->err = "a present hand box is empty or leaves the frame";
        return worst;
    });
}

// ---- fast-mode body extraction (srcmx/Batch_motion_Estimation.py:68-113) -----------------------
// pose_select on N device records -> pose / status: the caller's device pointers (out_device;
// asynchronous, OPOSE_OK) or the handle's buffers copied to the host, then the worst status
static int run_pose_select(opose_ctx* h, const uint8_t* rec_dev, int N, double* pose, int32_t* status,
                           bool out_device) {
    double* pd = out_device ? pose : h->px_pose.ensure<double>((size_t)N * 54, h->stream);
    int32_t* sd = out_device ? status : h->px_status.ensure<int32_t>((size_t)N, h->stream);
    ProfEntry pe;
    h->prof_begin(pe, "pose_select", 0, (double)N * (54 * 8 + 4));
    launch_pose_select(rec_dev, N, make_record_layout(h->ppp, h->maxp), pd, sd, h->stream);
    h->prof_end(pe);
    if (out_device) {
        h->prof_drain();
        return OPOSE_OK;
    }
    OPOSE_HIP_CHECK(hipMemcpyAsync(pose, pd, sizeof(double) * N * 54, hipMemcpyDeviceToHost, h->stream));
    const int worst = worst_slot_status(h, sd, N, status);
    h->prof_drain();
    if (worst != OPOSE_OK) h->err = "a frame's record carries a status, or indexes past its candidates";
    return worst;
}

int opose_body_records_pose(opose_t* h, const void* records, int N, double* pose, int32_t* status, int flags) {
    if (!h || !records || !pose || !status || N <= 0) return OPOSE_E_ARG;
    if (reinterpret_cast<uintptr_t>(records) % 8) return OPOSE_E_ARG;  // float64 rows at offset 16
    OPOSE_TRY(h, {
        enter_main(h);
        const uint8_t* rd = static_cast<const uint8_t*>(records);
        if (!(flags & OPOSE_IN_DEVICE)) {
            const size_t bytes = make_record_layout(h->ppp, h->maxp).bytes * N;
            uint8_t* buf = h->records.ensure<uint8_t>(bytes, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(buf, records, bytes, hipMemcpyHostToDevice, h->stream));
            rd = buf;
        }
        return run_pose_select(h, rd, N, pose, status, flags & OPOSE_OUT_DEVICE);
    });
}

int opose_batch_body_extract(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                             int64_t frame_stride, const opose_params* pp, double* pose, int32_t* status, int flags) {
    if (!h || !bgr || !pose || !status || N <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_BODY);
        // the records stay in the handle's buffer, sized (with the staged results) before anything
        // is enqueued.  The launch sequence is opose_batch_body_infer's into that buffer, under
        // that call's key; pose_select follows it eagerly on the same stream.
        uint8_t* rec = h->records.ensure<uint8_t>(make_record_layout(h->ppp, h->maxp).bytes * N, h->stream);
        if (!(flags & OPOSE_OUT_DEVICE)) {
            h->px_pose.ensure<double>((size_t)N * 54, h->stream);
            h->px_status.ensure<int32_t>((size_t)N, h->stream);
        }
        run_batch_body(h, bgr, N, H, W, row_stride, frame_stride, p, flags, [&] { return rec; });
        return run_pose_select(h, rec, N, pose, status, flags & OPOSE_OUT_DEVICE);
    });
}

int opose_hand_infer_crops(opose_t* h, const uint8_t* const* crops, const int* sizes, const int64_t* row_strides,
                           int n, const opose_params* pp, double* peaks, int32_t* found, int flags) {
    if (!h || !crops || !sizes || !row_strides || !peaks || !found || n <= 0) return OPOSE_E_ARG;
    for (int i = 0; i < n; ++i)
        if (!crops[i] || sizes[i] <= 0 || row_strides[i] < (int64_t)sizes[i] * 3) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const opose_params p = fill_params(pp, OPOSE_NET_HAND);
        const int ns = p.n_scales;
        // per-crop geometry; the network side (Hs, Ws, Hp, Wp per scale) must agree across crops
        std::vector<std::vector<ScaleGeom>> gs(n);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < ns; ++s) gs[i].push_back(geom(p.scales[s], p, sizes[i], sizes[i]));
        for (int i = 1; i < n; ++i)
            for (int s = 0; s < ns; ++s)
                if (gs[i][s].Hs != gs[0][s].Hs || gs[i][s].Ws != gs[0][s].Ws)
                    throw std::invalid_argument("crops do not share the network input size of a scale");
        // stage the crops (host -> one device buffer)
        std::vector<size_t> off(n + 1, 0);
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (size_t)row_strides[i] * sizes[i];
        uint8_t* buf = nullptr;
        if (!(flags & OPOSE_IN_DEVICE)) {
            buf = h->frames.ensure<uint8_t>(off[n], h->stream);
            for (int i = 0; i < n; ++i)
                OPOSE_HIP_CHECK(hipMemcpyAsync(buf + off[i], crops[i], host_span(1, sizes[i], sizes[i], row_strides[i], 0),
                                               hipMemcpyHostToDevice, h->stream));
        }
        // all crops of a scale form one batch; with the split-bf16 path all scales run in lockstep
        // (one conv launch per layer for every crop and scale).  Batches are cut so that the
        // largest activation (64 channels at the largest scale's full resolution, X6: 3 x 128 B
        // per pixel) stays below the 2 GiB the conv kernels address with 32-bit offsets.
        const bool lockstep = h->x6 && h->lockstep && ns > 1;
        if (lockstep && !h->loaded[OPOSE_NET_HAND]) throw std::runtime_error("hand weights not loaded");
        size_t maxpix = 0;
        for (int s = 0; s < ns; ++s) maxpix = std::max(maxpix, (size_t)gs[0][s].Hp * gs[0][s].Wp);
        const int chunk = (int)std::max<size_t>(1, (((size_t)1 << 31) - 1) / (3 * 128 * maxpix));
        // size every per-crop buffer for the largest crop / all crops up front: a reallocation
        // after the first batch would drop the results of the crops already done
        const int wmax = *std::max_element(sizes, sizes + n);
        h->avg.ensure<double>((size_t)21 * wmax * wmax, h->stream);
        h->hlab.ensure<int>((size_t)21 * wmax * wmax, h->stream);
        h->hsums.ensure<double>((size_t)21 * wmax * wmax, h->stream);
        if (!(flags & OPOSE_OUT_DEVICE)) {
            h->hpeaks.ensure<double>((size_t)n * 21 * 3, h->stream);
            h->hfound.ensure<int>((size_t)n * 21, h->stream);
        }
        for (int c0 = 0; c0 < n; c0 += chunk) {
            const int nc = std::min(chunk, n - c0);
            std::vector<NetSeg> segs;
            for (int s = 0; s < ns; ++s) {
                const ScaleGeom& g0 = gs[0][s];
                float* x = h->ws[lockstep ? s : h->slot].x.ensure<float>((size_t)nc * 3 * g0.Hp * g0.Wp, h->stream);
                ProfEntry pe;
                h->prof_begin(pe, "preprocess", 0, 0);
                for (int i = c0; i < c0 + nc; ++i) {
                    const ScaleGeom& g = gs[i][s];
                    const uint8_t* src = buf ? buf + off[i] : crops[i];
                    preprocess_scale(src, (int64_t)(off[i + 1] - off[i]), row_strides[i], 1, sizes[i], sizes[i], g, p,
                                     x + (size_t)(i - c0) * 3 * g.Hp * g.Wp, h->stream);
                }
                h->prof_end(pe);
                if (lockstep) {
                    segs.push_back(NetSeg{x, nc, g0.Hp, g0.Wp, s});
                    continue;
                }
                float* Sb = net_forward(h, OPOSE_NET_HAND, x, nc, g0.Hp, g0.Wp);
                upsample_to_mid(h, s, Sb, 150, nc, g0, 21);
            }
            if (lockstep) {
                const std::vector<float*> outs = net_forward_x6(h, OPOSE_NET_HAND, segs);
                for (int s = 0; s < ns; ++s) upsample_to_mid(h, s, outs[s], 150, nc, gs[0][s], 21);
            }
            for (int i = c0; i < c0 + nc; ++i)
                hand_post_common(h, 1, sizes[i], sizes[i], gs[i], p, peaks, found, flags & OPOSE_OUT_DEVICE, i - c0, i);
        }
        hand_finish(h, n, peaks, found, flags & OPOSE_OUT_DEVICE);
    });
    return OPOSE_OK;
}

int opose_hand_post(opose_t* h, const float* const* maps, const int* hl, const int* wl, const int* pad_down,
                    const int* pad_right, int n_scales, int N, int H, int W, const opose_params* pp,
                    double* peaks, int32_t* found, int flags) {
    if (!h || !maps || !hl || !wl || !pad_down || !pad_right || !peaks || !found || N <= 0 || H <= 0 || W <= 0 ||
        n_scales < 1 || n_scales > OPOSE_MAX_SCALES)
        return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        opose_params p = fill_params(pp, OPOSE_NET_HAND);
        std::vector<ScaleGeom> gs;
        for (int s = 0; s < n_scales; ++s) {
            const ScaleGeom g = geom_from_pads(hl[s], wl[s], pad_down[s], pad_right[s], H, W);
            if (g.Hs <= 0 || g.Ws <= 0) throw std::invalid_argument("bad pad");
            const float* md = stage_maps(h, maps[s], (size_t)N * 22 * g.hl * g.wl, flags);
            upsample_to_mid(h, s, md, 22, N, g, 21);
            gs.push_back(g);
        }
        hand_post_common(h, N, H, W, gs, p, peaks, found, flags & OPOSE_OUT_DEVICE);
        hand_finish(h, N, peaks, found, flags & OPOSE_OUT_DEVICE);
    });
    return OPOSE_OK;
}

// ---- drawing (src/util.py:44-77, srcmx/utilmx.py:212-227, srcmx/MotionEstimation.py:281-295) ----
// grid z runs over the frames; the coordinate bound of the pixel rule covers the frame size
bool opose::draw_dims_ok(int N, int H, int W) {
    return N > 0 && N <= 32767 && H > 0 && W > 0 && H <= 16384 && W <= 16384;
}

// primitive slots per frame: 18 discs + 17 limbs per person of a record at the handle's capacity
// (joints 0) or of the one person of a MotionMat row, and 20 edges + 21 discs per hand
int opose::draw_cap(const opose_ctx* h, int joints) { return joints == 0 ? 35 * h->maxp : (joints == 60 ? 117 : 35); }

void opose::run_draw_setup(opose_ctx* h, const uint8_t* rec_dev, const double* motion_dev, int joints, int N, int H,
                           int W, int32_t* prims, int32_t* counts, int32_t* status_dev) {
    const int cap = draw_cap(h, joints);
    ProfEntry pe;
    h->prof_begin(pe, "draw_setup", 0, (double)N * cap * (kDrawPrimInts * 4 + 48));
    launch_draw_setup(rec_dev, make_record_layout(h->ppp, h->maxp), motion_dev, joints, N, H, W, cap, prims, counts,
                      status_dev, h->stream);
    h->prof_end(pe);
}

// The two launches of a draw call on staged sources (device records, or device rows of `joints`
// joints) and what surrounds them: the frames staged like every frame entry point's, the canvases
// in the caller's device memory, or in the handle's and copied to the host.  out == bgr in one
// memory space draws in place.  Every buffer is sized before anything is enqueued.
static int run_draw(opose_ctx* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride, int64_t frame_stride,
                    const uint8_t* rec_dev, const double* motion_dev, int joints, uint8_t* out, int32_t* status,
                    int flags) {
    const bool id = flags & OPOSE_IN_DEVICE, od = flags & OPOSE_OUT_DEVICE;
    const bool inplace = out == bgr && id == od;
    const int cap = draw_cap(h, joints);
    const size_t dense = (size_t)N * H * W * 3;
    int32_t* prims = h->draw_prims.ensure<int32_t>((size_t)N * cap * kDrawPrimInts, h->stream);
    int32_t* counts = h->draw_counts.ensure<int32_t>((size_t)N, h->stream);
    int32_t* sd = od ? status : h->draw_status.ensure<int32_t>((size_t)N, h->stream);
    uint8_t* canvas = inplace ? nullptr : (od ? out : h->draw_out.ensure<uint8_t>(dense, h->stream));
    const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, flags);
    int64_t crs = (int64_t)W * 3, cfs = crs * H;
    if (inplace) {  // the caller's device frames, or their staged copy
        canvas = const_cast<uint8_t*>(fd);
        crs = row_stride;
        cfs = frame_stride;
    }
    run_draw_setup(h, rec_dev, motion_dev, joints, N, H, W, prims, counts, sd);
    ProfEntry pe;
    h->prof_begin(pe, "draw_pixels", 0, 2.0 * (double)dense);
    launch_draw_pixels(fd, frame_stride, row_stride, canvas, cfs, crs, N, H, W, prims, counts, cap, h->stream);
    h->prof_end(pe);
    if (od) {
        h->prof_drain();
        return OPOSE_OK;
    }
    if (!inplace) {
        OPOSE_HIP_CHECK(hipMemcpyAsync(out, canvas, dense, hipMemcpyDeviceToHost, h->stream));
    } else if (frame_stride == row_stride * H) {  // rows only: the bytes between them are the caller's
        OPOSE_HIP_CHECK(hipMemcpy2DAsync(out, row_stride, canvas, row_stride, (size_t)W * 3, (size_t)N * H,
                                         hipMemcpyDeviceToHost, h->stream));
    } else {
        for (int n = 0; n < N; ++n)
            OPOSE_HIP_CHECK(hipMemcpy2DAsync(out + (size_t)n * frame_stride, row_stride, canvas + (size_t)n * frame_stride,
                                             row_stride, (size_t)W * 3, H, hipMemcpyDeviceToHost, h->stream));
    }
    const int worst = worst_slot_status(h, sd, N, status);
    h->prof_drain();
    if (worst != OPOSE_OK) h->err = "a frame's record carries a status, indexes past its candidates, or a coordinate is out of range";
    return worst;
}

int opose_draw_records(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride, int64_t frame_stride,
                       const void* records, uint8_t* out, int32_t* status, int flags) {
    if (!h || !bgr || !records || !out || !status || !draw_dims_ok(N, H, W)) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    if (reinterpret_cast<uintptr_t>(records) % 8) return OPOSE_E_ARG;  // float64 rows at offset 16
    OPOSE_TRY(h, {
        enter_main(h);
        const uint8_t* rd = stage_values(h, h->records, static_cast<const uint8_t*>(records),
                                         make_record_layout(h->ppp, h->maxp).bytes * N, flags & OPOSE_IN_DEVICE);
        return run_draw(h, bgr, N, H, W, row_stride, frame_stride, rd, nullptr, 0, out, status, flags);
    });
}

int opose_draw_motion(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride, int64_t frame_stride,
                      const double* motion, int joints, uint8_t* out, int32_t* status, int flags) {
    if (!h || !bgr || !motion || !out || !status || !draw_dims_ok(N, H, W)) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    if (joints != 18 && joints != 60) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const double* md = stage_values(h, h->draw_motion, motion, (size_t)N * joints * 3, flags & OPOSE_IN_DEVICE);
        return run_draw(h, bgr, N, H, W, row_stride, frame_stride, nullptr, md, joints, out, status, flags);
    });
}

