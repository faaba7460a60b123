// engine.cpp — libopose host runtime: the handle (stream pool, profiling, lifetime) and the entry
// points that manage it.  The rest of the runtime: engine_weights.cpp (topology, weight packing),
// engine_plan.cpp (conv launch planning), engine_net.cpp (network drivers), engine_post.cpp
// (post-network drivers), engine_api.cpp (graph cache, pipelining, inference entry points),
// engine_rccl.cpp, engine_debug.cpp (test hooks); engine.h holds what they share.
//
// Mirrors hitmaxiang/pytorch-openpose:
//  * topology + state_dict order      src/model.py:25-104 (body), :136-195 (hand)
//  * Body.__call__ orchestration      src/body.py:24-212
//  * Hand.__call__ orchestration      src/hand.py:25-75
// The network runs as one launch per layer of the split-bf16 implicit-GEMM kernels (conv_win.hip,
// conv_x6.hip, conv1x1_chain.hip; conv.hip is the fp32 alternative): the two CPM branches of a
// stage and the scales of a pyramid share a launch as groups, each conv sums a pixel in an order
// fixed by its layer (k slabs, slab_count); stage concatenation is implicit (channel-slice writes).
#include "engine.h"

namespace opose {

bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return dflt ? !(e && e[0] == '0') : e && e[0] == '1';
}

// ---------------------------------------------------------------- streams
// Streams come from a process-wide pool and go back to it when a handle is destroyed (drained
// first), so test suites and services that create and destroy handles do not churn HIP streams.
struct StreamPool {
    std::mutex mu;
    std::map<std::pair<int, int>, std::vector<hipStream_t>> free;  // (device, priority) -> streams
};
static StreamPool& stream_pool() {
    static StreamPool* p = new StreamPool();  // never destroyed: handles may outlive static teardown
    return *p;
}
hipError_t pooled_stream(hipStream_t* s, int priority) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> g(stream_pool().mu);
        auto& v = stream_pool().free[{dev, priority}];
        if (!v.empty()) {
            *s = v.back();
            v.pop_back();
            return hipSuccess;
        }
    }
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority);
}
static void return_stream(hipStream_t s, int device, int priority) {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    std::lock_guard<std::mutex> g(stream_pool().mu);
    stream_pool().free[{device, priority}].push_back(s);
}

// Bumped whenever device memory that a captured hipGraph may reference is (re)allocated:
// graphs captured under an older epoch are dropped instead of replayed.
std::atomic<uint64_t> g_alloc_epoch{1};

static hipEvent_t lazy_event(hipEvent_t& e) {
    if (!e) OPOSE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return e;
}

}  // namespace opose

using namespace opose;

hipEvent_t opose_ctx::get_event() {
    if (!event_pool.empty()) {
        hipEvent_t e = event_pool.back();
        event_pool.pop_back();
        return e;
    }
    // timing-only events: no system-scope fence on record (no L2 writeback / invalidate
    // between the bracketed launches; only hipEventElapsedTime reads them)
    hipEvent_t e;
    OPOSE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    return e;
}
void opose_ctx::prof_begin(ProfEntry& pe, const char* cls, double flops, double bytes) {
    if (!prof || (prof_conv7_only && std::strcmp(cls, "conv7x7") != 0)) return;
    pe.cls = cls;
    pe.flops = flops;
    pe.bytes = bytes;
    pe.e0 = get_event();
    pe.e1 = get_event();
    OPOSE_HIP_CHECK(hipEventRecord(pe.e0, stream));
}
void opose_ctx::prof_end(ProfEntry& pe) {
    if (!prof || !pe.e0) return;
    OPOSE_HIP_CHECK(hipEventRecord(pe.e1, stream));
    pending.push_back(pe);
}
// fold finished event pairs into agg; non-blocking (stops at the first unfinished pair, so a
// call does not wait for its own kernels) unless `all`
void opose_ctx::prof_drain(bool all) {
    size_t done = 0;
    for (auto& pe : pending) {
        if (!all && hipEventQuery(pe.e1) != hipSuccess) break;
        ++done;
        OPOSE_HIP_CHECK(hipEventSynchronize(pe.e1));
        float ms = 0;
        OPOSE_HIP_CHECK(hipEventElapsedTime(&ms, pe.e0, pe.e1));
        for (const std::string* key : {&pe.cls, &pe.detail}) {
            if (key->empty() || (key == &pe.detail && !detail)) continue;
            auto& a = agg[*key];
            a.count++;
            a.ms += ms;
            a.flops += pe.flops;
            a.bytes += pe.bytes;
        }
        event_pool.push_back(pe.e0);
        event_pool.push_back(pe.e1);
    }
    pending.erase(pending.begin(), pending.begin() + done);
}

void opose_ctx::release() {
    // drain every stream first, then the graph executables (they may reference the scale
    // streams' captured work), then streams, events and memory
    if (stream) (void)hipStreamSynchronize(stream);
    if (nstream) (void)hipStreamSynchronize(nstream);
    for (int i = 0; i < kMaxScales; ++i)
        if (sstream[i]) (void)hipStreamSynchronize(sstream[i]);
    for (auto& kv : graphs)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    graphs.clear();
    return_stream(nstream, device, nstream_prio);
    for (hipEvent_t e : {ev_net, ev_main, ev_post[0], ev_post[1], ev_ext, ev_sig, ev_in, ev_fork})
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < kMaxScales; ++i) {
        return_stream(sstream[i], device, 0);
        if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
    }
    for (int* p : sched_mem) (void)hipFree(p);
    for (auto e : event_pool) (void)hipEventDestroy(e);
    return_stream(own_stream, device, 0);
}

opose_ctx::~opose_ctx() {
    if (comm) (void)rccl().comm_destroy(comm);
    release();
}

void opose_default_params(int net, opose_params* p) {
    std::memset(p, 0, sizeof(*p));
    if (net == OPOSE_NET_HAND) {
        p->n_scales = 4;
        p->scales[0] = 0.5;
        p->scales[1] = 1.0;
        p->scales[2] = 1.5;
        p->scales[3] = 2.0;
    } else {
        p->n_scales = 1;
        p->scales[0] = 0.5;
    }
    p->boxsize = 368;
    p->stride = 8;
    p->pad_value = 128;
    p->thre1 = 0.1;
    p->thre2 = 0.05;
    p->thre_hand = 0.03;
}

int opose_create(int device, opose_t** out) {
    if (!out) return OPOSE_E_ARG;
    *out = nullptr;
    auto* h = new opose_ctx();
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || pooled_stream(&h->own_stream, 0) != hipSuccess) {
        delete h;
        return OPOSE_E_HIP;
    }
    h->stream = h->own_stream;
    *out = h;
    return OPOSE_OK;
}

void opose_destroy(opose_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)opose_flush(h);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

const char* opose_last_error(const opose_t* h) { return h ? h->err.c_str() : "null handle"; }

int opose_set_stream(opose_t* h, void* s) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        flush_post(h);
        const hipStream_t ns = s ? static_cast<hipStream_t>(s) : h->own_stream;
        if (ns != h->stream) {
            // work still queued on the old stream (and on the pipelined network stream) uses the
            // workspace the new stream's calls reuse: order the new stream after both
            hipEvent_t e = lazy_event(h->ev_sig);
            OPOSE_HIP_CHECK(hipEventRecord(e, h->stream));
            OPOSE_HIP_CHECK(hipStreamWaitEvent(ns, e, 0));
            if (h->nstream) {
                OPOSE_HIP_CHECK(hipEventRecord(e, h->nstream));
                OPOSE_HIP_CHECK(hipStreamWaitEvent(ns, e, 0));
            }
            h->stream = ns;
            h->main_dirty = true;  // the next pipelined network waits for the new stream
        }
    });
    return OPOSE_OK;
}

int opose_wait_stream(opose_t* h, void* s) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        const hipStream_t xs = static_cast<hipStream_t>(s);
        // Both library streams must come after `xs`: the handle's stream directly (nothing to do
        // when `xs` is that stream), the pipelined network stream through the event even then --
        // back-to-back pipelined calls do not otherwise order it after the handle's stream.
        // Before the network stream exists, the first pipelined call orders it after the
        // handle's stream (main_dirty), which by then has waited on every such `xs`.
        hipEvent_t e = lazy_event(h->ev_ext);
        OPOSE_HIP_CHECK(hipEventRecord(e, xs));
        if (xs != h->stream) OPOSE_HIP_CHECK(hipStreamWaitEvent(h->stream, e, 0));
        if (h->nstream) {
            if (xs != h->nstream) OPOSE_HIP_CHECK(hipStreamWaitEvent(h->nstream, e, 0));
        } else {
            h->main_dirty = true;
        }
    });
    return OPOSE_OK;
}

int opose_signal_stream(opose_t* h, void* s) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        flush_post(h);
        const hipStream_t xs = static_cast<hipStream_t>(s);
        if (xs == h->stream) return OPOSE_OK;
        hipEvent_t e = lazy_event(h->ev_sig);
        OPOSE_HIP_CHECK(hipEventRecord(e, h->stream));
        OPOSE_HIP_CHECK(hipStreamWaitEvent(xs, e, 0));
    });
    return OPOSE_OK;
}

int opose_signal_input(opose_t* h, void* s) {
    if (!h) return OPOSE_E_ARG;
    // Since the last entry point that queued work on the handle's stream (main_dirty), only
    // OPOSE_PIPELINE calls ran, and each read its device inputs on the network stream only (its
    // post-network part reads the mid buffers).  That stream waited for the handle's stream when
    // main_dirty was last cleared, so an event on it after the last network covers every input
    // read so far.  Otherwise the handle's stream holds input reads: opose_signal_stream.
    if (!h->nstream || h->main_dirty) return opose_signal_stream(h, s);
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        const hipStream_t xs = static_cast<hipStream_t>(s);
        if (xs == h->nstream) return OPOSE_OK;
        hipEvent_t e = lazy_event(h->ev_in);
        OPOSE_HIP_CHECK(hipEventRecord(e, h->nstream));
        OPOSE_HIP_CHECK(hipStreamWaitEvent(xs, e, 0));
    });
    return OPOSE_OK;
}

void* opose_get_stream(const opose_t* h) { return h ? h->stream : nullptr; }

int opose_flush(opose_t* h) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        flush_post(h);
    });
    return OPOSE_OK;
}

int opose_synchronize(opose_t* h) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        flush_post(h);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (h->nstream) OPOSE_HIP_CHECK(hipStreamSynchronize(h->nstream));
    });
    return OPOSE_OK;
}

int opose_set_capacity(opose_t* h, int ppp, int maxp) {
    if (!h || ppp < 1 || maxp < 1 || ppp > kMaxPeaksPerPart || maxp > kMaxPeople) return OPOSE_E_ARG;
    if (opose_flush(h) != OPOSE_OK) return OPOSE_E_HIP;
    h->ppp = ppp;
    h->maxp = maxp;
    return OPOSE_OK;
}

size_t opose_body_record_bytes(const opose_t* h) { return h ? make_record_layout(h->ppp, h->maxp).bytes : 0; }

int opose_profile_enable(opose_t* h, int enable) {
    if (!h) return OPOSE_E_ARG;
    h->prof = enable != 0;
    h->detail = enable == 2;
    h->prof_conv7_only = enable == 3;
    return OPOSE_OK;
}

int opose_profile_reset(opose_t* h) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, h->prof_drain(true));
    h->agg.clear();
    return OPOSE_OK;
}

int opose_profile_read(opose_t* h, char* buf, size_t len) {
    if (!h || !buf || !len) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (h->nstream) OPOSE_HIP_CHECK(hipStreamSynchronize(h->nstream));
        h->prof_drain(true);
    });
    std::string s = "{";
    bool first = true;
    for (auto& kv : h->agg) {
        char tmp[512];
        std::snprintf(tmp, sizeof tmp, "%s\"%s\":{\"count\":%ld,\"ms\":%.6f,\"flops\":%.6e,\"bytes\":%.6e}",
                      first ? "" : ",", kv.first.c_str(), kv.second.count, kv.second.ms, kv.second.flops,
                      kv.second.bytes);
        s += tmp;
        first = false;
    }
    s += "}";
    if (s.size() + 1 > len) return OPOSE_E_ARG;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return OPOSE_OK;
}
