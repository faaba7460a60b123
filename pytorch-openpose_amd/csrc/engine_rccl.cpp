// engine_rccl.cpp — libopose's RCCL loader and the entry points of the row-band halo exchange.
#include "engine.h"

namespace opose {

// the RCCL entry points (engine.h Rccl), resolved on first use
const Rccl& rccl() {
    static const Rccl r = [] {
        void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error("RCCL (librccl.so) not found");
        auto sym = [&](const char* n) {
            void* f = dlsym(lib, n);
            if (!f) throw std::runtime_error(std::string("RCCL without ") + n);
            return f;
        };
        Rccl x;
        x.get_unique_id = reinterpret_cast<decltype(x.get_unique_id)>(sym("ncclGetUniqueId"));
        x.comm_init_rank = reinterpret_cast<decltype(x.comm_init_rank)>(sym("ncclCommInitRank"));
        x.comm_destroy = reinterpret_cast<decltype(x.comm_destroy)>(sym("ncclCommDestroy"));
        x.comm_abort = reinterpret_cast<decltype(x.comm_abort)>(sym("ncclCommAbort"));
        x.send = reinterpret_cast<decltype(x.send)>(sym("ncclSend"));
        x.recv = reinterpret_cast<decltype(x.recv)>(sym("ncclRecv"));
        x.group_start = reinterpret_cast<decltype(x.group_start)>(sym("ncclGroupStart"));
        x.group_end = reinterpret_cast<decltype(x.group_end)>(sym("ncclGroupEnd"));
        x.error_string = reinterpret_cast<decltype(x.error_string)>(sym("ncclGetErrorString"));
        x.async_error = reinterpret_cast<decltype(x.async_error)>(sym("ncclCommGetAsyncError"));
        return x;
    }();
    return r;
}
void rccl_check(ncclResult_t r) {
    if (r != ncclSuccess) throw std::runtime_error(std::string("RCCL: ") + rccl().error_string(r));
}

}  // namespace opose

using namespace opose;

int opose_rccl_unique_id(void* id, size_t len) {
    if (!id || len < sizeof(ncclUniqueId)) return OPOSE_E_ARG;
    try {
        ncclUniqueId u;
        rccl_check(rccl().get_unique_id(&u));
        std::memcpy(id, &u, sizeof(u));
        return OPOSE_OK;
    } catch (const std::exception&) {
        return OPOSE_E_HIP;
    }
}

int opose_rccl_init(opose_t* h, const void* id, int rank, int nranks) {
    if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        if (h->comm) {
            rccl_check(rccl().comm_destroy(h->comm));
            h->comm = nullptr;
        }
        ncclUniqueId u;
        std::memcpy(&u, id, sizeof(u));
        rccl_check(rccl().comm_init_rank(&h->comm, nranks, u, rank));
        return OPOSE_OK;
    });
}

int opose_rccl_abort(opose_t* h) {
    if (!h) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        if (h->comm) {
            ncclComm_t c = h->comm;
            h->comm = nullptr;
            h->band_up = h->band_dn = -1;
            rccl_check(rccl().comm_abort(c));
        }
        return OPOSE_OK;
    });
}

int opose_rccl_wait(opose_t* h, int timeout_ms) {
    if (!h || timeout_ms < 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(h->stream);
            if (q == hipSuccess) return OPOSE_OK;
            if (q != hipErrorNotReady) OPOSE_HIP_CHECK(q);
            ncclResult_t ae = ncclSuccess;
            if (h->comm) rccl_check(rccl().async_error(h->comm, &ae));
            const bool late = std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms);
            if ((ae != ncclSuccess && ae != ncclInProgress) || late) {
                // a band neighbour failed or never arrived: abort this rank's communicator, which
                // raises RCCL's abort flag that the queued send / recv kernels poll, so this rank's
                // stream drains instead of waiting on a peer that will not come
                if (h->comm) {
                    ncclComm_t c = h->comm;
                    h->comm = nullptr;
                    h->band_up = h->band_dn = -1;
                    (void)rccl().comm_abort(c);
                }
                h->err = late ? "RCCL halo exchange: no progress within the deadline (communicator aborted)"
                              : std::string("RCCL halo exchange: ") + rccl().error_string(ae) + " (communicator aborted)";
                return late ? OPOSE_E_TIMEOUT : OPOSE_E_HIP;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    });
}

int opose_set_band_peers(opose_t* h, int up, int dn) {
    if (!h) return OPOSE_E_ARG;
    h->band_up = up;
    h->band_dn = dn;
    return OPOSE_OK;
}

