// engine_shapelet.cpp — the shapelet search entry points: validation of the ragged batch, the block
// table of the candidate starts, chunking, and the launches of shapelet.hip; and the scan of whole
// streams for many patterns (its pattern table, chunks and occurrence outputs); and the training of
// the learned shapelet models (shapelet_net.hip: its checks, staged state and the epoch loop).
#include "engine.h"

namespace opose {

// The ragged batch of a window call: off[0] = 0, non-decreasing, every sequence at least m rows, all
// within the limits of shapelet.h.  Nothing is launched unless this returns OPOSE_OK.
static int shp_check(opose_ctx* h, const int64_t* off, int n_seq, int D, int m) {
    if (n_seq < 1 || D < 1 || m < 1 || off[0] != 0) {
        h->err = "shapelet: n_seq, D and m must be positive and off[0] must be 0";
        return OPOSE_E_ARG;
    }
    if (n_seq > kShpMaxSeq || D > kShpMaxD || m > kShpMaxM) {
        h->err = "shapelet: n_seq, D or m beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    for (int j = 0; j < n_seq; ++j)
        if (off[j + 1] < off[j]) {
            h->err = "shapelet: off must not decrease";
            return OPOSE_E_ARG;
        }
    if (off[n_seq] > kShpMaxRows) {
        h->err = "shapelet: too many rows";
        return OPOSE_E_SHAPE;
    }
    for (int j = 0; j < n_seq; ++j)
        if (off[j + 1] - off[j] < m) {
            h->err = "shapelet: a sequence is shorter than the window";
            return OPOSE_E_SHAPE;
        }
    return OPOSE_OK;
}

// The candidate starts of the sequences `cands` (in the order given, r ascending) as table entries
// of at most kShpTR starts, grouped into chunks of at most `cap` candidates; an entry's out0 counts
// from its chunk's first candidate.  chunks: per chunk {first entry, entries, candidates}.
struct ShpChunk {
    int b0, nb, nc;
};
static int64_t shp_table(const int64_t* off, int m, const std::vector<int>& cands, int64_t cap,
                         std::vector<ShpBlock>& blocks, std::vector<ShpChunk>& chunks) {
    int64_t total = 0;
    ShpChunk cur{0, 0, 0};
    for (int i : cands) {
        const int P = (int)(off[i + 1] - off[i]) - m + 1;
        for (int r = 0; r < P;) {
            if (cur.nc == cap) {
                chunks.push_back(cur);
                cur = ShpChunk{(int)blocks.size(), 0, 0};
            }
            const int n = (int)std::min<int64_t>(std::min(kShpTR, P - r), cap - cur.nc);
            blocks.push_back(ShpBlock{i, r, n, cur.nc});
            cur.nb++;
            cur.nc += n;
            r += n;
            total += n;
        }
    }
    if (cur.nc) chunks.push_back(cur);
    return total;
}

template <class T>
static const T* shp_stage(opose_ctx* h, DevBuf& buf, const T* v, size_t n, bool in_device) {
    if (in_device) return v;
    T* d = buf.ensure<T>(n, h->stream);
    OPOSE_HIP_CHECK(hipMemcpyAsync(d, v, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return d;
}

// a host table the call built itself: on the device before the table goes out of scope
template <class T>
static const T* shp_upload(opose_ctx* h, DevBuf& buf, const std::vector<T>& v) {
    T* d = buf.ensure<T>(v.size(), h->stream);
    OPOSE_HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return d;
}

// The window lengths of a call: 1 .. kShpMaxLens of them, each at least 1, strictly ascending.
// (shp_check on the last length holds the rest: its limit, and every sequence that long.)
static int shp_lens_check(opose_ctx* h, const int32_t* m_lens, int n_lens, ShpLens* lens) {
    if (n_lens < 1) {
        h->err = "shapelet: at least one window length";
        return OPOSE_E_ARG;
    }
    if (n_lens > kShpMaxLens) {
        h->err = "shapelet: more window lengths than one call supports";
        return OPOSE_E_SHAPE;
    }
    *lens = ShpLens{};
    lens->n = n_lens;
    for (int l = 0; l < n_lens; ++l) {
        if (m_lens[l] < 1 || (l && m_lens[l] <= m_lens[l - 1])) {
            h->err = "shapelet: window lengths must be positive and strictly ascending";
            return OPOSE_E_ARG;
        }
        lens->m[l] = m_lens[l];
    }
    return OPOSE_OK;
}

// the starts of table entry b that are valid at window length m: its first so many
static int shp_valid_at(const int64_t* off, const ShpBlock& b, int m) {
    const int64_t P = off[b.seq + 1] - off[b.seq] - m + 1;
    return (int)std::min<int64_t>(std::max<int64_t>(P - b.r0, 0), b.nvalid);
}

static void run_mindist(opose_ctx* h, const float* seq, const int64_t* off, int n_seq, int D, const ShpLens& lens,
                        const ShpBlock* blocks, const ShpLenRows* rows, int nb, int nc, int64_t L, float* min2,
                        int32_t* loc) {
    ProfEntry pe;
    const int mx = lens.m[lens.n - 1];
    h->prof_begin(pe, "shapelet_mindist", 3.0 * nc * (double)(L - (int64_t)n_seq * (mx - 1)) * D,
                  8.0 * nc * n_seq * lens.n);
    launch_shapelet_mindist(seq, off, n_seq, D, lens, blocks, rows, nb, min2, loc, h->stream);
    h->prof_end(pe);
}

static void run_score(opose_ctx* h, const float* min2, int nc, int n_seq, int n_labels, const uint8_t* labels, int negs,
                      int32_t* num, double* loss) {
    ProfEntry pe;
    h->prof_begin(pe, "shapelet_score", 0, 4.0 * nc * n_seq);
    launch_shapelet_score(min2, nc, n_seq, n_labels, labels, negs, num, loss, h->stream);
    h->prof_end(pe);
}

static void run_select(opose_ctx* h, const int32_t* num, const double* loss, int nc, const ShpBlock* blocks, int nb,
                       const float* min2, const int32_t* loc, int n_seq, int first, int32_t* best, double* best_loss,
                       float* dis, int32_t* locs) {
    ProfEntry pe;
    h->prof_begin(pe, "shapelet_select", 0, 12.0 * nc);
    launch_shapelet_select(num, loss, nc, blocks, nb, min2, loc, n_seq, first, best, best_loss, dis, locs, h->stream);
    h->prof_end(pe);
}

// labels: n_labels values 0 / 1 for n_seq = n_labels or 2 * n_labels sequences; negs: the zeros
static int shp_labels_check(opose_ctx* h, const uint8_t* labels, int n_labels, int n_seq, int* negs) {
    if (n_labels < 1 || (n_seq != n_labels && n_seq != 2 * (int64_t)n_labels)) {
        h->err = "shapelet: n_seq must be n_labels or 2 * n_labels";
        return OPOSE_E_ARG;
    }
    if (n_labels > kShpMaxSeq) {
        h->err = "shapelet: too many labels";
        return OPOSE_E_SHAPE;
    }
    *negs = 0;
    for (int k = 0; k < n_labels; ++k) {
        if (labels[k] > 1) {
            h->err = "shapelet: labels must be 0 or 1";
            return OPOSE_E_ARG;
        }
        *negs += labels[k] == 0;
    }
    return OPOSE_OK;
}

// Where shapelet_select keeps the winners of nl window lengths over ns sequences.  With host outputs
// that is one workspace block,
//   int32 best[nl][4] | double best_loss[nl] | float dis[nl][ns] | int32 locs[nl][ns]
// (best_loss on a multiple of 8 bytes); with device outputs, the caller's four arrays.
struct ShpWinners {
    size_t nl, ns;
    int32_t* best;
    double* loss;
    float* dis;
    int32_t* locs;
    static size_t bytes(size_t nl, size_t ns) { return nl * (24 + 8 * ns); }
    static ShpWinners in_block(uint8_t* block, size_t nl, size_t ns) {
        return ShpWinners{nl,
                          ns,
                          reinterpret_cast<int32_t*>(block),
                          reinterpret_cast<double*>(block + 16 * nl),
                          reinterpret_cast<float*>(block + 24 * nl),
                          reinterpret_cast<int32_t*>(block + (24 + 4 * ns) * nl)};
    }
    // queued on the stream; the caller synchronises
    void to_host(opose_ctx* h, int32_t* hbest, double* hloss, float* hdis, int32_t* hlocs) const {
        OPOSE_HIP_CHECK(hipMemcpyAsync(hbest, best, 16 * nl, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(hloss, loss, 8 * nl, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(hdis, dis, 4 * nl * ns, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(hlocs, locs, 4 * nl * ns, hipMemcpyDeviceToHost, h->stream));
    }
};

}  // namespace opose

using namespace opose;

int opose_motion_features(opose_t* h, const double* motion, const int64_t* off, int n_seq, int joints, int featuremode,
                          float* out, int flags) {
    if (!h || !motion || !off || !out || n_seq < 1) return OPOSE_E_ARG;
    if ((joints != 18 && joints != 60) || featuremode < 0 || featuremode > 2 || off[0] != 0) return OPOSE_E_ARG;
    for (int j = 0; j < n_seq; ++j)
        if (off[j + 1] < off[j]) return OPOSE_E_ARG;
    const int64_t L = off[n_seq];
    if (L < 1) return OPOSE_E_ARG;
    if (L > kShpMaxRows) return OPOSE_E_SHAPE;
    OPOSE_TRY(h, {
        enter_main(h);
        const bool od = flags & OPOSE_OUT_DEVICE;
        const int F = joints == 18 ? 6 : 46;
        const size_t nblocks = (size_t)((L + kFeatRows - 1) / kFeatRows);
        const double* md = shp_stage(h, h->shp_in, motion, (size_t)L * joints * 3, flags & OPOSE_IN_DEVICE);
        const int64_t* offd = shp_stage(h, h->shp_off, off, (size_t)n_seq + 1, false);
        int32_t* carry = h->shp_carry.ensure<int32_t>(nblocks * 2 * joints, h->stream);
        float* outd = od ? out : h->shp_out.ensure<float>((size_t)L * F * 2, h->stream);
        ProfEntry pe;
        h->prof_begin(pe, "motion_features", 0, (double)L * (joints * 24.0 + F * 8.0));
        launch_motion_features(md, L, joints, offd, n_seq, featuremode, carry, outd, h->stream);
        h->prof_end(pe);
        if (!od) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(out, outd, (size_t)L * F * 8, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_sliding_distance(opose_t* h, const float* pattern, int m, const float* seq, const int64_t* off, int n_seq,
                           int D, float* dist, int flags) {
    if (!h || !pattern || !seq || !off || !dist) return OPOSE_E_ARG;
    if (const int rc = shp_check(h, off, n_seq, D, m)) return rc;
    OPOSE_TRY(h, {
        enter_main(h);
        const bool id = flags & OPOSE_IN_DEVICE, od = flags & OPOSE_OUT_DEVICE;
        const int64_t L = off[n_seq];
        const size_t n_out = (size_t)(L - (int64_t)n_seq * (m - 1));
        const float* sd = shp_stage(h, h->shp_seq, seq, (size_t)L * D, id);
        const float* pd = shp_stage(h, h->shp_in, pattern, (size_t)m * D, id);
        const int64_t* offd = shp_stage(h, h->shp_off, off, (size_t)n_seq + 1, false);
        float* outd = od ? dist : h->shp_out.ensure<float>(n_out, h->stream);
        ProfEntry pe;
        h->prof_begin(pe, "sliding_distance", 3.0 * n_out * m * D, 4.0 * n_out * m * D);
        launch_sliding_distance(pd, m, sd, offd, n_seq, D, L, outd, h->stream);
        h->prof_end(pe);
        if (!od) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(dist, outd, n_out * 4, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

// One window length is a list of one: the checks, in their order, and the outputs are those of the
// several-lengths calls below.
int opose_shapelet_mindist(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int m,
                           const int32_t* cand_seqs, int n_cand_seqs, float* min2, int32_t* loc, int flags) {
    const int32_t one = m;
    return opose_shapelet_mindist_lengths(h, seq, off, n_seq, D, &one, 1, cand_seqs, n_cand_seqs, min2, loc, flags);
}

int opose_debug_shapelet_score(opose_t* h, const float* min2, int n_cand, int n_seq, const uint8_t* labels,
                               int n_labels, int32_t* num, double* loss, int32_t* winner, double* win_loss) {
    if (!h || !min2 || !labels || !num || !loss || !winner || !win_loss || n_cand < 1) return OPOSE_E_ARG;
    int negs = 0;
    if (const int rc = shp_labels_check(h, labels, n_labels, n_seq, &negs)) return rc;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf mb, lb, yb, nb, sb, bb, tb;
        const size_t n = (size_t)n_cand * n_seq;
        float* md = mb.ensure<float>(n, h->stream);
        int32_t* ld = lb.ensure<int32_t>(n, h->stream);
        uint8_t* yd = yb.ensure<uint8_t>((size_t)n_labels, h->stream);
        int32_t* nd = nb.ensure<int32_t>((size_t)n_cand, h->stream);
        double* sd = sb.ensure<double>((size_t)n_cand, h->stream);
        const ShpWinners w = ShpWinners::in_block(bb.ensure<uint8_t>(ShpWinners::bytes(1, n_seq), h->stream), 1, n_seq);
        OPOSE_HIP_CHECK(hipMemcpyAsync(md, min2, n * 4, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(ld, 0, n * 4, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(yd, labels, (size_t)n_labels, hipMemcpyHostToDevice, h->stream));
        // one table entry for all rows: the winner's "start" is its row
        const std::vector<ShpBlock> one{ShpBlock{0, 0, n_cand, 0}};
        const ShpBlock* bd = shp_upload(h, tb, one);
        run_score(h, md, n_cand, n_seq, n_labels, yd, negs, nd, sd);
        run_select(h, nd, sd, n_cand, bd, 1, md, ld, n_seq, 1, w.best, w.loss, w.dis, w.locs);
        OPOSE_HIP_CHECK(hipMemcpyAsync(num, nd, (size_t)n_cand * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(loss, sd, (size_t)n_cand * 8, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(winner, w.best, 16, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(win_loss, w.loss, 8, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_shapelet_find(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int m,
                        const uint8_t* labels, int n_labels, int max_cands, int32_t* best, double* best_loss,
                        float* dis, int32_t* locs, int32_t* cand_num, double* cand_loss, int flags) {
    const int32_t one = m;
    return opose_shapelet_find_lengths(h, seq, off, n_seq, D, &one, 1, labels, n_labels, max_cands, best, best_loss, dis,
                                       locs, cand_num, cand_loss, flags);
}

int opose_shapelet_mindist_lengths(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D,
                                   const int32_t* m_lens, int n_lens, const int32_t* cand_seqs, int n_cand_seqs,
                                   float* min2, int32_t* loc, int flags) {
    if (!h || !seq || !off || !m_lens || !cand_seqs || !min2 || !loc || n_cand_seqs < 1) return OPOSE_E_ARG;
    ShpLens lens;
    if (const int rc = shp_lens_check(h, m_lens, n_lens, &lens)) return rc;
    if (const int rc = shp_check(h, off, n_seq, D, lens.m[n_lens - 1])) return rc;
    for (int i = 0; i < n_cand_seqs; ++i)
        if (cand_seqs[i] < 0 || cand_seqs[i] >= n_seq) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const bool od = flags & OPOSE_OUT_DEVICE;
        const int64_t L = off[n_seq];
        std::vector<ShpBlock> blocks;
        std::vector<ShpChunk> chunks;
        const std::vector<int> cands(cand_seqs, cand_seqs + n_cand_seqs);
        const int64_t nc0 = shp_table(off, lens.m[0], cands, INT32_MAX, blocks, chunks);
        // length l's block of rows follows the blocks of the shorter lengths, compacted
        std::vector<ShpLenRows> rows(blocks.size() * n_lens);
        int64_t total = 0;
        for (int l = 0; l < n_lens; ++l)
            for (size_t b = 0; b < blocks.size(); ++b) {
                const int nv = shp_valid_at(off, blocks[b], lens.m[l]);
                rows[b * n_lens + l] = ShpLenRows{(int32_t)total, nv};
                total += nv;
            }
        if (nc0 > INT32_MAX || total > INT32_MAX)
            throw std::invalid_argument("shapelet: too many candidates for one call");
        const size_t n_out = (size_t)total * n_seq;
        const float* sd = shp_stage(h, h->shp_seq, seq, (size_t)L * D, flags & OPOSE_IN_DEVICE);
        const int64_t* offd = shp_stage(h, h->shp_off, off, (size_t)n_seq + 1, false);
        float* md = od ? min2 : h->shp_min2.ensure<float>(n_out, h->stream);
        int32_t* ld = od ? loc : h->shp_loc.ensure<int32_t>(n_out, h->stream);
        const ShpBlock* bd = shp_upload(h, h->shp_blocks, blocks);
        const ShpLenRows* rd = shp_upload(h, h->shp_lrows, rows);
        run_mindist(h, sd, offd, n_seq, D, lens, bd, rd, (int)blocks.size(), (int)nc0, L, md, ld);
        if (!od) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(min2, md, n_out * 4, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipMemcpyAsync(loc, ld, n_out * 4, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_shapelet_find_lengths(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D,
                                const int32_t* m_lens, int n_lens, const uint8_t* labels, int n_labels, int max_cands,
                                int32_t* best, double* best_loss, float* dis, int32_t* locs, int32_t* cand_num,
                                double* cand_loss, int flags) {
    if (!h || !seq || !off || !m_lens || !labels || !best || !best_loss || !dis || !locs) return OPOSE_E_ARG;
    if (max_cands < 0 || (cand_num == nullptr) != (cand_loss == nullptr)) return OPOSE_E_ARG;
    int negs = 0;
    if (const int rc = shp_labels_check(h, labels, n_labels, n_seq, &negs)) return rc;
    if (negs == n_labels) {
        h->err = "shapelet: no positive sequence, so no candidate";
        return OPOSE_E_ARG;
    }
    ShpLens lens;
    if (const int rc = shp_lens_check(h, m_lens, n_lens, &lens)) return rc;
    if (const int rc = shp_check(h, off, n_seq, D, lens.m[n_lens - 1])) return rc;
    OPOSE_TRY(h, {
        enter_main(h);
        const bool od = flags & OPOSE_OUT_DEVICE;
        const int64_t L = off[n_seq];
        const size_t ns = (size_t)n_seq, nl = (size_t)n_lens;
        std::vector<int> cands;
        for (int i = 0; i < n_labels; ++i)
            if (labels[i]) cands.push_back(i);
        // the chunks are those of the shortest length, which has the most candidates
        std::vector<ShpBlock> blocks;
        std::vector<ShpChunk> chunks;
        const int64_t total0 = shp_table(off, lens.m[0], cands, max_cands ? max_cands : kShpDefaultCands, blocks, chunks);
        int cap = 0;
        for (const ShpChunk& c : chunks) cap = std::max(cap, c.nc);
        if (total0 > INT32_MAX || (int64_t)cap * n_lens > INT32_MAX)
            throw std::invalid_argument("shapelet: too many candidates for one call");
        // Per chunk and length: the rows the distance kernel writes (length l's block of the
        // workspace starts at row l * cap), and the table the selection reads, which leaves out the
        // entries without a valid start at that length and counts its rows from the block's first.
        struct Part {
            size_t t0;  // first entry in sel
            int nt, nc;
        };
        std::vector<ShpLenRows> rows(blocks.size() * nl);
        std::vector<ShpBlock> sel;
        std::vector<Part> parts(chunks.size() * nl);
        std::vector<size_t> first_out(nl + 1, 0);  // length l's first candidate among all lengths' candidates
        for (size_t ci = 0; ci < chunks.size(); ++ci)
            for (int l = 0; l < n_lens; ++l) {
                Part p{sel.size(), 0, 0};
                for (int b = chunks[ci].b0; b < chunks[ci].b0 + chunks[ci].nb; ++b) {
                    const int nv = shp_valid_at(off, blocks[b], lens.m[l]);
                    rows[(size_t)b * nl + l] = ShpLenRows{l * cap + p.nc, nv};
                    if (nv) {
                        sel.push_back(ShpBlock{blocks[b].seq, blocks[b].r0, nv, p.nc});
                        p.nt++;
                        p.nc += nv;
                    }
                }
                parts[ci * nl + l] = p;
                first_out[l + 1] += (size_t)p.nc;
            }
        for (int l = 0; l < n_lens; ++l) first_out[l + 1] += first_out[l];
        const float* sd = shp_stage(h, h->shp_seq, seq, (size_t)L * D, flags & OPOSE_IN_DEVICE);
        const int64_t* offd = shp_stage(h, h->shp_off, off, (size_t)n_seq + 1, false);
        const uint8_t* yd = shp_stage(h, h->shp_labels, labels, (size_t)n_labels, false);
        float* md = h->shp_min2.ensure<float>(nl * cap * ns, h->stream);
        int32_t* ld = h->shp_loc.ensure<int32_t>(nl * cap * ns, h->stream);
        // every candidate's num / loss when asked for (per length, concatenated), else one chunk's
        const bool all = cand_num != nullptr;
        const size_t n_score = all ? first_out[nl] : nl * cap;
        int32_t* nd = all && od ? cand_num : h->shp_num.ensure<int32_t>(n_score, h->stream);
        double* sl = all && od ? cand_loss : h->shp_loss.ensure<double>(n_score, h->stream);
        const ShpWinners w =
            od ? ShpWinners{nl, ns, best, best_loss, dis, locs}
               : ShpWinners::in_block(h->shp_best.ensure<uint8_t>(ShpWinners::bytes(nl, ns), h->stream), nl, ns);
        const ShpBlock* bd = shp_upload(h, h->shp_blocks, blocks);
        const ShpLenRows* rd = shp_upload(h, h->shp_lrows, rows);
        const ShpBlock* seld = shp_upload(h, h->shp_sel, sel);
        std::vector<size_t> done(nl, 0);
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            const ShpChunk& c = chunks[ci];
            run_mindist(h, sd, offd, n_seq, D, lens, bd + c.b0, rd + (size_t)c.b0 * nl, c.nb, c.nc, L, md, ld);
            for (size_t l = 0; l < nl; ++l) {
                const Part& p = parts[ci * nl + l];
                if (!p.nc) continue;  // only tail starts in this chunk: the length keeps its winner
                const float* ml = md + l * cap * ns;
                int32_t* cn = nd + (all ? first_out[l] + done[l] : l * cap);
                double* cl = sl + (all ? first_out[l] + done[l] : l * cap);
                run_score(h, ml, p.nc, n_seq, n_labels, yd, negs, cn, cl);
                run_select(h, cn, cl, p.nc, seld + p.t0, p.nt, ml, ld + l * cap * ns, n_seq, done[l] == 0, w.best + 4 * l,
                           w.loss + l, w.dis + l * ns, w.locs + l * ns);
                done[l] += (size_t)p.nc;
            }
        }
        if (!od) {
            w.to_host(h, best, best_loss, dis, locs);
            if (all) {
                OPOSE_HIP_CHECK(hipMemcpyAsync(cand_num, nd, first_out[nl] * 4, hipMemcpyDeviceToHost, h->stream));
                OPOSE_HIP_CHECK(hipMemcpyAsync(cand_loss, sl, first_out[nl] * 8, hipMemcpyDeviceToHost, h->stream));
            }
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

// ------------------------------------------------------------------------------------ scan
namespace opose {

// A ragged batch whose sequences may have any length >= 0 (the streams of a scan; the patterns,
// which the caller checks for empty ones): n >= 1 is the caller's.  OPOSE_E_ARG unless off starts
// at 0 and never decreases.
static int scan_offsets_check(opose_ctx* h, const int64_t* off, int n) {
    if (off[0] != 0) {
        h->err = "shapelet scan: offsets must start at 0";
        return OPOSE_E_ARG;
    }
    for (int j = 0; j < n; ++j)
        if (off[j + 1] < off[j]) {
            h->err = "shapelet scan: offsets must not decrease";
            return OPOSE_E_ARG;
        }
    return OPOSE_OK;
}

// The pick stage of one chunk: count, offsets, write.  pair0: the chunk's first pair in occ_off.
static void run_scan_pick(opose_ctx* h, const float* dist, const uint64_t* mask, const int32_t* m_slot,
                          const int64_t* off, int n_seq, int64_t L, int n_pairs, bool first, int32_t* counts,
                          int64_t* running, int64_t* occ_off, int32_t* occ_pos, float* occ_dist, int64_t cap) {
    for (int pass = 0; pass < 2; ++pass) {
        ProfEntry pe;
        h->prof_begin(pe, "shapelet_scan_pick", 0, (double)n_pairs * 16.0 + (double)(n_pairs / n_seq) * (double)L / 8.0);
        launch_shapelet_scan_pick(dist, mask, m_slot, off, n_seq, L, n_pairs, counts, occ_off, occ_pos, occ_dist, cap,
                                  pass == 1, h->stream);
        h->prof_end(pe);
        if (pass == 0) launch_shapelet_scan_offsets(counts, n_pairs, first, running, occ_off, h->stream);
    }
}

// the occurrence outputs of a call with host outputs: occ_off in full, then the first
// min(total, cap) entries; OPOSE_E_CAPACITY when the total exceeds cap
static int scan_copy_out(opose_ctx* h, int64_t n_pairs, const int64_t* offd, const int32_t* posd, const float* distd,
                         int64_t* occ_off, int32_t* occ_pos, float* occ_dist, int64_t cap) {
    OPOSE_HIP_CHECK(hipMemcpyAsync(occ_off, offd, (size_t)(n_pairs + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    const int64_t total = occ_off[n_pairs], n = std::min(total, cap);
    if (n > 0) {
        OPOSE_HIP_CHECK(hipMemcpyAsync(occ_pos, posd, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(occ_dist, distd, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    if (total > cap) {
        h->err = "shapelet scan: more occurrences than cap (occ_off holds the counts)";
        return OPOSE_E_CAPACITY;
    }
    return OPOSE_OK;
}

}  // namespace opose

int opose_shapelet_scan(opose_t* h, const float* pat, const int64_t* pat_off, int n_pat, const float* sigma,
                        const float* seq, const int64_t* off, int n_seq, int D, int max_pats, int64_t* occ_off,
                        int32_t* occ_pos, float* occ_dist, int64_t cap, int flags) {
    if (!h || !pat || !pat_off || !sigma || !seq || !off || !occ_off) return OPOSE_E_ARG;
    if (n_pat < 1 || n_seq < 1 || D < 1 || max_pats < 0 || cap < 0) return OPOSE_E_ARG;
    if (cap > 0 && (!occ_pos || !occ_dist)) return OPOSE_E_ARG;
    if (n_pat > kScanMaxPat || n_seq > kShpMaxSeq || D > kShpMaxD || (int64_t)n_pat * n_seq > kScanMaxPairs) {
        h->err = "shapelet scan: patterns, streams, pairs or D beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    if (const int rc = scan_offsets_check(h, pat_off, n_pat)) return rc;
    if (const int rc = scan_offsets_check(h, off, n_seq)) return rc;
    int m_max = 0;
    for (int p = 0; p < n_pat; ++p) {
        if (pat_off[p + 1] == pat_off[p]) {
            h->err = "shapelet scan: a pattern of 0 rows";
            return OPOSE_E_ARG;
        }
        m_max = (int)std::min<int64_t>(std::max<int64_t>(m_max, pat_off[p + 1] - pat_off[p]), kShpMaxM + 1);
    }
    if (m_max > kShpMaxM || off[n_seq] > kShpMaxRows) {
        h->err = "shapelet scan: a pattern or the batch beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    int status = OPOSE_OK;
    OPOSE_TRY(h, {
        enter_main(h);
        const bool id = flags & OPOSE_IN_DEVICE, od = flags & OPOSE_OUT_DEVICE;
        const int64_t L = off[n_seq], nwords = (L + 63) / 64, n_pairs = (int64_t)n_pat * n_seq;
        int chunk = max_pats;
        if (!chunk)  // the default, halved while the distance rows of a chunk exceed 1 GiB
            for (chunk = kScanDefaultPats; chunk > 1 && (int64_t)chunk * L > (int64_t)1 << 28;) chunk /= 2;
        chunk = std::min(chunk, n_pat);
        const bool lds = shapelet_scan_lds_bytes(m_max, D) <= (size_t)kScanLdsBytes;
        // per chunk of consecutive patterns: its table entries, sorted by length (then by pattern),
        // filled up to whole groups with copies of the last that write nothing
        struct Chunk {
            int p0, np, e0, groups, m_max;
            double rows;  // the sum of the window lengths
        };
        std::vector<Chunk> chunks;
        std::vector<ScanPat> table;
        std::vector<int32_t> m_all(n_pat);
        for (int p = 0; p < n_pat; ++p) m_all[p] = (int32_t)(pat_off[p + 1] - pat_off[p]);
        for (int p0 = 0; p0 < n_pat; p0 += chunk) {
            const int np = std::min(chunk, n_pat - p0);
            std::vector<int> order(np);
            for (int i = 0; i < np; ++i) order[i] = p0 + i;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return m_all[a] < m_all[b]; });
            Chunk c{p0, np, (int)table.size(), (np + kScanPG - 1) / kScanPG, m_all[order[np - 1]], 0.0};
            for (int i = 0; i < c.groups * kScanPG; ++i) {
                const int p = order[std::min(i, np - 1)];
                table.push_back(ScanPat{pat_off[p], m_all[p], i < np ? p - p0 : -1, sigma[p], 0});
                if (i < np) c.rows += m_all[p];
            }
            chunks.push_back(c);
        }
        const float* sd = L ? shp_stage(h, h->shp_seq, seq, (size_t)L * D, id) : nullptr;
        const float* pd = shp_stage(h, h->shp_in, pat, (size_t)pat_off[n_pat] * D, id);
        const int64_t* offd = shp_stage(h, h->shp_off, off, (size_t)n_seq + 1, false);
        float* dd = h->scan_dist.ensure<float>((size_t)chunk * std::max<int64_t>(L, 1), h->stream);
        uint64_t* mk = h->scan_mask.ensure<uint64_t>((size_t)chunk * std::max<int64_t>(nwords, 1), h->stream);
        int32_t* counts = h->scan_counts.ensure<int32_t>((size_t)chunk * n_seq, h->stream);
        int64_t* running = h->scan_total.ensure<int64_t>(1, h->stream);
        int64_t* ofd = od ? occ_off : h->scan_off.ensure<int64_t>((size_t)n_pairs + 1, h->stream);
        int32_t* posd = od ? occ_pos : h->scan_pos.ensure<int32_t>((size_t)std::max<int64_t>(cap, 1), h->stream);
        float* odd = od ? occ_dist : h->scan_odist.ensure<float>((size_t)std::max<int64_t>(cap, 1), h->stream);
        const ScanPat* td = shp_upload(h, h->scan_pats, table);
        const int32_t* md = shp_upload(h, h->scan_m, m_all);
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            const Chunk& c = chunks[ci];
            if (L) {
                ProfEntry pe;
                h->prof_begin(pe, "shapelet_scan_dist", 3.0 * c.rows * (double)L * D,
                              4.0 * c.groups * (double)L * D + 4.0 * c.np * (double)L + 8.0 * c.np * (double)nwords);
                launch_shapelet_scan_dist(pd, td + c.e0, c.groups, m_max, lds, sd, offd, n_seq, L, D, dd, mk, h->stream);
                h->prof_end(pe);
            }
            run_scan_pick(h, dd, mk, md + c.p0, offd, n_seq, L, c.np * n_seq, ci == 0, counts, running,
                          ofd + (size_t)c.p0 * n_seq, posd, odd, cap);
        }
        if (!od) status = scan_copy_out(h, n_pairs, ofd, posd, odd, occ_off, occ_pos, occ_dist, cap);
        h->prof_drain();
    });
    return status;
}

int opose_debug_shapelet_pick(opose_t* h, const float* dist, const int64_t* off, int n_seq, int m, float sigma,
                              int64_t* occ_off, int32_t* occ_pos, float* occ_dist, int64_t cap) {
    if (!h || !dist || !off || !occ_off || n_seq < 1 || m < 1 || cap < 0) return OPOSE_E_ARG;
    if (cap > 0 && (!occ_pos || !occ_dist)) return OPOSE_E_ARG;
    if (n_seq > kShpMaxSeq || m > kShpMaxM) return OPOSE_E_SHAPE;
    if (const int rc = scan_offsets_check(h, off, n_seq)) return rc;
    if (off[n_seq] > kShpMaxRows) return OPOSE_E_SHAPE;
    int status = OPOSE_OK;
    OPOSE_TRY(h, {
        enter_main(h);
        const int64_t L = off[n_seq], nwords = (L + 63) / 64;
        DevBuf db, mb, ob, sb, cb, rb, fb, pb, eb;
        float* dd = db.ensure<float>((size_t)std::max<int64_t>(L, 1), h->stream);
        uint64_t* mk = mb.ensure<uint64_t>((size_t)std::max<int64_t>(nwords, 1), h->stream);
        int64_t* offd = ob.ensure<int64_t>((size_t)n_seq + 1, h->stream);
        int32_t* counts = cb.ensure<int32_t>((size_t)n_seq, h->stream);
        int64_t* running = rb.ensure<int64_t>(1, h->stream);
        int64_t* ofd = fb.ensure<int64_t>((size_t)n_seq + 1, h->stream);
        int32_t* posd = pb.ensure<int32_t>((size_t)std::max<int64_t>(cap, 1), h->stream);
        float* odd = eb.ensure<float>((size_t)std::max<int64_t>(cap, 1), h->stream);
        const std::vector<int32_t> one{m};
        const int32_t* md = shp_upload(h, sb, one);
        OPOSE_HIP_CHECK(hipMemcpyAsync(offd, off, ((size_t)n_seq + 1) * 8, hipMemcpyHostToDevice, h->stream));
        if (L) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(dd, dist, (size_t)L * 4, hipMemcpyHostToDevice, h->stream));
            launch_shapelet_scan_mask(dd, offd, n_seq, L, m, sigma, mk, h->stream);
        }
        run_scan_pick(h, dd, mk, md, offd, n_seq, L, n_seq, true, counts, running, ofd, posd, odd, cap);
        status = scan_copy_out(h, n_seq, ofd, posd, odd, occ_off, occ_pos, occ_dist, cap);
        h->prof_drain();
    });
    return status;
}

// ------------------------------------------------------------------------------------ learned model
namespace opose {

// What a training call's kernels need of its geometry: the model table, the shortest and longest
// query, and the forward grid's tiles (those of the most positions any clip and model have).
struct NetGeom {
    std::vector<NetModel> tab;
    int m_min = 0, m_max = 0, tiles = 0;
};

// The checks of opose_shapelet_net_train after its pointers and scalars, in the order include/opose.h
// documents.  Nothing is launched unless this returns OPOSE_OK.
static int net_check(opose_ctx* h, const int64_t* off, int n_seq, int D, int t_pad, const uint8_t* labels,
                     const int64_t* q_off, int n_models, NetGeom* g) {
    if (n_seq < 1 || D < 1 || n_models < 1 || t_pad < 0) {
        h->err = "shapelet net: n_seq, D and n_models must be positive and t_pad not negative";
        return OPOSE_E_ARG;
    }
    if (n_seq > kShpMaxSeq || D > kShpMaxD || n_models > kNetMaxModels) {
        h->err = "shapelet net: n_seq, D or n_models beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    if (const int rc = scan_offsets_check(h, off, n_seq)) return rc;
    if (off[n_seq] > kShpMaxRows) {
        h->err = "shapelet net: too many rows";
        return OPOSE_E_SHAPE;
    }
    if (q_off[0] != 0) {
        h->err = "shapelet net: q_off must start at 0";
        return OPOSE_E_ARG;
    }
    for (int k = 0; k < n_models; ++k)
        if (q_off[k + 1] <= q_off[k]) {
            h->err = "shapelet net: a query of no rows, or q_off decreases";
            return OPOSE_E_ARG;
        }
    g->tab.resize(n_models);
    g->m_min = kShpMaxM + 1;
    g->m_max = 0;
    for (int k = 0; k < n_models; ++k) {
        const int64_t m = q_off[k + 1] - q_off[k];
        if (m > kShpMaxM) {
            h->err = "shapelet net: a query longer than the supported window";
            return OPOSE_E_SHAPE;
        }
        g->tab[k] = NetModel{q_off[k], (int32_t)m, 0};
        g->m_min = std::min(g->m_min, (int)m);
        g->m_max = std::max(g->m_max, (int)m);
    }
    for (int i = 0; i < n_seq; ++i)
        if (labels[i] > 1) {
            h->err = "shapelet net: labels must be 0 or 1";
            return OPOSE_E_ARG;
        }
    int64_t len_min = INT64_MAX, len_max = 0;
    for (int i = 0; i < n_seq; ++i) {
        len_min = std::min(len_min, off[i + 1] - off[i]);
        len_max = std::max(len_max, off[i + 1] - off[i]);
    }
    if (t_pad == 0 && len_min < g->m_max) {
        h->err = "shapelet net: a clip is shorter than a query (and t_pad is 0)";
        return OPOSE_E_SHAPE;
    }
    if (t_pad != 0 && (t_pad < len_max || t_pad < g->m_max)) {
        h->err = "shapelet net: t_pad is shorter than a clip or a query";
        return OPOSE_E_SHAPE;
    }
    const int64_t p_max = (t_pad ? t_pad : len_max) - g->m_min + 1;
    g->tiles = (int)((p_max + kNetTC - 1) / kNetTC);
    return OPOSE_OK;
}

// Adam's two per-step scalars as torch forms them: in float64 from the step count, rounded once
static void net_adam_scalars(double lr, int64_t t, float* step, float* bc2s) {
    *step = (float)(lr / (1.0 - std::pow(0.9, (double)t)));
    *bc2s = (float)std::sqrt(1.0 - std::pow(0.999, (double)t));
}

}  // namespace opose

int opose_shapelet_net_train(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int t_pad,
                             const uint8_t* labels, const int64_t* q_off, int n_models, float* query, float* head,
                             float* q_m, float* q_v, float* head_m, float* head_v, int64_t step0, int epochs, double lr,
                             float* dis, int32_t* locs, double* loss, int32_t* correct, double* loss_hist, int flags) {
    if (!h || !seq || !off || !labels || !q_off || !query || !head || !q_m || !q_v || !head_m || !head_v || !dis ||
        !locs || !loss || !correct)
        return OPOSE_E_ARG;
    if (!(lr > 0.0) || epochs < 0 || step0 < 0) {
        h->err = "shapelet net: lr must be positive, epochs and step0 not negative";
        return OPOSE_E_ARG;
    }
    NetGeom geo;
    if (const int rc = net_check(h, off, n_seq, D, t_pad, labels, q_off, n_models, &geo)) return rc;
    OPOSE_TRY(h, {
        enter_main(h);
        const bool od = flags & OPOSE_OUT_DEVICE;
        const int64_t L = off[n_seq];
        const size_t ns = (size_t)n_seq, nm = (size_t)n_models, nq = (size_t)q_off[n_models] * D, ne = (size_t)epochs;
        // (every clip may be empty in the padded mode: then no row is ever addressed)
        const float* sd = L ? shp_stage(h, h->shp_seq, seq, (size_t)L * D, flags & OPOSE_IN_DEVICE) : nullptr;
        const int64_t* offd = shp_stage(h, h->shp_off, off, ns + 1, false);
        const uint8_t* yd = shp_stage(h, h->shp_labels, labels, ns, false);
        // the state: the caller's device arrays, or one staged block
        //   float query[nq] | q_m[nq] | q_v[nq] | head[4 nm] | head_m[4 nm] | head_v[4 nm]
        float* st[6] = {query, q_m, q_v, head, head_m, head_v};
        float* const host_st[6] = {query, q_m, q_v, head, head_m, head_v};
        const size_t st_n[6] = {nq, nq, nq, 4 * nm, 4 * nm, 4 * nm};
        if (!od) {
            float* p = h->net_state.ensure<float>(3 * nq + 12 * nm, h->stream);
            for (int a = 0; a < 6; ++a) {
                st[a] = p;
                p += st_n[a];
            }
        }
        // the outputs: the caller's, or one staged block
        //   double loss[nm] | loss_hist[nm][epochs] | float dis[nm][ns] | int32 locs[nm][ns] | correct[nm]
        float* dd = dis;
        int32_t* ld = locs;
        double* sl = loss;
        int32_t* cd = correct;
        double* hd = loss_hist;
        if (!od) {
            uint8_t* p = h->net_out.ensure<uint8_t>(8 * nm * (1 + ne) + 8 * nm * ns + 4 * nm, h->stream);
            sl = reinterpret_cast<double*>(p);
            hd = loss_hist ? sl + nm : nullptr;
            dd = reinterpret_cast<float*>(p + 8 * nm * (1 + ne));
            ld = reinterpret_cast<int32_t*>(dd + nm * ns);
            cd = ld + nm * ns;
        }
        uint64_t* best = h->net_best.ensure<uint64_t>(2 * nm * ns, h->stream);
        float* gd = h->net_g.ensure<float>(nm * ns, h->stream);
        double* ws = h->net_ws.ensure<double>(5 * nm * ns, h->stream);
        const NetModel* tab = shp_upload(h, h->net_tab, geo.tab);
        if (!od)
            for (int a = 0; a < 6; ++a)
                OPOSE_HIP_CHECK(hipMemcpyAsync(st[a], host_st[a], st_n[a] * 4, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(best, 0xff, 2 * nm * ns * 8, h->stream));
        ProfEntry pe;
        h->prof_begin(pe, "shapelet_net_train", 0, 0);
        // Three launches per epoch, back to back in stream order: the forward pass into one key
        // buffer, the head (which also resets the other buffer for the next epoch), the query step.
        for (int e = 0; e < epochs; ++e) {
            float step, bc2s;
            net_adam_scalars(lr, step0 + e + 1, &step, &bc2s);
            uint64_t* cur = best + (size_t)(e & 1) * nm * ns;
            uint64_t* nxt = best + (size_t)((e + 1) & 1) * nm * ns;
            launch_shapelet_net_forward(sd, offd, n_seq, D, t_pad, tab, n_models, geo.m_max, geo.tiles, st[0], cur,
                                        h->stream);
            launch_shapelet_net_head(cur, nxt, yd, n_seq, n_models, st[3], st[4], st[5], step, bc2s, true, gd, ws,
                                     hd ? hd + e : nullptr, epochs, nullptr, nullptr, nullptr, nullptr, h->stream);
            launch_shapelet_net_step(sd, offd, n_seq, D, tab, n_models, geo.m_max, cur, gd, st[0], st[1], st[2], step,
                                     bc2s, nullptr, h->stream);
        }
        // the closing forward pass with the final parameters
        uint64_t* cur = best + (size_t)(epochs & 1) * nm * ns;
        launch_shapelet_net_forward(sd, offd, n_seq, D, t_pad, tab, n_models, geo.m_max, geo.tiles, st[0], cur, h->stream);
        launch_shapelet_net_head(cur, nullptr, yd, n_seq, n_models, st[3], st[4], st[5], 0.0f, 1.0f, false, nullptr, ws,
                                 sl, 1, dd, ld, cd, nullptr, h->stream);
        h->prof_end(pe);
        if (!od) {
            for (int a = 0; a < 6; ++a)
                OPOSE_HIP_CHECK(hipMemcpyAsync(host_st[a], st[a], st_n[a] * 4, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipMemcpyAsync(loss, sl, 8 * nm, hipMemcpyDeviceToHost, h->stream));
            if (loss_hist && ne)
                OPOSE_HIP_CHECK(hipMemcpyAsync(loss_hist, hd, 8 * nm * ne, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipMemcpyAsync(dis, dd, 4 * nm * ns, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipMemcpyAsync(locs, ld, 4 * nm * ns, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipMemcpyAsync(correct, cd, 4 * nm, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_debug_shapelet_net_grad(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int t_pad,
                                  const uint8_t* labels, const float* query, int m, const float* head, float* g,
                                  float* dq, double* dhead, double* loss) {
    if (!h || !seq || !off || !labels || !query || !head || !g || !dq || !dhead || !loss) return OPOSE_E_ARG;
    const int64_t q_off[2] = {0, m};
    NetGeom geo;
    if (const int rc = net_check(h, off, n_seq, D, t_pad, labels, q_off, 1, &geo)) return rc;
    OPOSE_TRY(h, {
        enter_main(h);
        const int64_t L = off[n_seq];
        const size_t ns = (size_t)n_seq, nq = (size_t)m * D;
        DevBuf sb, ob, yb, tb, qb, hb, bb, gb, wb, db, rb;
        float* sd = sb.ensure<float>((size_t)std::max<int64_t>(L, 1) * D, h->stream);
        int64_t* offd = ob.ensure<int64_t>(ns + 1, h->stream);
        uint8_t* yd = yb.ensure<uint8_t>(ns, h->stream);
        float* qd = qb.ensure<float>(nq, h->stream);
        float* hd = hb.ensure<float>(4, h->stream);
        uint64_t* best = bb.ensure<uint64_t>(ns, h->stream);
        float* gd = gb.ensure<float>(ns, h->stream);
        double* ws = wb.ensure<double>(5 * ns, h->stream);
        float* dqd = db.ensure<float>(nq, h->stream);
        double* rd = rb.ensure<double>(5, h->stream);  // dhead [4] | loss
        const NetModel* tab = shp_upload(h, tb, geo.tab);
        if (L) OPOSE_HIP_CHECK(hipMemcpyAsync(sd, seq, (size_t)L * D * 4, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(offd, off, (ns + 1) * 8, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(yd, labels, ns, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(qd, query, nq * 4, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(hd, head, 16, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(best, 0xff, ns * 8, h->stream));
        launch_shapelet_net_forward(sd, offd, n_seq, D, t_pad, tab, 1, m, geo.tiles, qd, best, h->stream);
        launch_shapelet_net_head(best, nullptr, yd, n_seq, 1, hd, nullptr, nullptr, 0.0f, 1.0f, false, gd, ws, rd + 4, 1,
                                 nullptr, nullptr, nullptr, rd, h->stream);
        launch_shapelet_net_step(sd, offd, n_seq, D, tab, 1, m, best, gd, qd, nullptr, nullptr, 0.0f, 1.0f, dqd,
                                 h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(g, gd, ns * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(dq, dqd, nq * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(dhead, rd, 32, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(loss, rd + 4, 8, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}
