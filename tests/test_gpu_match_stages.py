"""GPU: the four kernels that turn peak lists into people -- peaks_finalize, paf_score, limb_greedy,
assemble_people (csrc/post.hip) -- one at a time through their debug hooks, each against the oracle
of the same lines of the reference, at the sizes where they take another path: 1024 peaks ranked by
128 threads, a second trip of paf_score's grid-stride loop, limb_greedy's register slots against its
tail and exact ties in every stage of its merge, more than 64 subset rows, a frame with more
connections than assemble_people stages at once, both capacity statuses and the third-row status.

All four are float64 in the reference's operation order: every comparison of the exact mode is
equality.  The fast mode's PAF values are float32 resamples with torch's taps and are held to
fast_stage_cases' bar.  The cases and what they come from are in tests/match_stage_cases.py;
tests/test_match_stage_cases.py asserts that each reaches its path."""
import ctypes
import os

import numpy as np
import pytest

import match_stage_cases as mc
from conftest import GOLDEN, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handles(native):
    """one handle per capacity"""
    made = {}

    def get(cap, maxp):
        if (cap, maxp) not in made:
            made[cap, maxp] = native.Handle(0)
            made[cap, maxp].set_capacity(cap, maxp)
        return made[cap, maxp]
    return get


# ------------------------------------------------------------------------------- the hooks
def finalize(native, h, cnt, lst, score, N, H, W, cap, maxp):
    rec = np.full((N, mc.record_bytes(cap, maxp)), 0x5a, np.uint8)
    pos = np.full((N, 18, cap), -7, np.int32)
    pcnt = np.full((N, 18), -7, np.int32)
    h.check(native.lib.opose_debug_peaks_finalize(h.h, cnt.ctypes.data, lst.ctypes.data, score.ctypes.data, N, H, W,
                                                  rec.ctypes.data, pos.ctypes.data, pcnt.ctypes.data))
    return rec, pos, pcnt


def paf_score(native, h, fast, maps, geoms, pos, pcnt, N, H, W, cap):
    """geoms [(hl, wl, pad_down | nh, pad_right | nw)] -> score bit patterns [N, 19, cap * cap]"""
    ptrs = (ctypes.c_void_p * len(maps))(*[m.ctypes.data for m in maps])
    g = np.array(geoms, np.int32).T.copy()
    score = np.zeros((N, 19, cap * cap), np.float64)
    h.check(native.lib.opose_debug_paf_score(h.h, fast, len(maps), ptrs, g[0].ctypes.data, g[1].ctypes.data,
                                             g[2].ctypes.data, g[3].ctypes.data, pos.ctypes.data, pcnt.ctypes.data,
                                             N, H, W, mc.THRE2, score.ctypes.data))
    return score.view(np.uint64)


def limb_greedy(native, h, score, pcnt, N, cap):
    ci = np.full((N, 19, cap), -7, np.int32)
    cj = np.full((N, 19, cap), -7, np.int32)
    cs = np.zeros((N, 19, cap), np.float64)
    ccnt = np.full((N, 19), -7, np.int32)
    h.check(native.lib.opose_debug_limb_greedy(h.h, score.ctypes.data, pcnt.ctypes.data, N, ci.ctypes.data,
                                               cj.ctypes.data, cs.ctypes.data, ccnt.ctypes.data))
    return ci, cj, cs, ccnt


def assemble(native, h, rec, pcnt, ci, cj, cs, ccnt):
    rec = rec.copy()
    stage = ctypes.c_int(-1)
    h.check(native.lib.opose_debug_assemble(h.h, rec.ctypes.data, pcnt.ctypes.data, ci.ctypes.data, cj.ctypes.data,
                                            cs.ctypes.data, ccnt.ctypes.data, len(rec), ctypes.byref(stage)))
    return rec, stage.value


def same_records(got, want, cap):
    """byte for byte, with the first difference named"""
    for n in range(len(want)):
        assert got[n, :16].view(np.int32).tolist() == want[n, :16].view(np.int32).tolist(), (n, "header")
        off = 16 + 32 * 18 * cap
        a, b = got[n, 16:off].view(np.float64).reshape(-1, 4), want[n, 16:off].view(np.float64).reshape(-1, 4)
        assert np.array_equal(a, b), (n, "candidate row", int(np.argwhere((a != b).any(1))[0, 0]))
        a, b = got[n, off:].view(np.float64).reshape(-1, 20), want[n, off:].view(np.float64).reshape(-1, 20)
        assert np.array_equal(a, b), (n, "subset row", int(np.argwhere((a != b).any(1))[0, 0]))
    assert np.array_equal(got, want)


# --------------------------------------------------------------------------- peaks_finalize
@pytest.mark.parametrize("name", list(mc.FINALIZE))
def test_peaks_finalize(native, handles, name):
    """Header, candidate rows (x, y, score, id), peak_pos in row-major order and part_cnt: any arrival
    order, 0 .. cap peaks per part, three frames with other counts, 1024 peaks, one peak too many."""
    c = mc.finalize_case(name)
    cap, maxp = c["cap"], c["maxp"]
    rec, pos, pcnt = finalize(native, handles(cap, maxp), c["cnt"], c["list"], c["score"], c["N"], c["H"], c["W"],
                              cap, maxp)
    assert np.array_equal(pcnt, c["part_cnt"])
    assert np.array_equal(pos, c["peak_pos"]), np.argwhere(pos != c["peak_pos"])[:4]
    same_records(rec, c["records"], cap)  # (the hook zeroes the records first: nothing but the rows is written)


# -------------------------------------------------------------------------------- paf_score
@pytest.mark.parametrize("name", list(mc.PAF))
def test_paf_score_exact(native, handles, name):
    """where(accept, score, -inf) of every pair, bit for bit, and the fill everywhere else: a true
    resize, the cropped x8 map as the frame, a resize at step 1.0 along one axis, three scales."""
    c = mc.paf_case(name)
    cap = c["cap"]
    got = paf_score(native, handles(*mc.DEFAULT_CAP), 0, c["maps"], c["scales"], c["peak_pos"], c["part_cnt"],
                    c["N"], c["H"], c["W"], cap)
    want = c["expect"]
    for n in range(c["N"]):
        for k in range(19):
            size = int(c["part_cnt"][n, mc.LIMB_A[k]]) * int(c["part_cnt"][n, mc.LIMB_B[k]])
            a, b = got[n, k, :size].view(np.float64), want[n, k, :size].view(np.float64)
            assert np.array_equal(np.isinf(a), np.isinf(b)), (n, k, "accept", np.flatnonzero(np.isinf(a) != np.isinf(b))[:8])
            assert np.array_equal(a, b), (n, k, "score", np.flatnonzero(a != b)[:8])
            assert (got[n, k, size:] == mc.FILL).all(), (n, k, "written beyond nA * nB")
    assert np.array_equal(got, want)


def test_paf_score_fast_taps(native, handles):
    """The fast mode's PAF samples (torch's taps, float32): scores within 4 e_ref of the float64
    oracle where both oracles accept, accept bits equal wherever the float64 oracle decides by more
    than 8 e_ref."""
    c = mc.paf_fast_case()
    cap = c["cap"]
    got = paf_score(native, handles(*mc.DEFAULT_CAP), 1, [c["maps"]], [c["low"] + c["crop"]], c["peak_pos"],
                    c["part_cnt"], c["N"], c["H"], c["W"], cap).view(np.float64)
    idx, s32, s64, a32, a64, decided = mc.paf_fast_reference(c)
    mine = got[idx[:, 0], idx[:, 1], idx[:, 2]]
    written = np.zeros(got.shape, bool)
    written[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    assert (got.view(np.uint64)[~written] == mc.FILL).all() and not np.isnan(mine).any()
    accept = ~np.isinf(mine)
    excluded = 1 - decided.mean()
    assert excluded <= mc.fc.HAND_EXCLUDED_SHARE
    assert np.array_equal(accept[decided], a64[decided]), np.flatnonzero(decided & (accept != a64))[:8]
    both = a32 & a64 & accept
    assert both.sum() >= 0.99 * (a32 & a64).sum()
    worst, mean, bad = mc.fc.float_bar(mine[both], s32[both], s64[both])
    line = ("match stage paf_score fast taps: max err %.2f e_ref (e_ref %.3g), mean err %.2f x the float32 oracle's, "
            "%.2f %% of %d pairs left out of the accept comparison" % (
                worst, mc.fc.e_ref(s32[both], s64[both]), mean, 100 * excluded, len(decided)))
    print(line)
    report(line)
    assert bad is None, bad


# ------------------------------------------------------------------------------ limb_greedy
@pytest.mark.parametrize("name", list(mc.GREEDY))
def test_limb_greedy(native, handles, name):
    """(i, j, s) in order and conn_cnt against the stable-sort greedy: one register slot, just under
    and just over the eight slots, the tail, ties on four levels and an all-equal matrix, an empty
    part, a limb without a pair, pairs that run out; 2 * 256 flags of dynamic LDS."""
    c = mc.greedy_case(name)
    cap = c["cap"]
    ci, cj, cs, ccnt = limb_greedy(native, handles(cap, c["maxp"]), c["score"], c["part_cnt"], c["N"], cap)
    for (n, k), rows in sorted(c["expect"].items()):
        if rows is None:
            assert ccnt[n, k] == -1, (n, k)
            continue
        m = len(rows)
        assert ccnt[n, k] == m, (n, k, int(ccnt[n, k]), m)
        got = list(zip(ci[n, k, :m].tolist(), cj[n, k, :m].tolist(), cs[n, k, :m].tolist()))
        assert got == rows, (n, k, next(r for r in range(m) if got[r] != rows[r]))
        assert (ci[n, k, m:] == -1).all() and (cj[n, k, m:] == -1).all() and np.isnan(cs[n, k, m:]).all()


# -------------------------------------------------------------------------- assemble_people
@pytest.mark.parametrize("name", list(mc.ASSEMBLE))
def test_assemble(native, handles, name):
    """Status, n_people and the subset rows against oracle.assemble on the same lists: every branch,
    more than 64 rows with a merge below row 64, exactly max_people rows and one more, 72 KB of LDS
    with limb-by-limb staging, the third-row status beside a clean frame, an incoming status."""
    c = mc.assemble_case(name)
    got, _ = assemble(native, handles(c["cap"], c["maxp"]), c["records"], c["part_cnt"], c["conn_i"], c["conn_j"],
                      c["conn_s"], c["conn_cnt"])
    same_records(got, c["expect"], c["cap"])


def test_assemble_at_the_staging_boundary(native, handles):
    """As many connections as the kernel stages at once (the number from the launcher, through the
    hook), and one more: staged whole, then limb by limb."""
    h = handles(*mc.STAGE_CAP)
    empty = mc.assemble_inputs(mc.STAGE_CAP[0], mc.STAGE_CAP[1], [([[] for _ in range(18)], [[]] * 19, list(range(19)))])
    got, stage = assemble(native, h, empty["records"], empty["part_cnt"], empty["conn_i"], empty["conn_j"],
                          empty["conn_s"], empty["conn_cnt"])
    same_records(got, empty["expect"], mc.STAGE_CAP[0])
    assert mc.STAGE_CAP[0] <= stage < 19 * mc.STAGE_CAP[0]  # (else every frame is staged whole)
    for total in (stage, stage + 1):
        c = mc.assemble_total_case(total)
        assert c["conn_cnt"].clip(0).sum() == total
        got, again = assemble(native, h, c["records"], c["part_cnt"], c["conn_i"], c["conn_j"], c["conn_s"],
                              c["conn_cnt"])
        assert again == stage and c["expect"][0, :16].view(np.int32)[2] > 10
        same_records(got, c["expect"], mc.STAGE_CAP[0])


# ---------------------------------------------------------------------------- bad arguments
def test_hooks_refuse_what_the_kernels_would_index_with(native, handles):
    h = handles(*mc.DEFAULT_CAP)
    cap, maxp = mc.DEFAULT_CAP
    E = native.OPOSE_E_ARG
    f = mc.finalize_case("overflow")

    def run_finalize(cnt=f["cnt"], lst=f["list"], H=f["H"]):
        out = [np.zeros_like(f[k]) for k in ("records", "peak_pos", "part_cnt")]
        return native.lib.opose_debug_peaks_finalize(h.h, cnt.ctypes.data, lst.ctypes.data, f["score"].ctypes.data,
                                                     f["N"], H, f["W"], *[o.ctypes.data for o in out])
    bad = f["cnt"].copy()
    bad[1, 3] = -1
    assert run_finalize(cnt=bad) == E
    bad = f["list"].copy()
    bad[0, 11, 5] = f["H"] * f["W"]
    assert run_finalize(lst=bad) == E and run_finalize(H=0) == E and run_finalize() == 0

    p = mc.paf_case("b_frame")
    ptrs = (ctypes.c_void_p * 1)(p["maps"][0].ctypes.data)
    out = np.zeros((p["N"], 19, cap * cap))

    def run_paf(geom=p["scales"][0], pos=p["peak_pos"], pcnt=p["part_cnt"], fast=0):
        g = [np.array([v], np.int32) for v in geom]
        return native.lib.opose_debug_paf_score(h.h, fast, 1, ptrs, *[v.ctypes.data for v in g], pos.ctypes.data,
                                                pcnt.ctypes.data, p["N"], p["H"], p["W"], mc.THRE2, out.ctypes.data)
    bad = p["part_cnt"].copy()
    bad[1, 2] = cap + 1
    assert run_paf(pcnt=bad) == E
    bad = p["peak_pos"].copy()
    bad[0, 1, 0] = -1
    assert run_paf(pos=bad) == E
    assert run_paf(geom=(6, 8, 48, 1)) == E and run_paf(geom=(0, 8, 3, 1)) == E
    assert run_paf(geom=(6, 8, 49, 1), fast=1) == E and run_paf(geom=(6, 8, 0, 1), fast=1) == E

    g = mc.greedy_case("cap128")
    bad = g["part_cnt"].copy()
    bad[0, 0] = cap + 1
    outs = [np.zeros((2, 19, cap), t) for t in (np.int32, np.int32, np.float64)] + [np.zeros((2, 19), np.int32)]
    assert native.lib.opose_debug_limb_greedy(h.h, g["score"].ctypes.data, bad.ctypes.data, 2,
                                              *[o.ctypes.data for o in outs]) == E

    a = mc.assemble_case("index_error")
    stage = ctypes.c_int()

    def run_assemble(ci=a["conn_i"], cj=a["conn_j"], ccnt=a["conn_cnt"]):
        rec = a["records"].copy()
        return native.lib.opose_debug_assemble(h.h, rec.ctypes.data, a["part_cnt"].ctypes.data, ci.ctypes.data,
                                               cj.ctypes.data, a["conn_s"].ctypes.data, ccnt.ctypes.data, a["N"],
                                               ctypes.byref(stage))
    bad = a["conn_i"].copy()
    bad[0, 0, 1] = 3  # three peaks per part
    assert run_assemble(ci=bad) == E
    bad = a["conn_j"].copy()
    bad[0, 1, 2] = -1
    assert run_assemble(cj=bad) == E
    bad = a["conn_cnt"].copy()
    bad[1, 4] = cap + 1
    assert run_assemble(ccnt=bad) == E
    bad[1, 4] = -2
    assert run_assemble(ccnt=bad) == E


# ------------------------------------------------------------------------------------ chain
@pytest.mark.parametrize("name", mc.CHAIN)
def test_chain_of_hooks_is_the_product_path(native, handles, name):
    """A planted golden's candidate rows as a shuffled peak list, then the four hooks in sequence on
    the golden's maps: the golden's candidate and subset."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = mc.chain_case(g, np.random.default_rng(11))
    cap, maxp = mc.DEFAULT_CAP
    h = handles(cap, maxp)
    H, W = c["H"], c["W"]
    rec, pos, pcnt = finalize(native, h, c["cnt"], c["list"], c["score"], 1, H, W, cap, maxp)
    _, _, hl, wl = c["maps"].shape
    score = paf_score(native, h, 0, [c["maps"]], [(hl, wl) + c["pads"]], pos, pcnt, 1, H, W, cap)
    ci, cj, cs, ccnt = limb_greedy(native, h, score.view(np.float64), pcnt, 1, cap)
    rec, _ = assemble(native, h, rec, pcnt, ci, cj, cs, ccnt)
    status, cand, subset = native.decode_record(rec[0], cap, maxp)
    assert status == 0
    assert np.array_equal(cand, c["candidate"]) and np.array_equal(subset, c["subset"])
    assert len(subset) >= 2
