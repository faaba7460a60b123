"""CPU: the inputs of tests/test_gpu_match_stages.py alone -- that every case reaches the path it is
there for, from the oracle and the case tables only, and a digest per case so that a changed
generator cannot quietly lose an edge."""
import numpy as np
import pytest

import match_stage_cases as mc
from oracle import body_post


# --------------------------------------------------------------------------- peaks_finalize
def test_finalize_cases_reach_their_sizes():
    c = mc.finalize_case("cap128")
    assert c["N"] == 3 and {0, 1, 64, 127, 128} <= set(c["cnt"][0].tolist())
    assert len({tuple(r) for r in c["cnt"].tolist()}) == 3  # other counts per frame
    for p in range(18):  # frame 0 arrives in reversed raster order, the others in neither order
        k = c["cnt"][0, p]
        assert (np.diff(c["list"][0, p, :k]) < 0).all()
    for n in (1, 2):
        d = [np.diff(c["list"][n, p, :c["cnt"][n, p]]) for p in range(18)]
        assert sum(((x > 0).any() and (x < 0).any()) for x in d) >= 10
    big = mc.finalize_case("cap1024")
    assert big["cap"] == 1024 and (big["H"], big["W"]) == (40, 60)
    assert big["cnt"][0, 2] == 1000 and big["cnt"][0, 7] == 1024
    over = mc.finalize_case("overflow")
    assert over["cnt"][0, 11] == over["cap"] + 1 and (np.delete(over["cnt"][0], 11) <= over["cap"]).all()
    hdr = over["records"][:, :16].view(np.int32)
    assert hdr[:, 0].tolist() == [-5, 0] and hdr[0, 1] == over["part_cnt"][0].sum() == over["cnt"][0].sum() - 1
    for c in (c, big, over):  # the expectation's own shape: positions ascend, ids run on
        for n in range(c["N"]):
            total = int(c["part_cnt"][n].sum())
            cand = c["records"][n, 16:16 + 32 * total].view(np.float64).reshape(-1, 4)
            assert np.array_equal(cand[:, 3], np.arange(total))
            assert np.array_equal(cand[:, 1] * c["W"] + cand[:, 0],
                                  np.concatenate([c["peak_pos"][n, p, :c["part_cnt"][n, p]] for p in range(18)]))
            for p in range(18):
                assert (np.diff(c["peak_pos"][n, p, :c["part_cnt"][n, p]]) > 0).all()


# -------------------------------------------------------------------------------- paf_score
def _paf_details(name):
    c = mc.paf_case(name)
    det = []
    again = mc.score_blocks(c["peak_pos"], c["part_cnt"], c["pafs"], c["H"], c["W"], c["cap"], det)
    assert np.array_equal(again, c["expect"])
    return c, det


@pytest.mark.parametrize("name", list(mc.PAF))
def test_paf_cases_meet_their_conditions(name):
    c, det = _paf_details(name)
    H, W = c["H"], c["W"]
    assert c["N"] == 2 and not np.array_equal(c["peak_pos"][0], c["peak_pos"][1])
    sizes = {(n, k): s.size for n, k, s, *_ in det}
    for n in range(2):  # a second trip of paf_score's loop in at least three limbs, small and empty ones beside
        assert sum(v > mc.PAF_TRIP for (m, _), v in sizes.items() if m == n) >= 3
        assert sum(v <= 25 for (m, _), v in sizes.items() if m == n) >= 3
        assert sum((n, k) not in sizes for k in range(19)) >= 2
        for p in mc.BIG_PARTS:  # the four corners and every border
            v = c["peak_pos"][n, p, :c["part_cnt"][n, p]]
            y, x = v // W, v % W
            assert {0, W - 1, (H - 1) * W, H * W - 1} <= set(v.tolist())
            assert ((y == 0) & (x > 0) & (x < W - 1)).any() and ((y == H - 1) & (x > 0) & (x < W - 1)).any()
            assert ((x == 0) & (y > 0) & (y < H - 1)).any() and ((x == W - 1) & (y > 0) & (y < H - 1)).any()
    accept = np.concatenate([a.ravel() for _, _, _, a, *_ in det])
    assert 0.15 <= accept.mean() <= 0.85, accept.mean()
    same = far_yes = far_no = eight = nine = near_lo = near_hi = 0
    for n, k, score, acc, norm, s, fx, fy in det:
        ca, cb = (mc.all_peaks_of(c["peak_pos"][n], c["part_cnt"][n], W)[p] for p in (mc.LIMB_A[k], mc.LIMB_B[k]))
        px, py = c["pafs"][n][:, :, mc.PAF_X[k]], c["pafs"][n][:, :, mc.PAF_X[k] + 1]
        assert np.array_equal(mc.pair_details(ca, cb, px, py)[4], score)  # the restatement is limb_scores
        above = (s > mc.THRE2).sum(-1)
        assert np.array_equal(acc, (above > 8) & (score > 0))
        on = norm == 1e-10  # both peaks on one pixel: a zero vector, score 0, rejected
        assert (score[on] == 0).all() and not acc[on].any()
        same += on.sum()
        far_yes += (acc & (norm > H / 2)).sum()
        far_no += (~acc & (norm > H / 2)).sum()
        eight += (~acc & (above == 8)).sum()
        nine += (acc & (above == 9)).sum()
        # A sample coordinate is a + t (b - a) / 9 with integers a, b, t: a multiple of 1 / 9, so never
        # a half; the closest it comes to rint's boundary is 4 / 9 and 5 / 9 past an integer
        for f in (fx, fy):
            frac = f - np.floor(f)
            assert not (frac == 0.5).any()
            near_lo += (np.abs(frac - 4 / 9) < 1e-9).sum()
            near_hi += (np.abs(frac - 5 / 9) < 1e-9).sum()
    assert same >= 1 and far_yes >= 1 and far_no >= 1 and eight >= 1 and nine >= 1 and near_lo >= 1 and near_hi >= 1, (
        same, far_yes, far_no, eight, nine, near_lo, near_hi)
    # nothing beyond a limb's nA * nB entries
    for n in range(2):
        for k in range(19):
            size = sizes.get((n, k), 0)
            assert (c["expect"][n, k, size:] == mc.FILL).all() and not (c["expect"][n, k, :size] == mc.FILL).any()


def test_paf_geometries_take_their_branches():
    def sizes(name):
        c = mc.PAF[name]
        return c["hw"], [(8 * hl - pd, 8 * wl - pr) for hl, wl, pd, pr in c["scales"]]
    (H, W), [(hs, ws)] = sizes("a_resize")
    assert hs < H and ws < W
    (H, W), [(hs, ws)] = sizes("b_frame")
    assert (hs, ws) == (H, W)
    (H, W), [(hs, ws)] = sizes("c_rows_equal")
    assert hs == H and ws != W
    (H, W), three = sizes("d_three_scales")
    assert len(three) == 3 and three[0][0] * 1.5 < H and H < three[1][0] * 1.5 and three[2][0] > 1.5 * H


def test_paf_fast_case_decides_enough():
    c = mc.paf_fast_case()
    assert (c["low"], c["crop"], (c["H"], c["W"])) == ((7, 9), (53, 70), (60, 81))
    idx, s32, s64, a32, a64, decided = mc.paf_fast_reference(c)
    assert 1 - decided.mean() <= mc.fc.HAND_EXCLUDED_SHARE, 1 - decided.mean()
    assert np.array_equal(a32[decided], a64[decided])
    assert 0.15 <= a64.mean() <= 0.85 and (a32 & a64).sum() > 1000
    assert not np.array_equal(s32, s64)  # float32 taps: the two oracles differ


# ------------------------------------------------------------------------------ limb_greedy
def test_greedy_walk_is_connect_limbs():
    c = mc.paf_case("a_resize")
    rows = 0
    for n in range(2):
        peaks = mc.all_peaks_of(c["peak_pos"][n], c["part_cnt"][n], c["W"])
        conns, special = body_post.connect_limbs(peaks, c["pafs"][n], c["H"], mc.THRE2)
        for k in range(19):
            nA, nB = len(peaks[mc.LIMB_A[k]]), len(peaks[mc.LIMB_B[k]])
            if k in special:
                assert nA == 0 or nB == 0
                continue
            got = mc.greedy(c["expect"][n, k].view(np.float64), nA, nB)
            assert [(r[3], r[4], r[2]) for r in conns[k].tolist()] == [(float(i), float(j), s) for i, j, s in got]
            rows += len(got)
    assert rows > 150


def test_greedy_cases_reach_their_sizes():
    c = mc.greedy_case("cap128")
    assert c["N"] == 2
    shape = {(n, k): (int(c["part_cnt"][n, mc.LIMB_A[k]]), int(c["part_cnt"][n, mc.LIMB_B[k]]))
             for n in range(2) for k in range(19)}
    for want in [(1, 1), (1, 128), (128, 1), (16, 16), (45, 45), (46, 45), (128, 100), (128, 128)]:
        assert want in [shape[0, k] for k in range(19)], want
    assert 45 * 45 < mc.TAIL < 46 * 45 and 16 * 16 == mc.GR_THREADS
    assert c["expect"][0, 5] is None and shape[0, 5][1] == 0                        # an empty part
    assert c["expect"][0, 16] == [] and min(shape[0, 16]) > 0                       # all -inf
    few = c["expect"][0, 17]
    assert 0 < len(few) < min(shape[0, 17])                                         # the accepted pairs run out
    assert shape[1, 0] == shape[1, 4] == (128, 128)
    assert [(i, j) for i, j, _ in c["expect"][1, 4]] == [(i, i) for i in range(128)]  # all equal: the diagonal
    for (n, k), rows in c["expect"].items():
        if rows is None:
            continue
        nA, nB = shape[n, k]
        assert len(rows) <= min(nA, nB)
        assert len({i for i, _, _ in rows}) == len({j for _, j, _ in rows}) == len(rows)
        assert (np.diff([s for _, _, s in rows]) <= 0).all()
    big = mc.greedy_case("cap256")
    assert big["cap"] == 256 and (big["part_cnt"][0, 1], big["part_cnt"][0, 2]) == (200, 256)
    assert len(big["expect"][0, 0]) > 150


def test_greedy_ties_reach_every_stage_of_the_merge():
    c = mc.greedy_case("cap128")
    rounds = mc.tie_rounds(c["score"][1, 0], 128, 128)
    assert len(set(c["score"][1, 0, :128 * 128].tolist())) == 4
    tied = [r for r in rounds if len(r) >= 2]
    assert len(tied) >= len(rounds) / 2 and len(rounds) == 128
    wave = lambda e: (e % mc.GR_THREADS) // mc.GR_WAVE
    assert any(len(set(wave(r).tolist())) > 1 for r in tied)                          # the four-wave merge
    assert any(len(set((r[r < mc.TAIL] // mc.GR_THREADS).tolist())) > 1 for r in tied)  # two register slots
    assert any((r < mc.TAIL).any() and (r >= mc.TAIL).any() for r in tied)            # register against tail
    # the winner is a tail pair with rivals in other waves and on its own thread
    assert any(r[0] >= mc.TAIL and len(set(wave(r).tolist())) > 1 for r in tied)
    assert any(r[0] >= mc.TAIL and (r[1:] % mc.GR_THREADS == r[0] % mc.GR_THREADS).any() for r in tied)
    # rows and columns the tail must skip: a tail pair that beats the round's winner but is used
    sc = c["score"][1, 0, :128 * 128].reshape(128, 128)
    rows = c["expect"][1, 0]
    used_i, used_j, skipped = set(), set(), 0
    for i, j, s in rows:
        if used_i:
            mask = np.zeros((128, 128), bool)
            mask[sorted(used_i), :] = True
            mask[:, sorted(used_j)] = True
            mask.ravel()[:mc.TAIL] = False
            skipped += bool((sc[mask] >= s).any())
        used_i.add(i)
        used_j.add(j)
    assert skipped >= 64


# -------------------------------------------------------------------------- assemble_people
def _trace(name, n=0):
    tr = {}
    exp = mc.expected_frame(mc.assemble_case(name)["scenes"][n], mc.ASSEMBLE[name]["cap"][1], 0, tr)
    return tr, exp


def test_assemble_scenes_take_every_branch():
    tally = dict.fromkeys(("new", "skipped_k17", "found1_write", "found1_noop", "merge", "conflict"), 0)
    reasons = set()
    for name in mc.TALLY_CASES:
        tr, exp = _trace(name)
        assert exp[0] == 0 and len(exp[2]) >= 1
        for key in tally:
            tally[key] += tr[key]
        reasons |= {r for _, r in tr["pruned"]}
    assert all(tally.values()) and reasons == {"count", "mean"}, (tally, reasons)
    tr, _ = _trace("p60")  # the row shift after a merge crosses the ballot's 64-row boundary
    assert 64 < tr["peak_rows"] <= 96 and any(row < 64 < rows for row, rows in tr["merges"])


def test_assemble_capacity_edges():
    tr, exp = _trace("p100_rows96")
    assert tr["peak_rows"] == 96 and exp[0] == 0
    tr, exp = _trace("p100_rows97")
    assert tr["peak_rows"] == 97 and exp[0] == -5 and exp[2] is None
    a, b = mc.assemble_case("p100_rows96"), mc.assemble_case("p100_rows97")
    assert b["conn_cnt"].sum() == a["conn_cnt"].sum() + 1 and b["conn_cnt"][0, 0] == a["conn_cnt"][0, 0] + 1
    tr, exp = _trace("p200_cap1024")
    c = mc.assemble_case("p200_cap1024")
    assert 128 < tr["peak_rows"] <= 256 and exp[0] == 0 and c["conn_cnt"].clip(0).sum() > 1500
    assert c["part_cnt"].max() > 128
    for total in (768, 769):  # (the GPU test takes the number from the hook)
        c = mc.assemble_total_case(total)
        assert c["conn_cnt"].clip(0).sum() == total and c["part_cnt"].max() <= mc.STAGE_CAP[0]
        tr = {}
        assert mc.expected_frame(c["scenes"][0], mc.STAGE_CAP[1], 0, tr)[0] == 0 and tr["peak_rows"] > 64


def test_assemble_statuses():
    c = mc.assemble_case("index_error")
    with pytest.raises(IndexError):
        body_post.assemble(*c["scenes"][0])
    assert len({j for _, j in mc.INDEX_ERROR[1][1]}) == 1  # the list that raises is no matching
    hdr = c["expect"][:, :16].view(np.int32)
    assert hdr[:, 0].tolist() == [-6, 0] and hdr[0, 2] == 0 and hdr[1, 2] >= 1
    c = mc.assemble_case("status_in")
    hdr = c["expect"][:, :16].view(np.int32)
    assert hdr[:, 0].tolist() == [-5, 0] and c["records"][0, :16].view(np.int32)[0] == -5
    assert np.array_equal(c["expect"][0], c["records"][0])  # untouched, its subset fill included
    assert (c["records"][0, 16 + 32 * 18 * 128:].view(np.float64) == 7.0).all()
    c = mc.assemble_case("mixed3")
    assert c["expect"][:, :16].view(np.int32)[:, 0].tolist() == [0, -6, 0]


# ---------------------------------------------------------------------------------- digests
def _digest(name):
    kind, _, case = name.partition(":")
    if kind == "finalize":
        c = mc.finalize_case(case)
        return mc.digest(c["cnt"], c["list"], c["score"], c["records"], c["peak_pos"], c["part_cnt"])
    if kind == "paf":
        c = mc.paf_case(case)
        return mc.digest(*c["maps"], c["peak_pos"], c["part_cnt"], c["expect"])
    if kind == "paf_fast":
        c = mc.paf_fast_case()
        return mc.digest(c["maps"], c["peak_pos"], c["part_cnt"], *mc.paf_fast_reference(c)[1:])
    if kind == "greedy":
        c = mc.greedy_case(case)
        rows = [np.array(c["expect"][key] or [], np.float64) for key in sorted(c["expect"])]
        return mc.digest(c["score"], c["part_cnt"], *rows)
    c = mc.assemble_total_case(int(case)) if kind == "total" else mc.assemble_case(case)
    return mc.digest(c["part_cnt"], c["conn_i"], c["conn_j"], c["conn_s"], c["conn_cnt"], c["records"], c["expect"])


DIGESTS = {
    'finalize:cap128': '8d9b0bca5b51bc94',
    'finalize:cap1024': '7e295a8807526824',
    'finalize:overflow': 'b4b03dc5764a9b9d',
    'paf:a_resize': 'd3894b7c1da7383c',
    'paf:b_frame': 'a5ac4d57f6610702',
    'paf:c_rows_equal': 'a8fb18bc95751f34',
    'paf:d_three_scales': '09937cb561cb9bb0',
    'paf_fast:': 'cdbd8290e935a2a6',
    'greedy:cap128': '8dc8d688fe4941e9',
    'greedy:cap256': 'e6bff3171e8685c0',
    'assemble:p5': '7beecd0efd2f8d35',
    'assemble:p40': '077dacff00e2b4f5',
    'assemble:p60': 'ff227520624dfb6c',
    'assemble:p100_rows96': '9213685613f2a4e4',
    'assemble:p100_rows97': 'd23d216e25ca836e',
    'assemble:p200_cap1024': '14ad6188907fbd11',
    'assemble:index_error': 'b1db8f2f301b4171',
    'assemble:status_in': 'c5e212728c0ed82a',
    'assemble:mixed3': '09fab77f41e8ea4a',
    'total:768': 'e5e579148ddd13c7',
    'total:769': 'be8842b58ce6de1d',
}


@pytest.mark.parametrize("name", ["finalize:" + n for n in mc.FINALIZE] + ["paf:" + n for n in mc.PAF] +
                         ["paf_fast:"] + ["greedy:" + n for n in mc.GREEDY] +
                         ["assemble:" + n for n in mc.ASSEMBLE] + ["total:768", "total:769"])
def test_digests(name):
    assert _digest(name) == DIGESTS[name]
