"""CPU: the several-lengths statement of tests/shapelet_lengths_cases.py equals the single-length
statement of tests/shapelet_cases.py per length, bit for bit, and each seeded case has the geometry
its comment claims (empty tail entry, all-tail chunk, ties, differing winners)."""
import numpy as np
import pytest

import shapelet_cases as sc
import shapelet_lengths_cases as lc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_find(got, want):
    for k in ("shapeindex", "cand", "num", "loss", "n_cand"):
        assert got[k] == want[k], k
    for k in ("dis", "min2"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    for k in ("locs", "loc", "nums"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["losses"].view(np.uint64), want["losses"].view(np.uint64))


# the cases whose single-length statement is cheap enough to take for every length
@pytest.mark.parametrize("name", [n for n in lc.MINDIST_CASES if not n.startswith("full_")])
def test_every_snapshot_equals_the_single_length_statement(name):
    seqs, m_lens, cands = lc.mindist_case(name)
    got = lc.mindist_expected(name)
    assert len(got) == len(m_lens)
    for m, (min2, loc) in zip(m_lens, got):
        want2, wantloc = sc.mindist(seqs, cands, m)
        assert min2.shape == want2.shape == (sum(len(seqs[i]) - m + 1 for i in cands), len(seqs))
        assert np.array_equal(bits(min2), bits(want2)) and np.array_equal(loc, wantloc), m


@pytest.mark.parametrize("which", list(lc.FULL_LENGTHS))
def test_full_register_set_cases(which):
    """kShpMaxLens lengths; the shortest, one inside and the longest against the single-length statement."""
    seqs, m_lens, cands = lc.mindist_case("full_" + which)
    assert len(m_lens) == lc.MAXLENS and m_lens[-1] == (lc.MAXM if which == "high" else lc.MAXLENS)
    assert [len(y) for y in seqs] == [lc.MAXM, lc.MAXM + lc.TR + 1]
    got = lc.mindist_expected("full_" + which)
    for l in (0, 7, lc.MAXLENS - 1):
        want2, wantloc = sc.mindist(seqs, cands, m_lens[l])
        assert np.array_equal(bits(got[l][0]), bits(want2)) and np.array_equal(got[l][1], wantloc), l


def test_edge_cases_have_the_claimed_block_geometry():
    for key, lens in lc.EDGE_LENGTHS.items():
        seqs, m_lens, cands = lc.mindist_case("edges_" + key)
        mx = lens[-1]
        assert m_lens == lens and seqs[0].shape == (mx, lc.DC + 3) and cands == list(range(len(seqs)))
        P = [len(y) - mx + 1 for y in seqs]  # at the longest length
        assert P == [1, 2, lc.TR, lc.TR + 1, lc.TR + 2, 2 * lc.TC + 4]
        # at the shortest length the same clips have other block counts: the edges move with the length
        blocks = lambda m: [-(-(len(y) - m + 1) // lc.TR) for y in seqs]  # noqa: E731
        assert blocks(lens[0]) != blocks(mx)
    assert lc.EDGE_LENGTHS["long"][-2:] == [lc.TC + 1, lc.TC + 8]


def test_reference_case_is_the_reference_loop():
    seqs, m_lens, _ = lc.mindist_case("reference")
    assert m_lens == list(range(15, 40, 2)) and len(m_lens) == 13
    assert [y.shape for y in seqs] == [(39, 92), (52, 92), (67, 92), (80, 92)]


def test_ties_go_to_the_first_position_at_every_length():
    seqs, m_lens, cands = lc.mindist_case("ties")
    p1, p2, p3 = lc.TIE_PLACES
    assert p1 % lc.SUB == p2 % lc.SUB == p3 % lc.SUB  # one thread of the start meets all three
    assert p1 // lc.TC == p2 // lc.TC != p3 // lc.TC   # twice in one position block, once in the next
    assert p2 - p1 >= m_lens[-1] and p3 - p2 >= m_lens[-1]
    for m, (min2, loc) in zip(m_lens, lc.mindist_expected("ties")):
        for p in lc.TIE_PLACES:
            assert np.array_equal(seqs[1][p:p + m], seqs[0][1:1 + m])
        assert min2[1, 1] == 0 and loc[1, 1] == p1


@pytest.mark.parametrize("name", ["tail_position", "clip_boundary"])
def test_position_validity_cases(name):
    seqs, (m0, m1), cands = lc.mindist_case(name)
    (short2, shortloc), (long2, longloc) = lc.mindist_expected(name)
    P0, P1 = len(seqs[1]) - m0 + 1, len(seqs[1]) - m1 + 1
    assert shortloc[0, 1] == P0 - 1 and P0 - 1 > P1 - 1  # past the long length's last position
    assert 0 <= longloc[0, 1] <= P1 - 1
    if name == "clip_boundary":  # the window that runs on into clip 2 would win
        cat = np.concatenate(seqs)
        g = len(seqs[0]) + P0 - 1
        crossing = sc.s_matrix(seqs[0][:m1], cat[g:g + m1], m1)[0, 0]
        assert crossing < long2[0, 1]


@pytest.mark.parametrize("seed", lc.FIND_SEEDS)
@pytest.mark.parametrize("mirror", [None, "x-mirror"])
def test_find_lengths_equals_find_per_length(seed, mirror):
    seqs, labels = lc.find_set(seed, mirror)
    got = lc.find_expected(seed, mirror)
    for m, g in zip(lc.FIND_LENGTHS, got):
        same_find(g, sc.find(seqs, labels, m))
    if seed == 0 and mirror is None:
        winners = [(g["shapeindex"], g["cand"]) for g in got]
        assert winners == lc.FIND_WINNERS_SEED0 and len(set(winners)) == len(winners)
    # max_cands = 40 cuts the candidates of the shortest length into several chunks
    n0 = got[0]["n_cand"]
    assert n0 > 2 * lc.FIND_CANDS[1]


@pytest.mark.parametrize("name", list(lc.CHUNK_CASES))
def test_chunk_trap_cases(name):
    seqs, labels, m_lens = lc.chunk_case(name)
    got = lc.chunk_expected(name)
    for m, g in zip(m_lens, got):
        same_find(g, sc.find(seqs, labels, m))
    lengths = [len(y) for y in seqs]
    chunks = lc.length_chunks(lengths, labels, m_lens, lc.CHUNK_CANDS)
    long_counts = [sum(n for _, _, n in c[-1]) for c in chunks]
    where = {}  # (clip, start) -> chunk
    for ci, c in enumerate(chunks):
        for i, r, n in c[0]:
            for k in range(n):
                where[(i, r + k)] = ci
    win_chunk = where[(got[-1]["shapeindex"], got[-1]["cand"])]
    if name.startswith("empty_chunk"):
        assert lengths[0] - m_lens[0] + 1 == 24
        assert long_counts[0] > 0 and long_counts[2] == 0  # the third chunk: only tail starts
        if name == "empty_chunk":
            assert got[-1]["shapeindex"] > 0 and win_chunk > 2
        else:  # the winner comes before the empty chunk and candidates are scored after it
            assert got[-1]["shapeindex"] == 0 and win_chunk == 0 and any(long_counts[3:])
    else:
        assert lengths[0] - m_lens[0] + 1 == lc.TR + 2
        # in one chunk (max_cands = 0) clip 0's second entry is its tail, empty at the long length
        one = lc.length_chunks(lengths, labels, m_lens, sc.DEFAULT_CANDS)
        assert len(one) == 1 and one[0][0][1] == (0, lc.TR, 2) and one[0][-1][1] == (0, lc.TR, 0)
        # in chunks of 8 that tail shares a chunk with the next clip's first starts, the winner among them
        tail = [ci for ci, c in enumerate(chunks) if (0, lc.TR, 2) in c[0]][0]
        assert chunks[tail][-1][0] == (0, lc.TR, 0) and chunks[tail][-1][1][:2] == (2, 0)
        assert got[-1]["shapeindex"] == 2 and win_chunk == tail
