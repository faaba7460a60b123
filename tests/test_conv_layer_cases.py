"""CPU: the inputs and bars of the conv layer tests (tests/conv_layer_cases.py) are what the GPU
test (tests/test_gpu_conv_layers.py) relies on -- every k of a one-hot layer is hit, its values
have third bf16 pieces to lose, the float32 CPU oracle meets every dense bar with room to spare,
the correctly rounded product meets the one-hot bar, and the seeded inputs are the pinned ones."""
import numpy as np
import pytest

import conv_layer_cases as cc


@pytest.mark.parametrize("name", cc.ALL_CASES)
def test_input_digests(name):
    assert cc.case_digest(name) == cc.INPUT_DIGESTS[name]
    assert sorted(cc.INPUT_DIGESTS) == sorted(cc.ALL_CASES)


def test_split3_is_exact():
    v = cc._full_mantissa(np.random.default_rng(1), 4096)
    h0, h1, h2 = cc.split3(v)
    assert np.array_equal((h0.astype(np.float64) + h1) + h2, v.astype(np.float64))
    for h in (h0, h1, h2):
        assert not (h.view(np.uint32) & 0xffff).any()  # bf16 values


@pytest.mark.parametrize("name", list(cc.ONE_HOT_CASES))
def test_one_hot_covers_every_k_with_third_pieces(name):
    c = cc.ONE_HOT_CASES[name]
    x, sets = cc.one_hot_case(name)
    assert cc.one_hot_covered(name).min() >= 1
    assert len(sets) <= 10
    assert cc.third_piece_share(x) >= 0.9
    assert (np.abs(x) >= 0.5).all() and (np.abs(x) < 2).all() and (x < 0).any() and (x > 0).any()
    every = []
    for terms in sets:
        w = cc.one_hot_weights(terms, c["cin"], c["ks"])
        nz = w[w != 0]
        assert len(nz) == sum(len(t) for t in terms)
        assert (np.abs(nz) >= 0.5).all() and (np.abs(nz) < 2).all() and (nz < 0).any() and (nz > 0).any()
        every.append(nz)
    assert cc.third_piece_share(np.concatenate(every)) >= 0.9


@pytest.mark.parametrize("name", list(cc.ONE_HOT_CASES))
def test_rounded_product_meets_the_one_hot_bar(name):
    """The float64 sum of products rounded to fp32 -- what a kernel without any error of its own
    would return -- lies within every one-hot bar, conv1_1's 2^-23 included; a product that lost
    its (1,1) piece term does not."""
    c = cc.ONE_HOT_CASES[name]
    x, sets = cc.one_hot_case(name)
    exp, mag, nterms = cc.one_hot_expected(x, sets[0], c["ks"])
    assert nterms == 1
    y = exp.astype(np.float32).astype(np.float64)
    assert (np.abs(y - exp) <= cc.one_hot_bound(mag, 1, cc.ONE_HOT_FMA)).all()
    assert (exp == 0).any() == (c["ks"] > 1)  # taps outside the frame: exact zeros
    # the same products without their x1 * w1 piece term (each piece 1 is at most 2^-9 of its
    # value: up to 2^-18 |a b|, 8 x the bar): a fifth of the set's outputs leave the bar, the
    # worst by 4x
    x1 = cc.split3(x)[1].astype(np.float64)
    over = []
    for ts in sets[0]:
        ch, _, v = ts[0]
        lost = np.abs(x1[:, ch] * cc.split3(np.float32(v))[1].astype(np.float64).item())
        over.append(lost / (cc.ONE_HOT * np.abs(x[:, ch].astype(np.float64) * np.float64(v))))
    over = np.concatenate([o.ravel() for o in over])
    assert (over > 1).mean() >= 0.2 and over.max() >= 4, ((over > 1).mean(), over.max())


@pytest.mark.parametrize("name", list(cc.DENSE))
def test_float32_oracle_meets_the_dense_bars(name):
    _, _, _, refs = cc.dense_case(name)
    for (i, pool), (ref, bound, o32) in refs.items():
        ratio = np.abs(o32 - ref) / bound
        assert ratio.max() <= 0.25, (name, i, pool, float(ratio.max()))


@pytest.mark.parametrize("name", list(cc.CHAIN))
def test_float32_oracle_meets_the_chain_bars(name):
    _, _, refs = cc.chain_case(name)
    for ref, bound, o32 in refs:
        assert (np.abs(o32 - ref) / bound).max() <= 0.25
        assert (np.abs(np.maximum(o32, 0) - np.maximum(ref, 0)) / bound).max() <= 0.25  # relu2


@pytest.mark.parametrize("stage", [1, 2])
def test_float32_oracle_meets_the_conv1_bars(stage):
    xs, w, b, refs = cc.conv1_case(stage)
    for x, (ref, bound, o32) in zip(xs, refs):
        assert ref.shape == (x.shape[0], 64) + tuple(s // (1 if stage == 1 else 2) for s in x.shape[2:])
        assert (np.abs(o32 - ref) / bound).max() <= 0.25
