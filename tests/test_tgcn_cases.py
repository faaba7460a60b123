"""CPU: the TGCN cases have the geometry they claim, clip_inputs and load_state_dict do what
src/tgcn.py says, and the golden files (the reference's float32 CPU logits) agree with the float64
statement of tests/tgcn_cases.py within its network bound."""
import json
import os

import numpy as np
import pytest

import tgcn_cases as tc
from conftest import report


def test_bars_are_the_projects():
    import conv_layer_cases as cl
    assert (tc.REL, tc.ABS, tc.ONE_HOT) == (cl.REL, cl.ABS, cl.ONE_HOT) == (4e-6, 1e-6, 2.0 ** -21)


@pytest.mark.parametrize("name", list(tc.LAYER_CASES))
def test_layer_case_geometry(name):
    c = tc.LAYER_CASES[name]
    sd, x, res, refs = tc.layer_case(name)
    assert c["B"] <= 3
    assert x.shape == (c["B"], c["V"], c["F"]) and res.shape == (c["B"], c["V"], c["H"])
    assert sd["gc1.weight"].shape == (c["F"], c["H"]) and sd["gc1.att"].shape == (c["V"], c["V"])
    for r in (False, True):
        y, bound = refs[r]
        assert y.shape == bound.shape == (c["B"], c["V"], c["H"]) and y.dtype == np.float64
        assert np.isfinite(y).all() and (bound > 0).all()
    a, cc = tc.fold(sd, "gc1", "bn1")
    pre = np.arctanh(np.clip(refs[False][0], -1 + 1e-16, 1 - 1e-16))
    if name.startswith("large_a"):
        assert np.abs(a).min() > 100 and (np.abs(refs[False][0]) < 0.99).mean() > 0.5  # large |a|, not all saturated
    if name.startswith("saturated_plus"):
        assert (refs[False][0] == 1.0).all() or refs[False][0].min() > 1 - 1e-15
    if name.startswith("saturated_minus"):
        assert refs[False][0].max() < -1 + 1e-15
    if name.startswith("tiny"):
        assert not cc.any() and 1e-8 < np.abs(pre).max() < 1e-5


def test_layer_cases_cover_the_limits_and_the_tiles():
    geo = {(c["V"], c["F"], c["H"]) for c in tc.LAYER_CASES.values()}
    assert {(55, 64, 64), (64, 64, 64), (1, 1, 1), (17, 50, 100), (64, 1024, 8), (64, 8, 1024)} <= geo


def test_one_hot_model_is_single_term():
    sd, xval = tc.one_hot_model()
    g = tc.ONE_HOT_GEOM
    assert 0.5 <= abs(xval) < 2
    for k in ("gc1.weight", "gc1.att"):
        assert ((np.abs(sd[k]) >= 0.5) & (np.abs(sd[k]) < 2)).all()
    want, tol = tc.one_hot_expected(sd, xval, 23, 31)
    assert want.shape == (g["V"], g["H"]) and (np.abs(want) > 0).all() and (tol < 1e-5).all()
    assert {(0, 0), (g["V"] - 1, g["F"] - 1)} <= set(tc.ONE_HOT_AT)
    # a lost (1,1), (2,0) or (0,2) piece product costs up to 2^-18 of a product: 3x the bar
    assert 2.0 ** -18 > 3 * (2 * tc.ONE_HOT + 2.0 ** -23)


# ------------------------------------------------------------------------------------ clip_inputs
@pytest.mark.parametrize("num_samples,copies", [(5, 1), (4, 3), (1, 4)])
def test_clip_inputs_equals_the_loop(num_samples, copies):
    from src.tgcn import clip_inputs
    rng = np.random.default_rng(5)
    data = rng.standard_normal((60, 7, 3))
    S = copies * num_samples
    # len below, equal to and above copies * num_samples; a one-frame clip; the last frame
    ranges = [(3, 3 + max(S - 2, 1)), (10, 10 + S), (0, 60), (59, 60), (20, 20 + 2 * S + 1)]
    ranges = [(b, min(e, 60)) for b, e in ranges]
    got = clip_inputs(data, np.array(ranges), num_samples, copies)
    want = tc.clip_inputs_loop(data, ranges, num_samples, copies)
    assert got.dtype == np.float32 and got.shape == (len(ranges), 7, copies * 2 * num_samples)
    assert np.array_equal(got, want)
    import torch
    got_t = clip_inputs(torch.from_numpy(data), np.array(ranges), num_samples, copies)
    assert got_t.dtype == torch.float32 and np.array_equal(got_t.numpy(), want)


def test_clip_inputs_each_copy_spans_the_clip():
    from src.tgcn import clip_inputs
    data = np.zeros((40, 1, 2))
    data[:, 0, 0] = np.arange(40)
    out = clip_inputs(data, [(0, 40)], 5, 4)[0, 0].reshape(4, 5, 2)[:, :, 0]
    assert np.array_equal(out[:, 0], [0, 2, 4, 6]) and np.array_equal(out[:, -1], [32, 34, 36, 38])


@pytest.mark.parametrize("ranges", [[(5, 5)], [(7, 3)], [(0, 61)], [(-1, 4)]])
def test_clip_inputs_refuses_bad_ranges(ranges):
    from src.tgcn import clip_inputs
    with pytest.raises(ValueError):
        clip_inputs(np.zeros((60, 7, 3)), ranges, 4, 2)


# ------------------------------------------------------------------------------------ load_state_dict
def _model(g):
    from src.tgcn import GCN_muti_att
    return GCN_muti_att(g["F"], g["H"], g["C"], p_dropout=0.3, num_stage=g["S"], is_resi=g["is_resi"])


def test_load_state_dict_takes_the_references_keys():
    name = "g0_f16_h32_c10_s2"
    sd, _, _, _ = tc.golden_case(name)
    m = _model(tc.GOLDEN_CASES[name])
    assert set(m.expected_shapes()) == set(sd)
    extra = dict(sd)
    extra["bn1.num_batches_tracked"] = np.int64(3)
    m.load_state_dict(extra)
    g = tc.GOLDEN_CASES[name]
    V, H = 55, g["H"]
    per = lambda F: F * H + V * V + H + 4 * V * H  # noqa: E731
    assert m._params.dtype == np.float32 and m._params.size == per(g["F"]) + 2 * g["S"] * per(H) + g["C"] * H + g["C"]
    assert np.array_equal(m._params[:g["F"] * H], sd["gc1.weight"].ravel())
    assert np.array_equal(m._params[-g["C"]:], sd["fc_out.bias"])


def test_load_state_dict_refusals():
    name = "g1_f24_h48_c7_s1_plain"
    sd, _, _, _ = tc.golden_case(name)
    m = _model(tc.GOLDEN_CASES[name])
    for key in ("gc1.att", "gcbs.0.bn2.running_var", "fc_out.bias"):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match="no " + key):
            m.load_state_dict(bad)
    bad = dict(sd)
    bad["gc1.weight"] = sd["gc1.weight"].T
    with pytest.raises(ValueError, match="shape"):
        m.load_state_dict(bad)
    bad = dict(sd)
    bad["bn1.running_mean"] = sd["bn1.running_mean"].reshape(55, -1)
    with pytest.raises(ValueError, match="shape"):
        m.load_state_dict(bad)
    with pytest.raises(ValueError):
        _model(tc.GOLDEN_CASES[name]).forward(np.zeros((1, 55, 24), np.float32))  # no weights yet


def test_top_n_accuracy_is_the_references():
    from src.tgcn import top_n_accuracy
    logits = np.array([[0.1, 0.9, 0.5], [0.8, 0.1, 0.3], [0.2, 0.3, 0.9]])
    assert top_n_accuracy(np.array([1, 2, 0]), logits, 1) == 1 / 3
    assert top_n_accuracy(np.array([1, 2, 0]), logits, 2) == 2 / 3
    assert top_n_accuracy(np.array([1, 2, 0]), logits, 3) == 1.0


# ------------------------------------------------------------------------------------ golden files
def test_golden_files_are_small():
    size = sum(os.path.getsize(os.path.join(tc.GOLDEN, "tgcn_ref" + e)) for e in (".npz", ".json"))
    assert size < 1_000_000
    meta = json.load(open(os.path.join(tc.GOLDEN, "tgcn_ref.json")))
    assert set(meta["cases"]) == set(tc.GOLDEN_CASES) and len(meta["rejected"]) <= 1


@pytest.mark.parametrize("name", list(tc.GOLDEN_CASES))
def test_golden_reference_within_the_network_bound(name):
    g = tc.GOLDEN_CASES[name]
    sd, X, ref, meta = tc.golden_case(name)
    assert X.shape == (tc.GOLDEN_B, tc.GOLDEN_V, tc.GOLDEN_COPIES * g["F"]) and ref.shape == (tc.GOLDEN_B, g["C"])
    assert tc.num_stages(sd) == g["S"] and sd["gc1.att"].shape == (55, 55)
    # running statistics moved off the defaults
    assert np.abs(sd["bn1.running_mean"]).max() > 1e-3 and np.abs(sd["bn1.running_var"] - 1).max() > 1e-3
    want, bound, _ = tc.golden_ref(name)
    diff = np.abs(ref.astype(np.float64) - want)
    report("tgcn golden %s: reference float32 vs float64 statement, largest difference %.3g (recorded %.3g), "
           "bound there %.3g" % (name, diff.max(), meta["max_diff"], bound.flat[diff.argmax()]))
    assert (diff <= bound).all()
    top2 = np.sort(want, axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 2 * bound.max(1)).all()
    assert [int(v) for v in ref.argmax(1)] == meta["top1"]
