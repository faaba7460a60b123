"""CPU: the NumPy statement of the learned shapelet model (tests/shapelet_net_cases.py) against the
reference's goldens and against torch.autograd, and the geometry its forward cases claim."""
import json
import os

import numpy as np
import pytest
import torch

import shapelet_net_cases as nc
from conftest import GOLDEN

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "shapelet_net_ref.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN, "shapelet_net_ref.npz")), meta


def test_golden_file_is_what_the_generator_promises(golden):
    arrays, meta = golden
    assert [c["seed"] for c in meta["cases"]] == nc.GOLDEN_SEEDS
    assert all(c["seed"] == c["seed_used"] for c in meta["cases"])
    assert meta["seeds_rejected"] == nc.GOLDEN_REJECTED and len(nc.GOLDEN_REJECTED) <= 1
    assert tuple(meta["epochs"]) == nc.EPOCHS
    worst = max(v for c in meta["cases"] for v in c["max_param_diff"].values())
    assert meta["max_param_diff"] == worst and meta["param_atol"] == 4 * worst
    assert 0 < meta["param_atol"] < 1e-3  # far below the learning rate: a wrong step would show
    for seed in nc.GOLDEN_SEEDS:
        assert float(arrays["s%d_score" % seed]) == 1.0


@pytest.mark.parametrize("seed", nc.GOLDEN_SEEDS)
def test_statement_reproduces_the_reference(golden, seed):
    arrays, meta = golden
    atol = meta["param_atol"]
    clips, labels, q0 = nc.golden_case(seed)
    head0 = arrays["s%d_head0" % seed]
    state, hist, kept = nc.train(nc.new_state(q0, head0), clips, labels, nc.EPOCHS[-1], nc.LR, nc.GOLDEN_T,
                                 record=nc.EPOCHS)
    assert state["query"].dtype == F32 and state["head"].dtype == F32
    for e in nc.EPOCHS:
        q, hd, loc = kept[e]
        for got, name in ((q, "q"), (hd, "h")):
            for ref in (arrays["s%d_%s%d" % (seed, name, e)], arrays["s%d_%s%d_f64" % (seed, name, e)]):
                diff = float(np.max(np.abs(got.astype(F64) - ref)))
                print("seed %d epoch %d %s: %.3g (atol %.3g)" % (seed, e, name, diff, atol))
                assert diff <= atol
        assert np.array_equal(loc, arrays["s%d_loc%d" % (seed, e)])
    dis, loc, loss, correct = nc.outputs(state, clips, labels, nc.GOLDEN_T)
    assert np.array_equal(loc, arrays["s%d_loc" % seed]) and correct == len(labels)
    assert hist[-1] < hist[0]


@pytest.mark.parametrize("seed", nc.GOLDEN_SEEDS)
def test_float64_statement_gradients_equal_autograd(golden, seed):
    clips, labels, q0 = nc.golden_case(seed)
    hd = golden[0]["s%d_head0" % seed].astype(F64)
    got = nc.grads(q0, hd, clips, labels, nc.GOLDEN_T, F64)
    want = nc.autograd(q0, hd, clips, labels, nc.GOLDEN_T)
    assert np.array_equal(got["loc"], want["loc"])
    # 1e-12 relative to the largest element: the expansion form the autograd differentiates loses
    # a few of float64's digits where the direct form does not
    for a, b in ((got[k], want[k]) for k in ("dq", "dhead", "loss", "d", "g")):
        scale = float(np.max(np.abs(b)))
        print("seed %d: %.3g of %.3g" % (seed, float(np.max(np.abs(np.asarray(a) - b))), scale))
        assert np.max(np.abs(np.asarray(a) - b)) <= 1e-12 * scale


def test_float32_rule_is_the_shapelet_distance_rule():
    import shapelet_cases as sc
    clips, _, q0 = nc.golden_case(0)
    for x in clips:
        assert np.array_equal(nc.s_row(q0, x).view(np.uint32), sc.s_matrix(q0, x, len(q0))[0].view(np.uint32))


# ---------------------------------------------------------------------------------- case geometry
def test_constants_fit_a_launch():
    assert nc.Q_LDS + nc.X_LDS <= 65536 and nc.TC == 64 and nc.MAXMODELS >= 13


def test_forward_cases_have_the_geometry_they_claim():
    paths = {name: nc.lds_path(nc.forward_case(name)[1]) for name in nc.FORWARD_CASES}
    assert paths["q_lds_under"][0] and not paths["q_lds_over"][0]
    assert paths["q_global_x_lds"] == (False, True) and paths["D1024"] == (True, False)
    assert paths["q_lds_over"] == (False, False) and paths["tiles"] == (True, True)
    assert set(paths.values()) == {(True, True), (True, False), (False, True), (False, False)}
    positions = {name: [len(x) - nc.FORWARD_SHAPES[name][0] + 1 for x in nc.forward_case(name)[0]]
                 for name in ("one_tile", "tile+1", "tiles", "m128")}
    assert positions["one_tile"] == [nc.TC] and positions["tile+1"] == [nc.TC + 1]
    assert max(positions["tiles"]) > 3 * nc.TC and min(positions["m128"]) == 1
    assert nc.FORWARD_SHAPES["D_chunk+1"][1] == nc.DU + 1
    clips, _, t_pad = nc.forward_case("pad_short")
    assert min(len(x) for x in clips) == 0 and any(0 < len(x) < nc.FORWARD_SHAPES["pad_short"][0] for x in clips)


def test_planted_minima_are_where_the_cases_say():
    (d, loc), = nc.forward_expected("first_of_two")
    assert loc.tolist() == [nc.TC - 2, 9] and not d.any()
    clips, queries, t_pad = nc.forward_case("min_in_padding")
    (d, loc), = nc.forward_expected("min_in_padding")
    assert loc.tolist() == [len(x) - 2 for x in clips] and not d.any()
    assert all(l + len(queries[0]) > len(x) for l, x in zip(loc, clips))  # the window reaches the padding
    clips, labels, q, head, t_pad = nc.grad_case("all_in_padding")
    r = nc.grads(q, head, clips, labels, t_pad)
    assert not r["loc"].any() and np.all(r["d"] == np.sum(q.astype(F64) ** 2))


def test_gradient_cases_have_exact_distances():
    for name in nc.GRAD_CASES:
        clips, labels, q, head, t_pad = nc.grad_case(name)
        a, b = nc.forward(q, clips, t_pad), nc.forward(q, clips, t_pad, F64)
        assert np.array_equal(a[0].astype(F64), b[0]) and np.array_equal(a[1], b[1])
