"""The TGCN sign classifier's rule in NumPy float64, seeded case builders and the bounds the tests
hold the device to (tests/test_gpu_tgcn.py on the GPU, tests/test_tgcn_cases.py for the cases and
the golden files alone).

A model is a dict of float32 arrays under the reference's own state_dict keys
(cls/TGCN/tgcn_model.py): gc1.weight [F, H], gc1.att [V, V], gc1.bias [H], bn1.weight / bias /
running_mean / running_var [V * H], gcbs.{i}.gc{1,2}.*, gcbs.{i}.bn{1,2}.*, fc_out.weight [C, H],
fc_out.bias [C].

The rule (include/opose.h), evaluation mode:
    a = float32(gamma / sqrt(running_var + eps)), c = float32(beta + (bias - running_mean) * a64)
    layer(x) = tanh((att @ (x @ W)) * a + c)
    y = stem(x); per block y = layer2(layer1(y)) (+ y when is_resi)
    logits = fc_w @ mean over nodes of y + fc_b; with copies, the mean of the copies' logits.

Bounds.  REL, ABS and ONE_HOT are the project's bar for split-bf16 products
(tests/conv_layer_cases.py), not new numbers.  Per layer, elementwise,
    |a| * (REL * |att| @ (|x| @ |W|) + ABS)      the layer's own two products
  + |a| * |att| @ (bound_in @ |W|)               the error carried from its input (the chained form of
                                                 conv_layer_cases.chain_case)
  + 4 * 2^-24                                    tanhf's own error (tanh is 1-Lipschitz: the two lines
                                                 above pass through it unchanged)
  + the incoming bound on the residual path, unchanged.
The head: the node mean and |fc|-weighted sum of the last layer's bound, plus REL * (|fc| @ mean |y| +
|fc_b|) + ABS of its own.  The mean over copies: the mean of the copies' bounds plus copies * 2^-24 *
mean |logits_i| (copies - 1 fp32 additions and one division, each rounding by at most 2^-24 of a
partial sum that is at most sum |logits_i|).
"""
import functools
import hashlib
import json
import os

import numpy as np

from conv_layer_cases import ABS, ONE_HOT, REL  # noqa: F401  (the project's bar)

BN_EPS = 1e-5
TANHF = 4 * 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------ the rule
def layer_keys(num_stage):
    out = [("gc1", "bn1")]
    for i in range(num_stage):
        out += [(f"gcbs.{i}.gc1", f"gcbs.{i}.bn1"), (f"gcbs.{i}.gc2", f"gcbs.{i}.bn2")]
    return out


def num_stages(sd):
    return sum(1 for k in sd if k.startswith("gcbs.") and k.endswith(".gc1.weight"))


def fold(sd, gc, bn, eps=BN_EPS):
    """(a, c) [V, H] float32 of one layer, formed in float64 and rounded once."""
    V = sd[gc + ".att"].shape[0]
    H = sd[gc + ".weight"].shape[1]
    g, b, m, v = (sd[bn + "." + k].astype(np.float64).reshape(V, H)
                  for k in ("weight", "bias", "running_mean", "running_var"))
    a = g / np.sqrt(v + eps)
    c = b + (sd[gc + ".bias"].astype(np.float64)[None, :] - m) * a
    return a.astype(np.float32), c.astype(np.float32)


def layer_ref(sd, gc, bn, x, bound_in=None, residual=None, res_bound=None):
    """x [B, V, F] float64 -> (y [B, V, H] float64, its elementwise bound)."""
    W, att = sd[gc + ".weight"].astype(np.float64), sd[gc + ".att"].astype(np.float64)
    a, c = (t.astype(np.float64) for t in fold(sd, gc, bn))
    pre = (att @ (x @ W)) * a + c
    y = np.tanh(pre)
    bound = np.abs(a) * (REL * (np.abs(att) @ (np.abs(x) @ np.abs(W))) + ABS) + TANHF
    if bound_in is not None:
        bound = bound + np.abs(a) * (np.abs(att) @ (bound_in @ np.abs(W)))
    if residual is not None:
        y = y + residual
        if res_bound is not None:
            bound = bound + res_bound
    return y, bound


def network_ref(sd, x, is_resi=True):
    """x [B, V, F_in] (any float dtype) -> (logits [B, C] float64, bound [B, C])."""
    x = np.asarray(x, np.float64)
    keys = layer_keys(num_stages(sd))
    y, b = layer_ref(sd, *keys[0], x)
    for s in range(num_stages(sd)):
        y1, b1 = layer_ref(sd, *keys[1 + 2 * s], y, b)
        y, b = layer_ref(sd, *keys[2 + 2 * s], y1, b1, y if is_resi else None, b if is_resi else None)
    fw, fb = sd["fc_out.weight"].astype(np.float64), sd["fc_out.bias"].astype(np.float64)
    logits = y.mean(1) @ fw.T + fb
    bound = b.mean(1) @ np.abs(fw).T + REL * (np.abs(y).mean(1) @ np.abs(fw).T + np.abs(fb)) + ABS
    return logits, bound


def copies_ref(sd, X, copies, is_resi=True):
    """X [B, V, copies * F_in] -> (logits [B, C], bound, per-copy logits [B, copies, C])."""
    F = X.shape[2] // copies
    per = [network_ref(sd, X[:, :, i * F:(i + 1) * F], is_resi) for i in range(copies)]
    cl = np.stack([p[0] for p in per], 1)
    bound = np.stack([p[1] for p in per], 1).mean(1) + copies * 2.0 ** -24 * np.abs(cl).mean(1)
    return cl.mean(1), bound, cl


def ordered_mean_f32(copy_logits):
    """[B, copies, C] float32 -> the rule's mean: the sum over i ascending in float32 from +0, then
    one float32 division."""
    s = np.zeros(copy_logits.shape[::2], np.float32)
    for i in range(copy_logits.shape[1]):
        s = (s + copy_logits[:, i, :]).astype(np.float32)
    return (s / np.float32(copy_logits.shape[1])).astype(np.float32)


# ------------------------------------------------------------------------------------ seeded cases
def _seed(name):
    return int.from_bytes(hashlib.sha256(("tgcn_" + name).encode()).digest()[:4], "little")


def make_model(name, V, F, H, C, S, var=None, w_scale=1.0, shift=0.0):
    """A seeded model: W and att scaled so that pre-activations are O(1) (times w_scale), gamma in
    [0.5, 1.5], beta and running_mean ~ 0.1 N (beta + shift), running_var in [0.5, 1.5] (or var
    everywhere)."""
    rng = np.random.default_rng(_seed(name))
    sd = {}
    fin = F
    for gc, bn in layer_keys(S):
        sd[gc + ".weight"] = (rng.standard_normal((fin, H)) * w_scale / np.sqrt(fin)).astype(np.float32)
        sd[gc + ".att"] = (rng.standard_normal((V, V)) / np.sqrt(V)).astype(np.float32)
        sd[gc + ".bias"] = (0.1 * rng.standard_normal(H)).astype(np.float32)
        sd[bn + ".weight"] = rng.uniform(0.5, 1.5, V * H).astype(np.float32)
        sd[bn + ".bias"] = (0.1 * rng.standard_normal(V * H) + shift).astype(np.float32)
        sd[bn + ".running_mean"] = (0.1 * rng.standard_normal(V * H)).astype(np.float32)
        if var is not None:  # a large |a|: keep (bias - running_mean) * a of order 1
            sd[bn + ".running_mean"] = (np.tile(sd[gc + ".bias"], V) +
                                        np.sqrt(var + BN_EPS) * rng.standard_normal(V * H)).astype(np.float32)
        sd[bn + ".running_var"] = (rng.uniform(0.5, 1.5, V * H) if var is None else np.full(V * H, var)).astype(np.float32)
        fin = H
    sd["fc_out.weight"] = (rng.standard_normal((C, H)) / np.sqrt(H)).astype(np.float32)
    sd["fc_out.bias"] = (0.1 * rng.standard_normal(C)).astype(np.float32)
    return sd


def make_input(name, B, V, F):
    return np.random.default_rng(_seed(name + "_x")).standard_normal((B, V, F)).astype(np.float32)


# one layer through the debug hook: name -> V, F, H, B and what it covers
LAYER_CASES = {
    "ref_55_64_64": dict(V=55, F=64, H=64, B=3),      # the reference geometry, padded rows 55..63
    "full_64_64_64": dict(V=64, F=64, H=64, B=2),
    "smallest_1_1_1": dict(V=1, F=1, H=1, B=1),
    "odd_17_50_100": dict(V=17, F=50, H=100, B=3),    # K and N no multiple of any tile
    "k_limit_64_1024_8": dict(V=64, F=1024, H=8, B=2),
    "n_limit_64_8_1024": dict(V=64, F=8, H=1024, B=2),
    # a running_var of 1e-8: |a| ~ 300; W scaled down so that the layer is not saturated throughout
    "large_a_55_32_32": dict(V=55, F=32, H=32, B=2, var=1e-8, w_scale=1e-3),
    "saturated_plus_55_32_32": dict(V=55, F=32, H=32, B=2, shift=50.0),
    "saturated_minus_55_32_32": dict(V=55, F=32, H=32, B=2, shift=-50.0),
    "tiny_55_32_32": dict(V=55, F=32, H=32, B=2, w_scale=1e-6, zero_c=True),
}


@functools.lru_cache(maxsize=None)
def layer_case(name):
    """(model of one stem layer, x float32 [B, V, F], residual float32 [B, V, H], and per residual
    (False, True) the float64 statement and its bound); shared, never modified."""
    c = LAYER_CASES[name]
    sd = make_model(name, c["V"], c["F"], c["H"], 2, 0, c.get("var"), c.get("w_scale", 1.0), c.get("shift", 0.0))
    if c.get("zero_c"):  # pre-activations of the products' own size: c = 0 exactly
        sd["bn1.bias"][:] = 0
        sd["bn1.running_mean"] = np.tile(sd["gc1.bias"], c["V"])
    x = make_input(name, c["B"], c["V"], c["F"])
    res = make_input(name + "_res", c["B"], c["V"], c["H"])
    refs = {False: layer_ref(sd, "gc1", "bn1", x.astype(np.float64)),
            True: layer_ref(sd, "gc1", "bn1", x.astype(np.float64), None, res.astype(np.float64))}
    return sd, x, res, refs


def _full_mantissa(rng, shape):
    """random fp32 with full mantissas, magnitudes in [0.5, 2), both signs"""
    m = rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    e = rng.integers(126, 128, shape, dtype=np.uint32)
    s = rng.integers(0, 2, shape, dtype=np.uint32)
    return ((s << 31) | (e << 23) | m).view(np.float32)


ONE_HOT_GEOM = dict(V=55, F=50, H=100)
# (v, k): first and last row and column, and one interior pair
ONE_HOT_AT = [(0, 0), (0, 49), (54, 0), (54, 49), (23, 31)]


@functools.lru_cache(maxsize=None)
def one_hot_model():
    """Full-mantissa W and att, a = gamma (running_var = 1 - eps in float64 is not exact, so the
    statement uses fold's a) and c = 0 exactly (beta = 0, running_mean = bias): every output is one
    product a * att[v', v] * x * W[k, f]."""
    g = ONE_HOT_GEOM
    rng = np.random.default_rng(_seed("one_hot"))
    sd = make_model("one_hot", g["V"], g["F"], g["H"], 2, 0)
    sd["gc1.weight"] = _full_mantissa(rng, (g["F"], g["H"]))
    sd["gc1.att"] = _full_mantissa(rng, (g["V"], g["V"]))
    sd["bn1.weight"] = (_full_mantissa(rng, g["V"] * g["H"]) * np.float32(0.25)).astype(np.float32)
    sd["bn1.bias"][:] = 0
    sd["bn1.running_mean"] = np.tile(sd["gc1.bias"], g["V"])
    return sd, float(_full_mantissa(rng, 1)[0])


def one_hot_expected(sd, xval, v, k):
    """(expected output [V, H] float64, tolerance): tanh(a * att[:, v] * x * W[k, :]) within
    (2 * ONE_HOT + 2^-23) of the product -- each of the two matrix products one single-term output,
    the multiply by a one more rounding -- plus tanhf's own error."""
    a, c = fold(sd, "gc1", "bn1")
    assert not c.any()
    p = a.astype(np.float64) * np.outer(sd["gc1.att"][:, v].astype(np.float64),
                                        xval * sd["gc1.weight"][k, :].astype(np.float64))
    return np.tanh(p), (2 * ONE_HOT + 2.0 ** -23) * np.abs(p) + TANHF


# ------------------------------------------------------------------------------------ golden cases
GOLDEN_CASES = {
    "g0_f16_h32_c10_s2": dict(F=16, H=32, C=10, S=2, is_resi=True),
    "g1_f24_h48_c7_s1_plain": dict(F=24, H=48, C=7, S=1, is_resi=False),
}
GOLDEN_V, GOLDEN_B, GOLDEN_COPIES = 55, 6, 4


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """(model, X float32 [B, 55, 4 F], the reference's float32 CPU logits [B, C], meta) of
    tests/golden/tgcn_ref.npz (scripts/gen_tgcn_golden.py)."""
    d = np.load(os.path.join(GOLDEN, "tgcn_ref.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "tgcn_ref.json")))["cases"][name]
    pre = name + "/"
    sd = {k[len(pre) + 3:]: d[k] for k in d.files if k.startswith(pre + "sd/")}
    return sd, d[pre + "X"], d[pre + "logits"], meta


@functools.lru_cache(maxsize=None)
def golden_ref(name):
    sd, X, _, _ = golden_case(name)
    return copies_ref(sd, X, GOLDEN_COPIES, GOLDEN_CASES[name]["is_resi"])


@functools.lru_cache(maxsize=None)
def small_net_case():
    """V = 46 (the posehand feature rows), no block: against the statement alone."""
    sd = make_model("v46_s0", 46, 20, 40, 5, 0)
    X = make_input("v46_s0", 5, 46, 3 * 20)
    return sd, X, copies_ref(sd, X, 3)


# ------------------------------------------------------------------------------------ clip_inputs
def clip_inputs_loop(data, ranges, num_samples, copies):
    """clip_inputs restated as plain loops."""
    data = np.asarray(data)
    out = np.zeros((len(ranges), data.shape[1], copies * 2 * num_samples), np.float32)
    for n, (b, e) in enumerate(ranges):
        ln = e - b
        for k in range(num_samples):
            for i in range(copies):
                j = k * copies + i
                t = b + (j * ln) // (copies * num_samples)
                for v in range(data.shape[1]):
                    for c in range(2):
                        out[n, v, i * 2 * num_samples + 2 * k + c] = data[t, v, c]
    return out
