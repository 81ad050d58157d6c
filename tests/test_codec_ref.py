"""The codec per-op tests' reference cannot hide a failure (no GPU needed): on the GPU tests' own inputs
(codec_ref's case builders) a deliberately wrong float64 variant exceeds the bound e on at least 1 % of the
elements, for every mutant of every family it applies to, and a model of the kernel -- the restatement r, the
chain with every rounding applied -- lies within e of t everywhere.

A mutant is run on the cases of its family where the wrong variant computes something else at all (a dropped
bias needs a bias, a context mutant needs rows that read context, a window that is one key off needs rows
whose window is full); the choice is written at each test."""
import math

import numpy as np
import pytest

import codec_ref as cr
from codec_ref import CE_GAMMA, CE_RES, CE_ROPE, CE_SWIGLU
from linear_ref import mk, rb

MIN_SHARE = 0.01


def _share(ref, wrong):
    """share of elements where the wrong variant's value is outside the bound around the right one"""
    return float(np.mean(np.abs(wrong.t - ref.t) > ref.e))


def _conv_mutants(c):
    k, kind, full = c["k"], c["kind"], (c["k"] - 1) * c["dil"]
    m = []
    # a context mutant moves only the rows whose taps reach below row 0 ((k - 1) dil of them, one for the two-tap
    # transposed and strided convs): it is run where those are at least 2 % of the rows
    reach = (full if kind == 0 and not c["strided"] else 1) >= 0.02 * c["Lq"]
    if kind == 0 and not c["strided"] and k > 1:
        m.append("taps_rev")
        if c["Lq"] + c["npre"] > full:  # some row reads taps 0 and 1 inside the data
            m += ["tap01", "dil+1", "dil-1"]
        if c["npre"] < full and c["Lq"] > 1 and reach:
            m.append("zero_ctx")  # rows below lo read as data instead of causal zeros
    if kind == 1:
        m += ["phase_swap", "tap01"]
        if c["npre"] == 0 and reach:
            m.append("zero_ctx")
    if kind == 2:
        m.append("phase_swap")
    if c["strided"] and c["npre"] == 0 and reach:
        m.append("zero_ctx")
    if c["npre"] > 0 and k > 1 and reach:
        m.append("ctx_zero")  # the carried context rows read as zeros
    if c["bias"] is not None and not c["flags"] & CE_SWIGLU:
        m.append("no_bias")
    if c["flags"] & CE_GAMMA:
        m.append("no_gamma")
    if c["flags"] & CE_RES and kind in (1, 2) and c["Lq"] > 1:
        m.append("res_row")
    if c["flags"] & CE_ROPE:
        m.append("rope_pos")
    if c["alpha2"] is not None:
        m.append("snake_sin")
    return m


ALL_CONV = cr.conv_cases() + cr.tconv_cases() + cr.strided_cases() + cr.splitk_cases()


@pytest.mark.parametrize("c", ALL_CONV, ids=[c["name"] for c in ALL_CONV])
def test_conv_bounds_are_sharp_and_hold_for_the_restatement(c):
    ref = cr.conv_ref(c)
    for key, v in ref.items():
        assert (np.abs(v.r - v.t) <= v.e).all(), (c["name"], key)
    for mut in _conv_mutants(c):
        wrong = cr.conv_ref(c, mut)
        # the output a mutant shows in: the Snake mutant in out2 only, the others in whatever the case stores
        keys = ["out2"] if mut == "snake_sin" else list(ref)
        share = max(_share(ref[k], wrong[k]) for k in keys)
        assert share >= MIN_SHARE, (c["name"], mut, share)


@pytest.mark.parametrize("c", cr.conv2_cases()[:6], ids=[c["name"] for c in cr.conv2_cases()[:6]])
def test_conv2_restatement_within_bound(c):
    for key, v in cr.conv_ref(c).items():
        assert (np.abs(v.r - v.t) <= v.e).all(), (c["name"], key)
    for mut in ("taps_rev", "no_bias", "snake_sin"):
        if mut in _conv_mutants(c):
            ref, wrong = cr.conv_ref(c), cr.conv_ref(c, mut)
            assert max(_share(ref[k], wrong[k]) for k in (["out2"] if mut == "snake_sin" else list(ref))) >= MIN_SHARE


def test_every_conv_mutant_is_exercised():
    seen = set()
    for c in ALL_CONV:
        seen.update(_conv_mutants(c))
    assert seen == {"taps_rev", "tap01", "dil+1", "dil-1", "zero_ctx", "ctx_zero", "phase_swap", "no_bias", "no_gamma",
                    "res_row", "rope_pos", "snake_sin"}


@pytest.mark.parametrize("C,dil,npre", [(64, 1, 0), (96, 3, 18), (96, 9, 18)])
def test_resunit_reference(C, dil, npre):
    c = cr.resunit_case(C, dil, npre, True)
    ref = cr.resunit_ref(c)
    for key, v in ref.items():
        assert (np.abs(v.r - v.t) <= v.e).all(), key
    muts = ["taps_rev", "tap01", "dil+1", "dil-1", "no_bias", "snake_sin"] + (["ctx_zero"] if npre else []) \
        + (["zero_ctx"] if npre < 6 * dil else [])
    for mut in muts:
        wrong = cr.resunit_ref(c, mut)
        assert _share(ref["out2"], wrong["out2"]) >= MIN_SHARE and _share(ref["res"], wrong["res"]) >= MIN_SHARE, mut


# window one key too long / too short: rows whose window is full (Tn = window + 5 has 6 + npre of them); at 128
# and 512 keys one key's weight is below the bf16 rounding of the output, so those windows are run in fp32, and 512
# with npre = 511, where every row's window is full
@pytest.mark.parametrize("prec,window,hd,npre", [("bf16", 16, 32, 0), ("bf16", 16, 64, 3), ("fp32", 16, 32, 15),
                                                 ("fp32", 128, 64, 0), ("fp32", 128, 32, 3), ("fp32", 512, 32, 511)])
def test_window_attn_reference(prec, window, hd, npre):
    H, Tn = 2, window + 5
    qkv = mk(np.random.default_rng([window, hd, npre]), (npre + Tn, 3 * H * hd), prec)
    ref = cr.attn_ref(qkv, Tn, H, hd, window, npre, prec)
    assert (np.abs(ref.r - ref.t) <= ref.e).all()
    muts = ["win+1", "win-1"] + (["no_clamp"] if npre < window - 1 else [])
    for mut in muts:
        assert _share(ref, cr.attn_ref(qkv, Tn, H, hd, window, npre, prec, mut)) >= MIN_SHARE, mut


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_rope_reference(prec):
    H, hd, Tn, pos0 = 3, 32, 37, 1000
    x = mk(np.random.default_rng([pos0, hd]), (Tn, 3 * H * hd), prec)
    tab = cr.rope_table(pos0 + Tn + 2, hd, 10000.0)
    ref = cr.rope_ref(x, Tn, H, hd, tab, pos0, prec)
    assert (np.abs(ref.r - ref.t) <= ref.e).all()
    assert _share(ref, cr.rope_ref(x, Tn, H, hd, tab, pos0, prec, "rope_pos")) >= MIN_SHARE


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("D,npre", [(128, 6), (2048, 2)])
def test_dwconv_ln_reference(prec, D, npre):
    L = 19
    rng = np.random.default_rng([D, npre])
    x = mk(rng, (npre + L, D), prec)
    dw, db = mk(rng, (D, 7), prec, 1 / math.sqrt(7)), mk(rng, (D,), prec, 0.5)
    lw, lb = rb(prec)((1 + 0.1 * rng.standard_normal(D)).astype(np.float32)), mk(rng, (D,), prec, 0.1)
    ref = cr.dwconv_ln_ref(x, L, D, npre, dw, db, lw, lb, prec)
    assert (np.abs(ref.r - ref.t) <= ref.e).all()
    for mut in ("dw_rev", "ctx_zero") + (("zero_ctx",) if npre < 6 else ()):
        assert _share(ref, cr.dwconv_ln_ref(x, L, D, npre, dw, db, lw, lb, prec, mut)) >= MIN_SHARE, mut


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_snake_reference(prec):
    x, alpha = cr.snake_case(prec)
    ref = cr.snake_ref(x, alpha, prec)
    assert (np.abs(ref.r - ref.t) <= ref.e).all()
    assert _share(ref, cr.snake_ref(x, alpha, prec, "sin")) >= MIN_SHARE
    assert cr.DELTA_SIN == 2 * cr.DELTA_SIN_MEASURED and cr.DELTA_SIN <= cr.DELTA_SIN_CAP == 2.0 ** -16


def test_delta_sin_estimator_recovers_a_planted_error():
    """delta_sin_from on a simulated fp32 Snake whose sine is off by a known amount"""
    y = np.linspace(0, cr.TWO_PI, 1 << 16, endpoint=False).astype(np.float32)
    rev = (y * np.float32(0.159154943091895336)).astype(np.float32)
    fr = (rev - np.floor(rev)).astype(np.float64)
    for planted in (0.0, 3e-7, 5e-6):
        s = (np.sin(cr.TWO_PI * fr) + planted).astype(np.float32)
        got = (y + (s * s).astype(np.float32)).astype(np.float32)
        d = cr.delta_sin_from(y, got).max()
        assert d <= planted + 2.0 ** -24 and d >= 0.5 * planted, (planted, d)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_short_chain_references(prec):
    rng = np.random.default_rng(3)
    g, u = mk(rng, (5000,), prec, 3.0), mk(rng, (5000,), prec)
    v = cr.silu_mul_ref(g, u, prec)
    assert (np.abs(v.r - v.t) <= v.e).all()
    w = cr.wn_fold_ref(mk(rng, (5,), "fp32"), mk(rng, (5, 300), "fp32"))
    assert (np.abs(w.r - w.t) <= w.e).all()
    nq1, D, sem, cbs, cd, Tn = 10, 1024, 64, 32, 8, 9
    cb_sem, cb = mk(rng, (sem, cd), "fp32"), mk(rng, (nq1 - 1, cbs, cd), "fp32")
    wt, b = mk(rng, (nq1, D, cd), "fp32", 1 / math.sqrt(cd)), mk(rng, (nq1, D), "fp32", 0.5)
    codes = rng.integers(0, cbs, (nq1, Tn)).astype(np.int32)
    z = cr.rvq_ref(codes, cb_sem, cb, wt, b, prec)
    assert (np.abs(z.r - z.t) <= z.e).all()
    codes2 = codes.copy()
    codes2[1] = (codes2[1] + 1) % cbs  # one stage reads the neighbouring codebook row
    assert _share(z, cr.rvq_ref(codes2, cb_sem, cb, wt, b, prec)) >= MIN_SHARE


@pytest.mark.parametrize("cbn,seed", cr.VQ_CASES)
def test_vq_encode_undecided_share_is_within_its_cap(cbn, seed):
    """at most 2 % of the (frame, stage) pairs have a second candidate within the fp32 error of the distance, the
    reference's own choice is acceptable everywhere, and the restated residual lies within its bound"""
    c = cr.vq_case(cbn, seed)
    codes, ok, und, r = cr.vq_ref(c)
    assert und.mean() <= cr.VQ_UNDECIDED_CAP, und.mean()
    assert ok.all() and (np.abs(r.r - r.t) <= r.e).all()
    # a wrong chain: one stage picks the second-best row
    d = codes.copy()
    d[3] = (d[3] + 1) % cbn[3]
    _, ok2, _, r2 = cr.vq_ref(c, got_codes=d)
    assert not ok2[3].any() and _share(r, r2) >= MIN_SHARE
