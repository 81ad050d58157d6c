"""The attention per-op tests' reference cannot hide a failure (no GPU needed).  On the very inputs
tests/test_gpu_attn_ops.py runs (attn_ref's case lists):

  * the operand families are what they claim: the peaked key holds p >= 0.999 with a margin >= 30, rising /
    falling scores are monotone with the stated step, large scores would overflow exp() in fp32, tied scores tie;
  * every wrong variant of the reference leaves the bound on at least one named case (and the GPU test asserts
    that bound on that case): the mask off by one either way, the stale cache row at pos, row_slot ignored,
    layer_off ignored, the wrong kv head, no rescale of the accumulator, a split's partial dropped, RoPE at pos +- 1;
  * the fast-path form of the reference (every documented rounding applied) lies inside the derived fast bound
    of the exact form.  A fast-path rounding OMITTED does not separate, and cannot: the bound is the sum of the
    roundings, so a kernel that skips one moves towards the exact form (asserted: such variants stay inside).

Where a variant is caught says what it takes: mask-1 needs weight on the last key (peaked there, rising, a short
tied context), no_rescale a maximum that rises between passes (rising, or a peak past the first pass), drop_split
weight in the last split, RoPE at pos +- 1 scores that depend on the angle (diffuse, large: the peaked key stays
the peak under a rotation of one position, and is not listed for it)."""
import numpy as np
import pytest

import attn_ref as ar

FORM_SHAPES = [(form, shape) for form, v in ar.SLOW_FORMS.items() for shape in v[4]]


def _tol(c, flash=False):
    return ar.SLOW_TOL["bf16_flash" if flash else c["precision"]]


def _caught(cases, mut, **kw):
    """the cases (family, pos) on which variant `mut` leaves the slow-path bound"""
    hit = []
    for c in cases:
        ref = ar.reference(c)[0]
        if not ar.rel_err(ar.reference(c, mut=mut, **kw)[0], ref) <= _tol(c):
            hit.append((c["family"], c["pos"].tolist()))
    return hit


@pytest.fixture(scope="module")
def fd4():
    return ar.slow_form_cases("fd4", "bf16", (4, 1, 128))


@pytest.mark.parametrize("form, shape", FORM_SHAPES)
def test_families_are_what_they_claim(form, shape):
    cases = ar.slow_form_cases(form, "bf16", shape) + ar.peak_walk_cases(form, "bf16", shape)
    seen = set()
    for c in cases:
        assert np.isnan(c["kc"][0, 0, :, int(c["pos"][0]):]).all() and np.isnan(c["vc"][0, 0, :, int(c["pos"][0]):]).all()
        assert np.isfinite(ar.reference(c)[0]).all()
        n, fam = int(c["pos"][0]), c["family"]
        seen.add(fam)
        for s, p in ar.probs(c)[0]:
            if fam == "peaked":
                pk = int(c["peak"][0])
                assert p[pk] >= 0.999 and (n == 0 or s[pk] - np.delete(s, pk).max() >= 30), (form, shape, n, pk)
            elif fam in ("rising", "falling") and n > 0:
                step, sign = min(3.0, 280.0 / n), (1 if fam == "rising" else -1)
                # the keys' rounding (2^-8 of |s| <= 280) blurs a step: monotone position by position where the
                # step is 3 units, and by at least 2 units over any wave's 16 positions everywhere
                d, d16 = np.diff(s) * sign, (s[16:] - s[:-16]) * sign
                assert np.abs(d - step).max() <= 2 * 280 * ar.U and (step < 3 or (d > 0).all()), (form, shape, n, d.min())
                assert (d16 >= 2).all(), (form, shape, n)
                assert int(np.argmax(s)) == (n if fam == "rising" else 0)
            elif fam == "large":
                with np.errstate(over="ignore"):
                    assert s.min() > 55 and s.max() < 105 and (n < 31 or np.exp(np.float32(s.max())) == np.inf)
            elif fam == "tied":
                assert (s == 0).all() and np.ptp(p) == 0
    assert seen == set(ar.FAMILIES)


def test_mask_off_by_one_and_stale_row_are_caught(fd4):
    # rows > pos and the stale row pos are NaN: one key too many, or the stale row, is never finite
    assert len(_caught([c for c in fd4 if c["pos"][0] < c["S"] - 1], "mask+1")) == len(fd4) - 6
    assert len(_caught(fd4, "stale_row")) == len(fd4)
    hit = _caught(fd4, "mask-1")
    fams = {f for f, _ in hit}
    assert {"rising", "peaked", "tied", "diffuse"} <= fams, hit
    # the deepest catch: a peak on the last key is caught at any depth, where a diffuse row's share is 1 / pos
    assert ("peaked", [max(c["pos"][0] for c in fd4)]) in hit or any(f == "rising" and p[0] > 500 for f, p in hit), hit


@pytest.mark.parametrize("form, shape", [("fd8", (6, 2, 128)), ("decode2", (8, 2, 128)), ("dec3", (4, 2, 64))])
def test_slot_layer_and_kv_head_are_caught(form, shape):
    cases = ar.slot_cases(form, "bf16", shape)
    for mut in ("no_slot", "no_layer"):
        assert len(_caught(cases, mut)) == len(cases), mut  # the other slots and layer 0 are NaN
    hit = _caught(cases + ar.slow_form_cases(form, "bf16", shape)[:12], "kv_head")
    assert {"peaked", "rising", "diffuse", "large"} <= {f for f, _ in hit}, hit


@pytest.mark.parametrize("form", ["fd4", "fd8", "fd16", "decode2", "dec3"])
def test_rescale_and_dropped_split_are_caught(form):
    kernel, nw, cap, S, shapes = ar.SLOW_FORMS[form]
    cases = ar.slow_form_cases(form, "bf16", shapes[0]) + ar.peak_walk_cases(form, "bf16", shapes[0])
    hit = _caught(cases, "no_rescale", tile=16 * nw)  # the kernel's own pass
    assert any(f == "rising" for f, _ in hit) and any(f == "peaked" for f, _ in hit), hit
    nsp_max = ar.form_nsp_max(kernel)
    for c in cases:  # the split each case is cut into: the variant drops the last one
        c["_split"] = ar.fd_split(int(c["pos"][0]) + 1, cap, nsp_max)[1]
    hit = [(c["family"], c["pos"].tolist()) for c in cases
           if not ar.rel_err(ar.reference(c, mut="drop_split", split=c["_split"])[0], ar.reference(c)[0]) <= _tol(c)]
    assert {"rising", "peaked", "diffuse", "tied"} <= {f for f, _ in hit}, hit


def test_fp32_large_needs_its_own_bound():
    """At |s| ~ 100 fp32 itself misses 2e-5: the float32 restatement of the definition does, so the fp32 `large` cases
    are held to 2e-5 + 4 x its error (attn_ref.fp32_large_tol, never above 2e-4); the wrong variants are outside
    that, and every other family's restatement is inside the 2e-5 with room."""
    worst, worst_other = 0.0, 0.0
    for form, shape in (("fd4", (4, 1, 128)), ("fd4", (3, 1, 64)), ("decode2", (5, 1, 32))):
        for c in ar.slow_form_cases(form, "fp32", shape):
            if c["pos"][0] < 31:
                continue
            f32 = ar.float32_restatement(c)
            if c["family"] != "large":
                worst_other = max(worst_other, ar.rel_err(f32, ar.reference(c)[0]))
                continue
            worst = max(worst, ar.rel_err(f32, ar.reference(c)[0]))
            assert ar.slow_share(c, f32) <= 0.25 + 1e-9 and ar.fp32_large_tol(c) <= 2e-4
            for mut in ("rope+1", "mask+1") + (("no_rescale",) if c["pos"][0] >= 511 else ()):
                if c["pos"][0] < c["S"] - 1:
                    assert ar.slow_share(c, ar.reference(c, mut=mut)[0]) > 1.0, (mut, c["pos"])
    assert worst > 2e-5 and worst_other < 2e-6, (worst, worst_other)


def test_rope_position_is_caught(fd4):
    for mut in ("rope+1", "rope-1"):
        hit = _caught([c for c in fd4 if 0 < c["pos"][0] < c["S"] - 1], mut)
        assert {"diffuse", "large"} <= {f for f, _ in hit}, (mut, hit)
        # and the new key itself moves by far more than the 1-ulp bound it is held to
        c = fd4[7]
        k, kw = ar.reference(c)[1], ar.reference(c, mut=mut)[1]
        assert (np.abs(k - kw) > 4 * ar.ulp(k, "bf16")).mean() > 0.3


@pytest.mark.parametrize("shape", ar.FAST_SHAPES)
@pytest.mark.parametrize("cpos, S", [(0, 16), (1, 16), (7, 16), (15, 16), (16, 24), (20, 24)])
def test_fast_path_form_inside_bound_and_variants_outside(shape, cpos, S):
    for c in ar.fast_cases(shape, "bf16", cpos, S, R=3):
        exact, _, _, bound = ar.reference(c, bound=True)
        assert np.isfinite(bound).all()
        if c["family"] in ("diffuse", "peaked", "tied"):  # (a bf16 score of 70 has an ulp of 0.5: large / rising are loose)
            assert (bound < 0.2 * np.abs(c["qkv"][:, -c["nkv"] * c["hd"]:]).max()).all(), float(bound.max())
        fast = ar.reference(c, fast=True)[0]
        assert (np.abs(fast - exact) <= bound).all(), (c["family"], float((np.abs(fast - exact) / bound).max()))
        for mut in ("no_round_s", "no_round_p", "no_round_o"):  # an omitted rounding stays inside: see the docstring
            assert (np.abs(ar.reference(c, fast=True, mut=mut)[0] - exact) <= bound).all(), mut
        for mut in ("mask+1", "stale_row", "no_slot", "no_layer"):
            if (mut == "mask+1" and cpos == S - 1) or (mut in ("no_slot", "no_layer") and cpos == 0):
                continue  # (nothing past the last row; at cpos 0 no cache row is read, only written)
            assert not (np.abs(ar.reference(c, mut=mut)[0] - exact) <= bound).all(), (c["family"], mut)
        if c["family"] == "peaked":
            for r in range(c["R"]):  # the output is that V row (or the new v) within the bound
                pk = int(c["peak"][r])
                v = ar.reference(c)[2][r] if pk == cpos else c["vc"][c["row_slot"][r], c["layer"], :, pk].astype(np.float64)
                g = c["nh"] // c["nkv"]
                assert (np.abs(exact[r] - np.repeat(v, g, axis=0)) <= 1e-9).all()
        if cpos > 0 and c["family"] in ("rising", "tied"):
            assert not (np.abs(ar.reference(c, mut="mask-1")[0] - exact) <= bound).all(), c["family"]
        if c["nkv"] > 1 and c["nh"] > c["nkv"] and c["family"] != "tied":
            assert not (np.abs(ar.reference(c, mut="kv_head")[0] - exact) <= bound).all(), c["family"]
