"""Per-op attention tests: the launch forms of the attention kernels (fm_attn.hip, fm_llm_kernels.hip, fm_rowgemv.hip) through
the fm_op_* hooks (each runs the production launcher on caller operands) against the float64 reference of
tests/attn_ref.py, on its operand families and under its bounds (derived there; tests/test_attn_ref.py shows on
these very inputs that the reference's wrong variants leave them).

Every case poisons what the kernel must not read: cache rows > pos, the stale row pos itself, every other slot
and layer are NaN, and so are the split partials no block writes.  After the launch the output is finite and
inside the bound, the row pos holds the reference's new k (QK_ROPE_ULPS) and the raw v, every other cache word has
its bits unchanged, no ticket word is left non-zero and the guard behind the partials is intact.

  slow decode   attn_fd x nwb {4, 8, 16}, attn_decode2, attn_dec3; bf16 and fp32; positions from the kernels' own
                constants (attn_ref.fd_positions); the frame's own (nwb, cap) for R = 1, 8, 9; shuffled slots in a
                two-layer cache; the slab form of the QKV input; a repeated launch
  prefill       qk_rope_cache_kernel; attn_prefill_kernel and attn_split + attn_combine on ragged chunks after a
                prefix, in a non-zero slot and layer; the many-slot split + combine
  fast decoder  fast_attn2 (and noq), fast_attn_fused, qk_rope_cache(fixed_pos) + fast_attn_kernel at every
                codebook position, under the fast-path bound; DESIGN.md claims none of these three bit-identical
                to another (their dot products sum in different orders), so each is held to the bound; the noq
                form is documented as the full form's bits (fm_kernels.h FastFusedArgs::noq) and held to them

  fused attention + wo   fattn_wo_kernel / fattn_wo_pair_kernel (the batch-1 production path) at every codebook
                position in bf16, int8 and int4: the bits of the launches it replaces and of ops.rowgemv on the
                fast_attn2 hook's output, ilp 0 = 1, the gathered residual, the table form and its clamp, the
                K / V-only form on a NaN Q, stale tagged words, pair 1 and 2 against two one-row launches; err == 0

Each test prints its worst error next to the bound (DESIGN.md's table is copied from a run on the MI355X)."""
import numpy as np
import pytest

import attn_ref as ar
from fishmi import native, ops

pytestmark = pytest.mark.gpu

PRECISIONS = ["bf16", "fp32"]
FP32_LARGE = []  # shares of attn_ref.fp32_large_tol the fp32 `large` cases used (printed with each test's worst error)
FORM_SHAPES = [(form, shape) for form, v in ar.SLOW_FORMS.items() for shape in v[4]]


def _check_cache(c, r, kc_in, kc_out, vc_in, vc_out, knew, vnew, touched):
    """row pos[r] of the row's slot and layer: the reference's new k within the qk_rope bound, the raw v's bits"""
    slot, n, prec = int(c["row_slot"][r]), int(c["pos"][r]), c["precision"]
    k = kc_out[slot, c["layer"], :, n]
    assert np.isfinite(k).all()
    d = np.abs(k - knew[r].astype(np.float32))
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    unit = ar.prep_unit(c["qkv"][r, nh * hd:(nh + nkv) * hd].reshape(nkv, hd), c["kn"], np.maximum(np.abs(k), np.abs(knew[r])),
                        prec, ar.rb(prec))
    assert (d <= ar.QK_ROPE_ULPS[prec] * unit).all(), (r, float((d / unit).max()))
    np.testing.assert_array_equal(ar.bits(vc_out[slot, c["layer"], :, n]), ar.bits(vnew[r].astype(np.float32)))
    touched[slot, c["layer"], :, n] = True


def _check_untouched(c, kc_out, vc_out, touched):
    """every cache word but the rows just written: bit patterns unchanged (NaN poison included)"""
    keep = ~touched
    np.testing.assert_array_equal(ar.bits(kc_out)[keep], ar.bits(c["kc"])[keep])
    np.testing.assert_array_equal(ar.bits(vc_out)[keep], ar.bits(c["vc"])[keep])


def _decode(c, kernel="fd", nwb=4, cap=32, frame=False, reps=1, qkv=None, slab=None, bias=None):
    return ops.decode_attn_ex(c["nh"], c["nkv"], c["hd"], c["row_slot"], c["pos"], c["kc"], c["vc"], c["rope_base"],
                              qkv=(c["qkv"] if qkv is None and slab is None else qkv), slab=slab, bias=bias, qn=c["qn"],
                              kn=c["kn"], layer=c["layer"], precision=c["precision"], kernel=kernel, nwb=nwb, cap=cap,
                              frame=frame, reps=reps)


def _check_decode(c, res, tol=None):
    """all the properties of the module docstring for one slow decode launch; returns the worst relative error (the
    fp32 `large` cases report their share of fp32_large_tol to FP32_LARGE instead)"""
    out, kco, vco, info = res
    assert np.isfinite(out).all(), (c["family"], c["pos"].tolist(), info)
    ref, knew, vnew = ar.reference(c)
    share = ar.slow_share(c, out, tol)  # (fp32 `large`: under attn_ref.fp32_large_tol)
    assert share <= 1.0, (c["family"], c["pos"].tolist(), c["peak"].tolist(), info, share)
    tol = ar.SLOW_TOL[c["precision"]] if tol is None else tol
    if c["family"] == "peaked":  # the output is that V row
        for r in range(c["R"]):
            pk, n = int(c["peak"][r]), int(c["pos"][r])
            v = vnew[r] if pk == n else c["vc"][c["row_slot"][r], c["layer"], :, pk].astype(np.float64)
            assert ar.rel_err(out[r], np.repeat(v, c["nh"] // c["nkv"], axis=0)) <= tol
    assert info["tickets"] == 0 and info["guard_ok"] == 1 and info["fd_nsp"] == ar.FD_NSP, info
    touched = np.zeros(c["kc"].shape, bool)
    for r in range(c["R"]):
        _check_cache(c, r, c["kc"], kco, c["vc"], vco, knew, vnew, touched)
    _check_untouched(c, kco, vco, touched)
    if c["precision"] == "fp32" and c["family"] == "large":
        FP32_LARGE.append(share)
        return 0.0
    return share * tol


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("form, shape", FORM_SHAPES)
def test_slow_decode_positions_and_families(form, shape, precision):
    """Every family at every position of fd_positions (0, a pass boundary and the row before it, cap - 1, cap,
    cap + 1, 2 cap, FD_NSP cap - 1, FD_NSP cap, a last split of one row, S - 1), the peaked key walking through
    peak_places; then the peaked key at each of its places at two depths."""
    kernel, nwb, cap, S, _ = ar.SLOW_FORMS[form]
    worst, plans = 0.0, set()
    for c in ar.slow_form_cases(form, precision, shape) + ar.peak_walk_cases(form, precision, shape):
        res = _decode(c, kernel, nwb, cap)
        worst = max(worst, _check_decode(c, res))
        info = res[3]
        assert info["kernel"] == kernel and info["nwb"] == nwb, info
        plans.add((info["kernel"], info["nwb"], info["cap"], info["splits"]))
    print(f"\n{form} {shape} {precision}: worst rel err {worst:.3g} (bound {ar.SLOW_TOL[precision]:.3g}); plans {sorted(plans)}"
          + (f"; fp32 large: worst share of fp32_large_tol {max(FP32_LARGE):.3g}" if precision == "fp32" and FP32_LARGE else ""))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("form, shape", [(f, ar.SLOW_FORMS[f][4][i]) for f in ar.SLOW_FORMS for i in (0, 1)])
def test_slow_decode_shuffled_slots_and_layers(form, shape, precision):
    """R = 1, 3, 9 rows in shuffled non-contiguous slots of a two-layer cache, layer 1: a kernel that indexed the
    cache by row, or dropped layer_off, reads NaN and writes where the comparison sees it."""
    kernel, nwb, cap, _, _ = ar.SLOW_FORMS[form]
    worst = 0.0
    for c in ar.slot_cases(form, precision, shape):
        assert c["layer"] == 1 and sorted(c["row_slot"]) != list(range(c["R"]))
        worst = max(worst, _check_decode(c, _decode(c, kernel, nwb, cap)))
    print(f"\n{form} {shape} {precision} slots: worst rel err {worst:.3g} (bound {ar.SLOW_TOL[precision]:.3g})")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("R", [1, 8, 9])
def test_slow_decode_as_the_frame_launches_it(R, precision):
    """The launch a decode frame of R rows makes under the knobs in force (attn_slow_plan, shared with the frame):
    batch 1 .. 8 on fd_nw-wave blocks with splits of fd_min16, more rows on fd_nw_batched waves with
    fd_min_batched.  The plan the hook reports is the one the knobs spell out."""
    t = {k: native.tune_get(k) for k in ("attn_fd", "fd_nw", "fd_min16", "fd_min", "fd_nw_batched", "fd_min_batched")}
    assert t["attn_fd"] == 1
    if R <= 8:
        want = (t["fd_nw"], max(16, t["fd_min16"])) if t["fd_nw"] > 4 else (4, max(16, t["fd_min"]))
    else:
        want = (t["fd_nw_batched"] if t["fd_nw_batched"] > 4 else 4, max(16, t["fd_min_batched"]))
    worst, plans = 0.0, set()
    for c in ar.frame_cases(R, want[1], precision):
        res = _decode(c, frame=True)
        info = res[3]
        assert (info["kernel"], info["nwb"], info["cap"]) == ("fd", want[0], want[1]), (info, want)
        assert info["splits"] == min(ar.FD_NSP, -(-c["S"] // want[1]))
        worst = max(worst, _check_decode(c, res))
        plans.add((info["kernel"], info["nwb"], info["cap"], info["splits"]))
    print(f"\nframe R={R} {precision}: plan {sorted(plans)}; worst rel err {worst:.3g} (bound {ar.SLOW_TOL[precision]:.3g})")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nwb", [4, 8, 16])
def test_slow_decode_slab_form_and_repeat(nwb, precision):
    """attn_fd reading round(sum of K-part slabs + bias) (bs_qkv_slab) gives the bits of the same operands handed
    over as a rounded qkv row (kp 1, 2, 8; with and without bias; 1 and 3 rows); and a second launch on the same
    tickets and partials repeats the first one's bits."""
    shape = {4: (4, 1, 128), 8: (3, 1, 64), 16: (2, 2, 32)}[nwb]
    cases = ar.slot_cases("fd4", precision, shape)
    nh, nkv, hd = shape
    for pos, slots in (([100], [2]), ([0, 33, 215], [4, 0, 3])):  # diffuse: the cache does not depend on the row's q
        c = ar.make_case("diffuse", nh, nkv, hd, pos, 216, precision, row_slot=slots, nslots=5, layers=2, layer=1, seed=10)
        for kp in (1, 2, 8):
            for with_bias in (False, True):
                slab, bias, qkv = ar.slab_form(c, kp, with_bias)
                a = _decode(c, "fd", nwb, 32, qkv=qkv)
                b = _decode(c, "fd", nwb, 32, slab=slab, bias=bias)
                for x, y in zip(a[:3], b[:3]):
                    np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
                _check_decode(dict(c, qkv=qkv), b)
    for c in cases:
        one, two = _decode(c, "fd", nwb, 32), _decode(c, "fd", nwb, 32, reps=2)
        for x, y in zip(one[:3], two[:3]):
            np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
        assert two[3]["tickets"] == 0 and two[3]["guard_ok"] == 1
        _check_decode(c, two)


@pytest.mark.parametrize("kernel", ["slow", "slow3"])
def test_slow_decode_repeat_on_the_ticket_kernels(kernel):
    for c in ar.slot_cases("decode2" if kernel == "slow" else "dec3", "bf16", (4, 2, 64)):
        one, two = _decode(c, kernel, 4, 32), _decode(c, kernel, 4, 32, reps=2)
        for x, y in zip(one[:3], two[:3]):
            np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
        _check_decode(c, two)


# ---- prefill ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nh, nkv, hd", [(3, 1, 32), (6, 2, 64), (4, 1, 128), (3, 1, 256)])
def test_qk_rope_cache(nh, nkv, hd, precision):
    """qk_rope_cache_kernel (one wave per head; head counts 5, 10, 6, 5: the last block of four is ragged; hd 256: two pairs
    per lane): rows with their own (slot, pos) in a two-layer cache, all rows at fixed_pos, and the slab form."""
    S = 40
    rng = np.random.default_rng(hd)
    R = 5
    slots = rng.permutation(R + 3)[:R]
    pos = np.array([0, 1, 17, 31, S - 1], np.int32)
    c = ar.make_case("diffuse", nh, nkv, hd, pos, S, precision, row_slot=slots, nslots=R + 3, layers=2, layer=1, seed=8)
    c["kc"][:], c["vc"][:] = np.nan, np.nan  # nothing is read: everything is poison
    tab = ar.rope(S, hd, c["rope_base"])
    rnd = ar.rb(precision)

    def check(q, kco, vco, cc, positions):
        _, knew, vnew = ar.reference(dict(cc, pos=np.asarray(positions, np.int32), kc=np.zeros_like(cc["kc"]), vc=np.zeros_like(cc["vc"])))
        touched = np.zeros(cc["kc"].shape, bool)
        for r in range(R):
            qr = ar.prep(cc["qkv"][r, : nh * hd].astype(np.float64).reshape(nh, hd), cc["qn"], tab[positions[r]], rnd)
            d = np.abs(q[r] - qr.astype(np.float32))
            unit = ar.prep_unit(cc["qkv"][r, : nh * hd].reshape(nh, hd), cc["qn"], np.maximum(np.abs(q[r]), np.abs(qr)),
                                precision, rnd)
            assert (d <= ar.QK_ROPE_ULPS[precision] * unit).all()
            _check_cache(dict(cc, pos=positions), r, None, kco, None, vco, knew, vnew, touched)
        _check_untouched(cc, kco, vco, touched)

    args = (nh, nkv, hd, slots, c["kc"], c["vc"], c["rope_base"])
    kw = dict(qn=c["qn"], kn=c["kn"], layer=1, precision=precision)
    q, kco, vco = ops.qk_rope_cache(*args, row_pos=pos, qkv=c["qkv"], **kw)
    check(q, kco, vco, c, pos)
    q, kco, vco = ops.qk_rope_cache(*args, fixed_pos=7, qkv=c["qkv"], **kw)
    check(q, kco, vco, c, [7] * R)
    for kp, with_bias in ((1, False), (2, True), (8, True)):
        slab, bias, qkv = ar.slab_form(c, kp, with_bias)
        a = ops.qk_rope_cache(*args, row_pos=pos, qkv=qkv, **kw)
        b = ops.qk_rope_cache(*args, row_pos=pos, slab=slab, bias=bias, **kw)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
        check(*b, dict(c, qkv=qkv), pos)


@pytest.mark.parametrize("kernel, precision", [("flash", "bf16"), ("split", "bf16"), ("split", "fp32")])
@pytest.mark.parametrize("family", ["diffuse", "peaked", "rising"])
def test_prompt_chunks(kernel, precision, family):
    """A prompt chunk of one slot (ragged 16-row blocks: 1, 15, 16, 17, 37 rows; after prefixes that are no multiple
    of the 32-key tile) in slot 2, layer 1 of a poisoned cache.  peaked: row i's own key carries its weight, so a
    causal mask one short is seen; rising: the running maximum moves in every tile."""
    worst = 0.0
    tol = ar.SLOW_TOL["bf16_flash" if kernel == "flash" else precision]
    for R, pos0 in ar.PROMPT_CHUNKS:
        for nh, nkv, hd in ((4, 1, 128), (6, 2, 128)) + (() if kernel == "flash" else ((5, 1, 64), (2, 2, 32))):
            if kernel == "flash" and nh // nkv > 4:
                continue
            c = ar.make_prompt_case(family, nh, nkv, hd, R, pos0, 160, precision, slot=2, nslots=4, layers=2, layer=1)
            out = ops.prompt_attn_ex(c["q"], nh, nkv, hd, [2] * R, pos0 + np.arange(R), c["kc"], c["vc"], True, layer=1,
                                     precision=precision, kernel=kernel)
            assert np.isfinite(out).all(), (R, pos0, nh, nkv, hd)
            err = ar.rel_err(out, ar.prompt_reference(c))
            assert err <= tol, (R, pos0, nh, nkv, hd, err)
            worst = max(worst, err)
    print(f"\nprompt {kernel} {precision} {family}: worst rel err {worst:.3g} (bound {tol:.3g})")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("family", ["diffuse", "peaked", "rising", "large"])
def test_prompt_many_slots(family, precision):
    """attn_split + attn_combine with one_slot false: every row its own slot and position, the positions
    straddling multiples of the 64-key split (63, 64, 65, 127, 128) and 0."""
    pos = [63, 64, 65, 127, 128, 0]
    slots = [4, 0, 6, 1, 7, 3]
    worst = 0.0
    for nh, nkv, hd in ((4, 1, 128), (6, 2, 64), (1, 1, 32)):
        c = ar.make_case(family, nh, nkv, hd, pos, 160, precision, row_slot=slots, nslots=8, layers=2, layer=1,
                         peak=[62, 64, 63, 127, 64, 0], seed=9)
        q, kc, vc = ar.prompt_from_decode(c)
        out = ops.prompt_attn_ex(q, nh, nkv, hd, slots, pos, kc, vc, False, layer=1, precision=precision, kernel="split")
        assert np.isfinite(out).all()
        share = ar.slow_share(c, out)
        assert share <= 1.0, (nh, nkv, hd, share)
        worst = max(worst, share)
    print(f"\nprompt many-slot {precision} {family}: worst error {worst:.3g} of the bound")


# ---- fast decoder ---------------------------------------------------------------------------------------------------
def _fast(c, kernel, qkv=None):
    return ops.fast_attn(c["qkv"] if qkv is None else qkv, c["nh"], c["nkv"], c["hd"], c["row_slot"], int(c["pos"][0]),
                         c["kc"], c["vc"], c["rope_base"], qn=c["qn"], kn=c["kn"], layer=c["layer"],
                         precision=c["precision"], kernel=kernel)


def _check_fast(c, res, exact, knew, vnew, bound):
    """one fast-decoder launch: finite, inside the fast-path bound (bf16: per element; fp32: 2e-5 of the head's
    max), cache as for the slow kernels.  Returns the worst error as a share of the bound."""
    out, kco, vco = res
    assert np.isfinite(out).all(), (c["family"], c["pos"].tolist())
    if c["precision"] == "bf16":
        share = float((np.abs(out - exact) / bound).max())
    else:
        share = ar.slow_share(c, out)
    assert share <= 1.0, (c["family"], int(c["pos"][0]), share)
    touched = np.zeros(c["kc"].shape, bool)
    for r in range(c["R"]):
        _check_cache(c, r, c["kc"], kco, c["vc"], vco, knew, vnew, touched)
    _check_untouched(c, kco, vco, touched)
    return share


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", ar.FAST_SHAPES)
def test_fast_decoder_forms(shape, precision):
    """fast_attn2 at every codebook position 0..15, fast_attn_fused and the unfused pair there and at 16 and 20 of
    24; one row everywhere, three rows in shuffled slots at 0, 5, 15, 20.  Each form inside the bound of the exact
    reference; how far the forms are from each other is printed (none is claimed equal to another)."""
    worst, same, failed = {}, {}, []
    for cpos, S in [(p, 16) for p in range(16)] + [(16, 24), (20, 24)]:
        for R in (1, 3) if cpos in (0, 5, 15, 20) else (1,):
            for c in ar.fast_cases(shape, precision, cpos, S, R):
                exact, knew, vnew, bound = ar.reference(c, bound=True)
                outs = {}
                for kernel in (("attn2",) if cpos < 16 else ()) + ("fused", "unfused"):
                    res = _fast(c, kernel)
                    outs[kernel] = res[0]
                    try:  # every form is tried: the failure names the forms that are off, not the first one
                        worst[kernel] = max(worst.get(kernel, 0.0), _check_fast(c, res, exact, knew, vnew, bound))
                    except AssertionError as e:
                        failed.append((kernel, c["family"], cpos, R, str(e).splitlines()[0][:60]))
                for a in outs:
                    for b in outs:
                        if a < b:
                            same.setdefault((a, b), []).append(np.array_equal(ar.bits(outs[a]), ar.bits(outs[b])))
    assert not failed, (sorted({f[0] for f in failed}), failed[:6])
    print(f"\nfast {shape} {precision}: worst error as a share of the bound {({k: round(v, 3) for k, v in worst.items()})}; "
          f"cases bit-equal {({k: f'{sum(v)}/{len(v)}' for k, v in same.items()})}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", ar.FAST_SHAPES)
def test_fast_decoder_noq(shape, precision):
    """fast_attn2's K / V-only form at codebook 0: the Q part of the input is NaN and is not read; the output is
    0 + v, the bits of the full form on the same row with a finite Q; k / v are cached as ever."""
    nh, nkv, hd = shape
    for c in ar.fast_cases(shape, precision, 0, 16, R=3):
        exact, knew, vnew, bound = ar.reference(c, bound=True)
        full = _fast(c, "attn2")
        qkv = c["qkv"].copy()
        qkv[:, : nh * hd] = np.nan
        noq = _fast(c, "attn2_noq", qkv=qkv)
        for x, y in zip(full, noq):
            np.testing.assert_array_equal(ar.bits(x), ar.bits(y))
        v = np.repeat(np.float32(0) + c["qkv"][:, (nh + nkv) * hd:].reshape(c["R"], nkv, hd), nh // nkv, axis=1)
        np.testing.assert_array_equal(ar.bits(noq[0]), ar.bits(v))
        _check_fast(c, noq, exact, knew, vnew, bound)


# ---- fused fast attention + wo (fattn_wo_kernel / fattn_wo_pair_kernel), the batch-1 production path ---------------------
import linear_ref as lr  # noqa: E402

FW_SHAPES = [(4, 1, 64), (4, 2, 128), (4, 4, 64)]  # g = 4, 2, 1; K = nh hd = 256, 512, 256
FW_N = 64


def _fw_operands(shape, seed=11):
    """wo [N][K] (unit-variance outputs), its bias, a five-row residual table; bf16-valued"""
    nh, nkv, hd = shape
    rng = np.random.default_rng([seed, nh, nkv, hd])
    K = nh * hd
    return (lr.mk(rng, (FW_N, K), "bf16", K ** -0.5), lr.mk(rng, (FW_N,), "bf16", 0.5), lr.mk(rng, (5, FW_N), "bf16"))


def _fw(c, w, res, **kw):
    return ops.fattn_wo(c["qkv"] if "qkv" not in kw else kw.pop("qkv"), c["nh"], c["nkv"], c["hd"], int(c["row_slot"][0]),
                        int(c["pos"][0]), kw.pop("kc", c["kc"]), kw.pop("vc", c["vc"]), c["rope_base"], w, res, qn=c["qn"],
                        kn=c["kn"], layer=c["layer"], **kw)


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(ar.bits(x), ar.bits(y))


def _check_fw_cache(c, res, positions=None):
    """the caches after a fused launch: as after any fast-decoder attention (row cpos written, the rest untouched)"""
    _, knew, vnew = ar.reference(c)
    touched = np.zeros(c["kc"].shape, bool)
    _check_cache(c, 0, c["kc"], res[1], c["vc"], res[2], knew, vnew, touched)
    _check_untouched(c, res[1], res[2], touched)


@pytest.mark.parametrize("quant", [0, 1, 2])
@pytest.mark.parametrize("shape", FW_SHAPES)
def test_fattn_wo_every_codebook_position(shape, quant):
    """One fused launch at every cpos 0..15 (bf16, int8 and int4 wo; ilp 1 and 0): dispatchable exactly where
    fattn_wo_ok says (int8 / int4 need K % 512 == 0: a status, not a launch), err == 0, the bits of the launches it
    replaces (fast_attn2 + row GEMV on the same device operands), of ops.rowgemv applied to the fast_attn2 hook's
    output (bf16, int8), ilp 0 = ilp 1; bf16: inside the linear bound of the float64 composition with the attention's
    fast-path bound as the error of x; the caches as after any fast attention."""
    nh, nkv, hd = shape
    K = nh * hd
    w, bias, res = _fw_operands(shape)
    bias = bias if quant == 0 else None
    kw = dict(quant=quant, gs=128, bias=bias)
    c0 = ar.fast_cases(shape, "bf16", 3, 16)[0]
    if quant and K % 512:
        assert _fw(c0, w, res, **kw)[3] is False  # not dispatchable: nothing launched, reported
        return
    worst = 0.0
    for cpos in range(16):
        for c in ar.fast_cases(shape, "bf16", cpos, 16):
            f = _fw(c, w, res, gen=1 + cpos, pos0=7, **kw)
            assert f[3] and f[4] == 0 and np.isfinite(f[0]).all(), (c["family"], cpos, f[3], f[4])
            _same(f, _fw(c, w, res, fused=False, **kw))
            _same(f, _fw(c, w, res, ilp=0, gen=1 + cpos, pos0=7, **kw))
            _check_fw_cache(c, f)
            if quant < 2:
                att = _fast(c, "attn2")[0].reshape(1, K)
                y = np.zeros(FW_N, np.float32)
                ops.rowgemv(w, att, y, 0, q8=bool(quant), bias=bias, res=res[:1])
                np.testing.assert_array_equal(ar.bits(f[0]), ar.bits(y))
            if quant == 0:
                exact, _, _, bound = ar.reference(c, bound=True)
                v = lr.v_acc(exact.reshape(1, K), w, dx=bound.reshape(1, K))
                v = lr.v_rnd(lr.v_add(lr.v_rnd(lr.v_add(v, bias), "bf16"), res[0]), "bf16")
                share = float((np.abs(f[0] - v.t[0]) / v.e[0]).max())
                assert share <= 1.0, (c["family"], cpos, share)
                worst = max(worst, share)
    print(f"\nfattn_wo {shape} quant {quant}: worst error {worst:.3g} of the bound (bf16 only)")


@pytest.mark.parametrize("quant", [0, 1, 2])
def test_fattn_wo_forms(quant):
    """The launch forms of the fused kernel at K = 512 (every quant dispatches): the residual row gathered by index;
    the QKV table form with the index at 0, qrows - 1 and out of range both ways (the clamp); the K / V-only form of
    codebook 0 with a NaN Q part; xt pre-filled with words tagged for the neighbouring gens.  Each equals the
    launches it replaces bit for bit and leaves err == 0."""
    shape = (4, 2, 128)
    nh, nkv, hd = shape
    K, ld = nh * hd, (nh + 2 * nkv) * hd
    w, bias, res = _fw_operands(shape)
    kw = dict(quant=quant, gs=128, bias=bias if quant == 0 else None)
    rng = np.random.default_rng(12)
    for cpos in (1, 6, 15):
        for c in ar.fast_cases(shape, "bf16", cpos, 16)[:3]:
            gen, pos0 = 1 + cpos, 123
            tag = lambda g: (pos0 * 41 + g) % 65535 + 1  # noqa: E731  (fm_kernels.h FattnWoArgs)
            plain = _fw(c, w, res, gen=gen, pos0=pos0, **kw)
            for g in (gen - 1, gen + 1):  # stale words of the neighbouring launches: never taken for fresh ones
                if 1 <= g <= 40:
                    xt = ((rng.integers(0, 1 << 16, 2 * K).astype(np.uint32) << 16) | np.uint32(tag(g))).astype(np.uint32)
                    f = _fw(c, w, res, gen=gen, pos0=pos0, xt_init=xt, **kw)
                    assert f[3] and f[4] == 0
                    _same(f, plain)
            idx = np.array([9, 3, 2], np.int32)
            f = _fw(c, w, res, idx=idx, idx_col=1, gen=gen, pos0=pos0, **kw)  # residual row 3
            assert f[3] and f[4] == 0
            _same(f, _fw(c, w, res[3:4], gen=gen, pos0=pos0, **kw))
            _same(f, _fw(c, w, res, idx=idx, idx_col=1, fused=False, **kw))
            qtab = ar.rb("bf16")(rng.standard_normal((5, ld))).astype(np.float32)
            for iv, row in ((0, 0), (4, 4), (7, 4), (-3, 0)):
                qtab[row] = c["qkv"][0]  # the row the index selects is the case's own row, the others are noise
                ix = np.array([iv], np.int32)
                f = _fw(c, w, res, qkv=np.full((1, ld), np.nan, np.float32), qtab=qtab, idx=ix, gen=gen, pos0=pos0, **kw)
                assert f[3] and f[4] == 0 and np.isfinite(f[0]).all(), (iv, f[3], f[4])
                _same(f, _fw(c, w, res[row:row + 1], gen=gen, pos0=pos0, **kw))
                qtab[row] = ar.rb("bf16")(rng.standard_normal(ld))
    for c in ar.fast_cases(shape, "bf16", 0, 16):
        qkv = c["qkv"].copy()
        qkv[:, : nh * hd] = np.nan
        f = _fw(c, w, res, qkv=qkv, kv0=True, gen=1, **kw)
        assert f[3] and f[4] == 0 and np.isfinite(f[0]).all()
        _same(f, _fw(c, w, res, gen=1, **kw))  # the full form on a finite Q
        _same(f, _fw(c, w, res, qkv=qkv, kv0=True, fused=False, **kw))
        _check_fw_cache(c, f)


@pytest.mark.parametrize("shape", FW_SHAPES)
def test_fattn_wo_pair_forms(shape):
    """Codebook positions 0 and 1 in one launch (bf16): pair 1 (both rows through wo) and pair 2 (the last layer: row 0
    ends at its K / V write) against two one-row launches, the K / V-only form at 0 and the plain (or table) form at
    1 on the cache the first left; row 0's Q part is NaN."""
    nh, nkv, hd = shape
    ld = (nh + 2 * nkv) * hd
    w, bias, res = _fw_operands(shape)
    rng = np.random.default_rng(13)
    for c in ar.fast_cases(shape, "bf16", 0, 16):
        row1 = ar.rb("bf16")(rng.standard_normal((1, ld))).astype(np.float32)
        row0 = c["qkv"].copy()
        row0[:, : nh * hd] = np.nan
        res0 = res[4]
        a = _fw(c, w, res0[None, :], qkv=row0, kv0=True, gen=1, pos0=5, bias=bias)
        c1 = dict(c, pos=np.array([1], np.int32))
        b = _fw(c1, w, res, qkv=row1, kc=a[1], vc=a[2], gen=3, pos0=5, bias=bias)
        assert a[3] and b[3] and a[4] == 0 and b[4] == 0
        both = np.concatenate([row0, row1])
        p1 = _fw(c1, w, res, qkv=both, pair=1, res0=res0, gen=3, pos0=5, bias=bias)
        assert p1[3] and p1[4] == 0
        np.testing.assert_array_equal(ar.bits(p1[0]), ar.bits(np.stack([a[0], b[0]])))
        np.testing.assert_array_equal(ar.bits(p1[1]), ar.bits(b[1]))
        np.testing.assert_array_equal(ar.bits(p1[2]), ar.bits(b[2]))
        p2 = _fw(c1, w, res, qkv=both, pair=2, gen=3, pos0=5, bias=bias)
        assert p2[3] and p2[4] == 0
        _same(p2, b)
        # the table form of pair 1: row 1's q|k|v row and its residual row by the same index
        qtab = ar.rb("bf16")(rng.standard_normal((5, ld))).astype(np.float32)
        qtab[2] = row1[0]
        ix = np.array([2], np.int32)
        bt = _fw(c1, w, res, qkv=row1, kc=a[1], vc=a[2], idx=ix, gen=3, pos0=5, bias=bias)
        pt = _fw(c1, w, res, qkv=np.concatenate([row0, np.full((1, ld), np.nan, np.float32)]), qtab=qtab, idx=ix, pair=1,
                 res0=res0, gen=3, pos0=5, bias=bias)
        assert pt[3] and pt[4] == 0
        np.testing.assert_array_equal(ar.bits(pt[0]), ar.bits(np.stack([a[0], bt[0]])))
        np.testing.assert_array_equal(ar.bits(pt[1]), ar.bits(bt[1]))
