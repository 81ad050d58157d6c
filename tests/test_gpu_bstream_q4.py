"""Batched decode linear (8 < R <= 32 rows, bsacc_kernel) streaming weight-only int4 codes and their group
(scale, zero) words (fm_tune "bstream_q4"), op level through fm_op_batched_linear_q4: the int4-code form
must be bit-identical to the bf16-fragment form of the dequantised weights -- same partition, same step
order, and the register expansion bf16(fma(q - 8, scale, zero)) is the stored copy's own arithmetic.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from linear_ref import v_acc, v_rnd, v_swiglu8  # float64 values with per-element bounds (test_gpu_linear_ops.py's docstring)
from test_gpu_bstream_q8 import SHAPES

pytestmark = pytest.mark.gpu

STORE, F32, SLAB, SWIGLU8 = 0, 3, 4, 7

# test_gpu_bstream_q8.py's shapes (every K a multiple of 128) at group sizes 128 and 256 (a 256 group spans two
# (scale, zero) units) wherever K % gs == 0.  None of those geometries refills its ring (the int4 ring, 4 TPI
# tiles deep, holds their blocks' whole runs), so two more: N = 12304 / 20496 at K = 1408 are the
# bsacc_kernel<10, 1, 5> and <10, 1, 6> instantiations, whose code ring (4 tiles) refills for tiles 4 and 5 and
# whose (scale, zero) ring (5 tiles) wraps at tile 5; their waves start at steps 0, 5, 11, 16, 22, 27, 33, 38:
# every offset into a 128-k unit, runs of 5 and 6 steps over 2 and 3 units.
CASES = [(N, K, R, epi, gs) for (N, K, R, epi) in SHAPES for gs in (128, 256) if K % gs == 0]
CASES += [(12304, 1408, 16, STORE, 128), (20496, 1408, 9, F32, 128)]


def _bf16(a):
    """fp32 array rounded to bf16 (round to nearest even), still held as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _sum_parts(parts):
    """raw fp32 K-part slabs summed in part order in fp32, as finalize_norm does (test_gpu_linear_ops.py)"""
    acc = parts[0].astype(np.float32)
    for q in range(1, len(parts)):
        acc = acc + parts[q].astype(np.float32)
    return acc.astype(np.float64)


@pytest.mark.parametrize("N,K,R,epi,gs", CASES)
def test_int4_codes_bit_identical_to_bf16_fragments(N, K, R, epi, gs):
    """y from the streamed int4 codes == y from the bf16 fragments of the dequantised weights, every bit, every
    shape and group size; the split-K shapes really split; the codes use all 16 values (a sign or nibble-order
    error cannot hide); the dequantised weights the hook returns are bf16(fma(q - 8, s, z)) of the codes and
    groups it returns, restated in float64 and rounded once to fp32, then to bf16 (s and z are bf16 values within
    2^20 of each other here and q - 8 has 4 bits, so the float64 product and sum are exact and the restatement
    rounds exactly as the device's fp32 fma then bf16 conversion: no double rounding can differ).  Against both
    forms being wrong together, y_bf16 is held to float64 x . wd^T element by element with linear_ref's bounds
    as test_gpu_linear_ops.py holds the bf16 bsacc instantiations: STORE / F32 to round(acc), the sum of the
    raw slabs to acc within the fp32 accumulation bound, SwiGLU8 to round(silu(round(g))) * round(u)."""
    from fishmi import ops
    from fishmi.synth import round_bf16

    rng = np.random.default_rng(1000 * epi + R + gs)
    w = _bf16(rng.standard_normal((N, K)).astype(np.float32) * 0.05)
    x = _bf16(rng.standard_normal((R, K)).astype(np.float32))
    y_q4, y_bf16, kparts, q, sc, zr, wd = ops.batched_linear_q4(w, x, epi, gs=gs)
    print(f"N={N} K={K} R={R} epi={epi} gs={gs}: kparts {kparts}, max|y_q4 - y_bf16| "
          f"{float(np.max(np.abs(y_q4.astype(np.float64) - y_bf16))):.3g}, max|y| {float(np.max(np.abs(y_bf16))):.3g}")
    assert set(np.unique(q).tolist()) == set(range(16))
    assert np.isfinite(y_bf16).all() and np.any(y_bf16 != 0)
    assert np.isfinite(y_q4).all() and np.any(y_q4 != 0)
    assert np.array_equal(y_q4, y_bf16)
    s64 = np.repeat(sc.astype(np.float64), gs, axis=1)
    z64 = np.repeat(zr.astype(np.float64), gs, axis=1)
    assert float(np.max(np.abs(z64) / np.abs(s64))) < 2.0 ** 20 and np.all(s64 != 0)
    restated = round_bf16(((q.astype(np.float64) - 8.0) * s64 + z64).astype(np.float32))
    assert np.array_equal(restated.view(np.uint32), wd.view(np.uint32))
    a = v_acc(x, wd)
    if epi == SLAB:
        assert kparts > 1 and y_q4.shape == (kparts, R, N)
        assert all(np.any(y_bf16[p] != 0) for p in range(kparts))
        got, v = _sum_parts(y_bf16), a
    elif epi == SWIGLU8:
        assert y_q4.shape == (R, N // 2)
        got, v = y_bf16.astype(np.float64), v_swiglu8(a, "bf16")
    else:
        assert y_q4.shape == (R, N)
        got, v = y_bf16.astype(np.float64), v_rnd(a, "bf16")
    err = np.abs(got - v.t)
    print(f"  max |got - ref| / bound {float((err / (v.e + 1e-300)).max()):.3g}, "
          f"{float((got == v.r).mean()) * 100:.2f}% bit-equal to the restatement")
    assert (err <= v.e).all(), float((err / (v.e + 1e-300)).max())


def test_int4_batched_linear_refuses_small_groups():
    """groups below one 128-k unit have no int4-code form: FM_ERR_ARG, not a silent bf16 run"""
    from fishmi import ops
    from fishmi.native import FishMIError

    rng = np.random.default_rng(3)
    w = _bf16(rng.standard_normal((256, 256)).astype(np.float32) * 0.05)
    x = _bf16(rng.standard_normal((9, 256)).astype(np.float32))
    with pytest.raises(FishMIError):
        ops.batched_linear_q4(w, x, STORE, gs=64)
