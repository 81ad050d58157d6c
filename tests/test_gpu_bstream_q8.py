"""Batched decode linear (8 < R <= 32 rows, bsacc_kernel) streaming weight-only int8 codes (fm_tune
"bstream_q8"), op level through fm_op_batched_linear_q8: the int8-code form must be bit-identical to
the bf16-fragment form of the same codes -- same partition, same step order, int8 -> bf16 exact.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from linear_ref import v_acc, v_q8, v_swiglu8  # float64 values with per-element bounds (test_gpu_linear_ops.py's docstring)

pytestmark = pytest.mark.gpu

STORE, F32, SLAB, SWIGLU8 = 0, 3, 4, 7

SHAPES = [
    (256, 128, 9, STORE),      # smallest: 4 waves, one step each, R just over the GEMV limit
    (200, 256, 12, F32),       # N not a multiple of 16: the tail tile and the scalar epilogue
    (6144, 2560, 12, STORE),   # wqkv geometry
    (2560, 4096, 17, SLAB),    # wo: 8 K parts, 2 steps per wave, R straddling the 16-column group
    (2560, 9728, 32, SLAB),    # w2: per-wave step ranges of 4-5 steps starting at odd steps
    (4096, 2560, 32, SWIGLU8), # 10 steps per wave, interleaved gate / up rows, scales of both halves
]


def _bf16(a):
    """fp32 array rounded to bf16 (round to nearest even), still held as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("N,K,R,epi", SHAPES)
def test_int8_codes_bit_identical_to_bf16_fragments(N, K, R, epi):
    """y from the streamed int8 codes == y from their bf16 fragment copy, every bit, every shape; the
    split-K shapes really split; and (against both forms being wrong together) the STORE / F32 outputs
    are within 2^-7 of max|ref| of the float64 restatement (x . q) * scale: the two bf16 roundings of
    round(round(acc) * scale) are at most half an ulp, 2^-8 relative, each; fp32 accumulation over
    K <= 9728 is far below that.  The SLAB and SWIGLU8 shapes are held to float64 too, element by element
    (linear_ref.py; derivation in test_gpu_linear_ops.py): the sum of the raw K-part slabs to x . q^T within
    the fp32 accumulation bound 2 K 2^-24 (|x| . |q|) alone (no scale yet: finalize_norm applies it), the
    SwiGLU outputs to round(silu(round(g))) * round(u) over g, u = round(round(acc) * scale) with every bf16
    rounding propagated.  Measured on MI355X: slab sums at 1.3e-5 and 4.4e-6 of their bound, SwiGLU at 0.29
    of its bound with 99.98 % of the elements bit-equal to the restatement."""
    from fishmi import ops

    rng = np.random.default_rng(1000 * epi + R)
    w = _bf16(rng.standard_normal((N, K)).astype(np.float32) * 0.05)
    x = _bf16(rng.standard_normal((R, K)).astype(np.float32))
    y_q8, y_bf16, kparts, q, scale = ops.batched_linear_q8(w, x, epi)
    print(f"N={N} K={K} R={R} epi={epi}: kparts {kparts}, max|y_q8 - y_bf16| "
          f"{float(np.max(np.abs(y_q8.astype(np.float64) - y_bf16))):.3g}, max|y| {float(np.max(np.abs(y_bf16))):.3g}")
    assert np.isfinite(y_bf16).all() and np.any(y_bf16 != 0)
    assert np.array_equal(y_q8, y_bf16)
    if epi == SLAB:
        assert kparts > 1 and y_q8.shape == (kparts, R, N)
        # (against both forms being wrong together) the raw slabs carry no rounding and no scale -- finalize_norm
        # applies it later: their sum is x . q^T within the fp32 accumulation bound alone, element by element
        v = v_acc(x, q)
        err = np.abs(y_bf16.astype(np.float64).sum(0) - v.t)
        print(f"  slab sum: max |got - x.q| / bound {float((err / v.e).max()):.3g}")
        assert (err <= v.e).all(), float((err / v.e).max())
    elif epi == SWIGLU8:
        assert y_q8.shape == (R, N // 2)
        # round(silu(round(g))) * round(u) over g, u = round(round(acc) * scale) of each tile's 8 gate / 8 up rows
        v = v_swiglu8(v_q8(v_acc(x, q), scale.astype(np.float64)[None, :], "bf16"), "bf16")
        err = np.abs(y_bf16.astype(np.float64) - v.t)
        print(f"  swiglu8: max |got - ref| / bound {float((err / v.e).max()):.3g}, "
              f"{float((y_bf16 == v.r).mean()) * 100:.2f}% bit-equal to the restatement")
        assert (err <= v.e).all(), float((err / v.e).max())
    else:
        ref = (x.astype(np.float64) @ q.astype(np.float64).T) * scale.astype(np.float64)[None, :]
        err = float(np.max(np.abs(y_bf16 - ref)))
        print(f"  max|y_bf16 - ref| {err:.3g} vs bound {2.0 ** -7 * float(np.max(np.abs(ref))):.3g}")
        assert err <= 2.0 ** -7 * float(np.max(np.abs(ref)))
