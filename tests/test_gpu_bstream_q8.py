"""Batched decode linear (8 < R <= 32 rows, bsacc_kernel) streaming weight-only int8 codes (fm_tune
"bstream_q8"), op level through fm_op_batched_linear_q8: the int8-code form must be bit-identical to
the bf16-fragment form of the same codes -- same partition, same step order, int8 -> bf16 exact.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

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
    K <= 9728 is far below that."""
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
    elif epi == SWIGLU8:
        assert y_q8.shape == (R, N // 2)
    else:
        ref = (x.astype(np.float64) @ q.astype(np.float64).T) * scale.astype(np.float64)[None, :]
        err = float(np.max(np.abs(y_bf16 - ref)))
        print(f"  max|y_bf16 - ref| {err:.3g} vs bound {2.0 ** -7 * float(np.max(np.abs(ref))):.3g}")
        assert err <= 2.0 ** -7 * float(np.max(np.abs(ref)))
