"""GPU, per op: the batched streamed decode's segment attention and K/V state refresh
(fm_op_codec_window_attn_seg: launch_window_attn_seg, then launch_kv_roll_seg) against the
single-stream kernel run once per segment.

fm_op_codec_window_attn is held to the float64 reference in test_gpu_codec_ops.py; the segment form
assigns the same scores to the same lanes and sums in the same order, so the bound here is
bit-for-bit equality with it.  The refreshed state is pure data movement: numpy gives it exactly.
"""
import json

import numpy as np
import pytest

from codec_ref import SENT
from linear_ref import mk

pytestmark = pytest.mark.gpu

WINDOW, GAP = 128, 3
CASES = [(1, 0), (5, 127), (130, 40)]  # (T, npre): shorter than the state, a full window carried, T > window


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_window_attn_seg_equals_per_segment_kernel(prec, golden):
    from fishmi import ops
    from fishmi.config import CodecConfig

    cfg = CodecConfig.from_spec(json.loads(str(golden("codec_full.npz")["spec"])))
    H, hd, W1 = cfg.t_heads, cfg.t_head_dim, WINDOW - 1
    ld3, n = 3 * H * hd, len(CASES)
    T, npre = [c[0] for c in CASES], [c[1] for c in CASES]
    span = sum(T) + GAP * (n - 1)
    rng = np.random.default_rng([H, hd, 7])
    # every row random, the gap rows and the state rows in front of the last npre included: the
    # segment kernel must not read them
    qkv = mk(rng, (span, ld3), prec)
    old = mk(rng, (n, W1, ld3), prec)
    state = np.full((n, W1 + 2, ld3), SENT, np.float32)
    state[:, :W1] = old
    out = np.full((span + 2, H * hd), SENT, np.float32)
    ops.codec_window_attn_seg(qkv, T, npre, GAP, H, hd, WINDOW, state, out, precision=prec)
    assert (out[span:] == SENT).all() and (state[:, W1:] == SENT).all(), "sentinel overwritten"
    off = 0
    for i in range(n):
        fresh = qkv[off:off + T[i]]
        ref = np.full((T[i] + 1, H * hd), SENT, np.float32)
        single = np.ascontiguousarray(np.concatenate([old[i, W1 - npre[i]:], fresh]))
        ops.codec_window_attn(single, T[i], H, hd, WINDOW, ref, npre=npre[i], precision=prec)
        np.testing.assert_array_equal(out[off:off + T[i]], ref[:T[i]], err_msg=f"segment {i} {prec}")
        np.testing.assert_array_equal(state[i, :W1], np.concatenate([old[i], fresh])[-W1:], err_msg=f"state {i} {prec}")
        if i + 1 < n:
            assert (out[off + T[i]:off + T[i] + GAP] == 0).all(), "gap rows are stored as zeros"
        off += T[i] + GAP


def test_window_attn_seg_refuses_bad_shapes():
    from fishmi import ops
    from fishmi.native import FishMIError

    H, hd = 2, 32
    q = np.zeros((5, 3 * H * hd), np.float32)
    for T, npre, rows in (([5], [128], 127), ([5], [0], 126), ([0, 2], [0, 0], 127)):
        n = len(T)
        qkv = q if n == 1 else np.zeros((2 + GAP, 3 * H * hd), np.float32)
        state = np.full((n, rows, 3 * H * hd), SENT, np.float32)
        out = np.full((8, H * hd), SENT, np.float32)
        with pytest.raises(FishMIError):
            ops.codec_window_attn_seg(qkv, T, npre, GAP, H, hd, WINDOW, state, out)
        assert (out == SENT).all() and (state == SENT).all()
