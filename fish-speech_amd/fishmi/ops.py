"""Per-op parity hooks of libfishmi (include/fishmi.h, fm_op_*): one production kernel of the decode
path on caller operands, used by tests/test_gpu_ops.py against the reference's per-op goldens.

Reference semantics pinned (file:line in PoTaTo-Mika/fish-speech):
  rmsnorm   RMSNorm.forward            llama.py:989-1000   (fp32 normalise, round, * weight, round)
  qk_rope   nn.RMSNorm(head_dim) +     llama.py:861-863, 900-902 (one rounding incl. the weight)
            apply_rotary_emb           llama.py:1025-1037 (bf16 cos/sin table, fp32 rotate, round)
  embed     forward_generate embedding llama.py:399-420
  rope_table precompute_freqs_cis      llama.py:1003-1022
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native

MODES = {"prologue_norm": 0, "prologue_prenorm": 1, "row_kernel": 2}


def _prec(precision: str) -> int:
    return native.FM_PREC_BF16 if precision == "bf16" else native.FM_PREC_FP32


def rmsnorm(x, w, eps, precision="bf16", mode="prologue_prenorm", device=0):
    x = np.ascontiguousarray(x, np.float32)
    R, d = x.reshape(-1, x.shape[-1]).shape
    w = np.ascontiguousarray(w, np.float32)
    y = np.zeros((R, d), np.float32)
    native.check(native.lib().fm_op_rmsnorm(device, _prec(precision), MODES[mode], native.f32p(x),
                                            native.f32p(w), R, d, float(eps), native.f32p(y)))
    return y.reshape(x.shape)


def qk_rope(qkv_row, nh, nkv, hd, pos, rope_base, qn=None, kn=None, eps=1e-6, precision="bf16",
            kernel="slow", device=0):
    """q (nh, hd) and k (nkv, hd) after qk-norm (if weights given) and RoPE at `pos`, as computed
    inside a decode attention kernel: "fd" attn_fd (the slow model's production kernel), "slow"
    attn_decode2, "slow3" attn_dec3, "fast" fast_attn2."""
    raw = np.ascontiguousarray(qkv_row, np.float32).reshape(-1)
    assert raw.size == (nh + 2 * nkv) * hd
    qk = qn is not None
    qn_ = np.ascontiguousarray(qn if qk else np.ones(hd), np.float32)
    kn_ = np.ascontiguousarray(kn if qk else np.ones(hd), np.float32)
    q = np.zeros(nh * hd, np.float32)
    k = np.zeros(nkv * hd, np.float32)
    kid = {"slow": 0, "fast": 1, "slow3": 2, "fd": 3}[kernel]  # attn_decode2 / fast_attn2 / attn_dec3 / attn_fd
    native.check(native.lib().fm_op_qk_rope(device, _prec(precision), kid,
                                            native.f32p(raw), nh, nkv, hd, native.f32p(qn_), native.f32p(kn_),
                                            int(qk), float(eps), float(rope_base), int(pos), native.f32p(q),
                                            native.f32p(k)))
    return q.reshape(nh, hd), k.reshape(nkv, hd)


ATTN_KERNELS = {"slow": 0, "slow3": 2, "fd": 3}  # attn_decode2 / attn_dec3 / attn_fd


def decode_attn(qkv, nh, nkv, hd, pos, kcache, vcache, rope_base, qn=None, kn=None, eps=1e-6,
                precision="bf16", kernel="fd", min_split=32, device=0):
    """The slow decode attention (llama.py:883-945) on R rows: qkv (R, (nh+2nkv)*hd) raw projections,
    pos (R,), kcache / vcache (R, nkv, S, hd) holding rows < pos[r].  Returns (out (R, nh, hd),
    kcache, vcache after the kernel's write of row pos[r])."""
    raw = np.ascontiguousarray(qkv, np.float32)
    R = raw.shape[0]
    assert raw.shape[1] == (nh + 2 * nkv) * hd
    kc = np.ascontiguousarray(kcache, np.float32)
    vc = np.ascontiguousarray(vcache, np.float32)
    S = kc.shape[2]
    assert kc.shape == (R, nkv, S, hd) and vc.shape == kc.shape
    p = np.ascontiguousarray(pos, np.int32)
    qk = qn is not None
    qn_ = np.ascontiguousarray(qn if qk else np.ones(hd), np.float32)
    kn_ = np.ascontiguousarray(kn if qk else np.ones(hd), np.float32)
    out = np.zeros((R, nh, hd), np.float32)
    kco = np.zeros_like(kc)
    vco = np.zeros_like(vc)
    native.check(native.lib().fm_op_decode_attn(device, _prec(precision), ATTN_KERNELS[kernel], native.f32p(raw), R,
                                                nh, nkv, hd, native.f32p(qn_), native.f32p(kn_), int(qk), float(eps),
                                                float(rope_base), native.i32p(p), native.f32p(kc), native.f32p(vc), S,
                                                int(min_split), native.f32p(out), native.f32p(kco), native.f32p(vco)))
    return out, kco, vco


def prompt_attn(q, nh, nkv, hd, pos0, kcache, vcache, precision="bf16", kernel="flash", device=0):
    """Causal attention of R prompt rows (positions pos0 .. pos0+R-1, one slot) over caches
    kcache / vcache (nkv, S, hd): q (R, nh*hd).  kernel "flash" (attn_prefill_kernel) or "split"."""
    qq = np.ascontiguousarray(q, np.float32)
    R = qq.shape[0]
    kc = np.ascontiguousarray(kcache, np.float32)
    vc = np.ascontiguousarray(vcache, np.float32)
    S = kc.shape[1]
    assert qq.shape[1] == nh * hd and kc.shape == (nkv, S, hd) and vc.shape == kc.shape
    out = np.zeros((R, nh, hd), np.float32)
    native.check(native.lib().fm_op_prompt_attn(device, _prec(precision), {"split": 0, "flash": 1}[kernel],
                                                native.f32p(qq), R, nh, nkv, hd, int(pos0), native.f32p(kc),
                                                native.f32p(vc), S, native.f32p(out)))
    return out


# ---- attention hooks on the model's cache layout [nslots][layers][nkv][S][hd] (tests/test_gpu_attn_ops.py) ----
def _norm_w(qn, kn, hd):
    qk = qn is not None
    return (int(qk), np.ascontiguousarray(qn if qk else np.ones(hd), np.float32),
            np.ascontiguousarray(kn if qk else np.ones(hd), np.float32))


def _caches(kcache, vcache, nkv, hd):
    kc = np.array(kcache, np.float32, order="C")  # copies: the hooks write them in place
    vc = np.array(vcache, np.float32, order="C")
    assert kc.ndim == 5 and kc.shape[2] == nkv and kc.shape[4] == hd and vc.shape == kc.shape, kc.shape
    return kc, vc


def _opt(a):
    return None if a is None else native.f32p(a)


def _raw_or_slab(qkv, slab, bias, ld):
    """(raw, slab, kp, bias, R) as contiguous fp32 arrays (None where not given)."""
    assert (qkv is None) != (slab is None)
    raw = None if qkv is None else np.ascontiguousarray(qkv, np.float32)
    sl = None if slab is None else np.ascontiguousarray(slab, np.float32)
    bi = None if bias is None else np.ascontiguousarray(bias, np.float32).reshape(ld)
    if raw is not None:
        assert raw.ndim == 2 and raw.shape[1] == ld
        return raw, None, 1, None, raw.shape[0]
    assert sl.ndim == 3 and sl.shape[2] == ld
    return None, sl, sl.shape[0], bi, sl.shape[1]


def decode_attn_ex(nh, nkv, hd, row_slot, pos, kcache, vcache, rope_base, qkv=None, slab=None, bias=None, qn=None,
                   kn=None, eps=1e-6, layer=0, precision="bf16", kernel="fd", cap=32, nwb=4, frame=False, reps=1,
                   device=0):
    """fm_op_decode_attn_ex: the slow decode attention on rows in slots row_slot of caches (nslots, layers, nkv, S, hd),
    from qkv (R, ld) or slab (kp, R, ld) + bias.  frame=True: kernel / nwb / cap as a frame of R rows launches them.
    Returns (out (R, nh, hd), kcache, vcache, info) with info = dict(kernel, nwb, cap, splits, tickets, guard_ok,
    fd_nsp, cap2)."""
    ld = (nh + 2 * nkv) * hd
    raw, sl, kp, bi, R = _raw_or_slab(qkv, slab, bias, ld)
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    rs = np.ascontiguousarray(row_slot, np.int32)
    p = np.ascontiguousarray(pos, np.int32)
    assert rs.shape == (R,) and p.shape == (R,)
    qk, qn_, kn_ = _norm_w(qn, kn, hd)
    out = np.zeros((R, nh, hd), np.float32)
    info = np.zeros(8, np.int32)
    native.check(native.lib().fm_op_decode_attn_ex(
        device, _prec(precision), ATTN_KERNELS[kernel], _opt(raw), _opt(sl), kp, _opt(bi), R, nh, nkv, hd,
        native.f32p(qn_), native.f32p(kn_), qk, float(eps), float(rope_base), native.i32p(rs), native.i32p(p), nslots,
        layers, int(layer), native.f32p(kc), native.f32p(vc), S, int(cap), int(nwb), int(frame), int(reps),
        native.f32p(out), native.i32p(info)))
    names = ("kernel", "nwb", "cap", "splits", "tickets", "guard_ok", "fd_nsp", "cap2")
    d = dict(zip(names, (int(v) for v in info)))
    d["kernel"] = {v: k for k, v in ATTN_KERNELS.items()}[d["kernel"]]
    return out, kc, vc, d


def prompt_attn_ex(q, nh, nkv, hd, row_slot, row_pos, kcache, vcache, one_slot, layer=0, precision="bf16",
                   kernel="split", device=0):
    """fm_op_prompt_attn_ex: prompt rows q (R, nh*hd) with their own (slot, position) over caches (nslots, layers,
    nkv, S, hd); one_slot=False is the many-slot split + combine route."""
    qq = np.ascontiguousarray(q, np.float32)
    R = qq.shape[0]
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    rs = np.ascontiguousarray(row_slot, np.int32)
    rp = np.ascontiguousarray(row_pos, np.int32)
    assert qq.shape == (R, nh * hd) and rs.shape == (R,) and rp.shape == (R,)
    out = np.zeros((R, nh, hd), np.float32)
    native.check(native.lib().fm_op_prompt_attn_ex(
        device, _prec(precision), {"split": 0, "flash": 1}[kernel], native.f32p(qq), R, nh, nkv, hd, native.i32p(rs),
        native.i32p(rp), int(one_slot), nslots, layers, int(layer), native.f32p(kc), native.f32p(vc), S,
        native.f32p(out)))
    return out


def qk_rope_cache(nh, nkv, hd, row_slot, kcache, vcache, rope_base, row_pos=None, fixed_pos=-1, qkv=None, slab=None,
                  bias=None, qn=None, kn=None, eps=1e-6, layer=0, precision="bf16", device=0):
    """fm_op_qk_rope_cache: the prefill's QK-norm + RoPE + cache write.  Returns (q (R, nh, hd), kcache, vcache)."""
    ld = (nh + 2 * nkv) * hd
    raw, sl, kp, bi, R = _raw_or_slab(qkv, slab, bias, ld)
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    rs = np.ascontiguousarray(row_slot, np.int32)
    rp = np.ascontiguousarray(row_pos if row_pos is not None else np.zeros(R), np.int32)
    assert rs.shape == (R,) and rp.shape == (R,) and (fixed_pos >= 0 or row_pos is not None)
    qk, qn_, kn_ = _norm_w(qn, kn, hd)
    q = np.zeros((R, nh, hd), np.float32)
    native.check(native.lib().fm_op_qk_rope_cache(
        device, _prec(precision), _opt(raw), _opt(sl), kp, _opt(bi), R, nh, nkv, hd, native.f32p(qn_), native.f32p(kn_),
        qk, float(eps), float(rope_base), native.i32p(rs), native.i32p(rp), int(fixed_pos), nslots, layers, int(layer),
        native.f32p(kc), native.f32p(vc), S, native.f32p(q)))
    return q, kc, vc


FAST_ATTN_KERNELS = {"attn2": 0, "attn2_noq": 1, "fused": 2, "unfused": 3}


def fast_attn(qkv, nh, nkv, hd, row_slot, cpos, kcache, vcache, rope_base, qn=None, kn=None, eps=1e-6, layer=0,
              precision="bf16", kernel="attn2", device=0):
    """fm_op_fast_attn: the fast decoder's attention at codebook position cpos on rows in slots row_slot of caches
    (nslots, layers, nkv, S = num_codebooks, hd).  kernel: "attn2" fast_attn2_kernel, "attn2_noq" its K/V-only form
    (cpos 0), "fused" fast_attn_fused_kernel, "unfused" qk_rope_cache(fixed_pos) + fast_attn_kernel.
    Returns (out (R, nh, hd), kcache, vcache)."""
    raw = np.ascontiguousarray(qkv, np.float32)
    R = raw.shape[0]
    assert raw.shape == (R, (nh + 2 * nkv) * hd)
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    rs = np.ascontiguousarray(row_slot, np.int32)
    assert rs.shape == (R,)
    qk, qn_, kn_ = _norm_w(qn, kn, hd)
    out = np.zeros((R, nh, hd), np.float32)
    native.check(native.lib().fm_op_fast_attn(
        device, _prec(precision), FAST_ATTN_KERNELS[kernel], native.f32p(raw), R, nh, nkv, hd, native.f32p(qn_),
        native.f32p(kn_), qk, float(eps), float(rope_base), native.i32p(rs), int(cpos), nslots, layers, int(layer),
        native.f32p(kc), native.f32p(vc), S, native.f32p(out)))
    return out, kc, vc


def fattn_wo(qkv, nh, nkv, hd, slot, cpos, kcache, vcache, rope_base, w, res, bias=None, qn=None, kn=None, eps=1e-6,
             layer=0, quant=0, gs=128, fused=True, qtab=None, idx=None, idx_col=0, res0=None, kv0=False, pair=0, ilp=1,
             gen=1, pos0=0, xt_init=None, device=0):
    """fm_op_fattn_wo: the batch-1 fast decoder's attention + wo in one launch (fused) or as fast_attn2 + row GEMV.
    qkv (1 or 2, ld); w (N, nh*hd); res (res_rows, ldr) the residual table (row idx[idx_col], or row 0).  Returns
    (y (N,) or (2, N) for pair 1, kcache, vcache, ok, err): ok False = not dispatchable, nothing was launched.  The
    pair forms take quant 1 / 2 (int8 / int4 wo) too.  fattn_wo.last_depth holds the last call's dispatched depth
    (status[0]: rowgemv_u's chunks per wave, 0 when nothing was launched)."""
    raw = np.ascontiguousarray(qkv, np.float32).reshape(-1, (nh + 2 * nkv) * hd)
    assert raw.shape[0] == (2 if pair else 1)
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    ww = np.ascontiguousarray(w, np.float32)
    N = ww.shape[0]
    assert ww.shape == (N, nh * hd)
    rr = np.ascontiguousarray(res, np.float32).reshape(-1, np.shape(res)[-1])
    qt = None if qtab is None else np.ascontiguousarray(qtab, np.float32)
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    bi = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r0 = None if res0 is None else np.ascontiguousarray(res0, np.float32)
    xt = None if xt_init is None else np.ascontiguousarray(xt_init, np.uint32)
    assert xt is None or xt.shape == (2 * nh * hd,)
    qk, qn_, kn_ = _norm_w(qn, kn, hd)
    y = np.zeros((2, N) if pair == 1 else (N,), np.float32)
    status = np.zeros(2, np.int32)
    native.check(native.lib().fm_op_fattn_wo(
        device, int(quant), int(gs), int(fused), native.f32p(raw), _opt(qt), 0 if qt is None else qt.shape[0],
        None if ix is None else native.i32p(ix), 0 if ix is None else ix.size, int(idx_col), nh, nkv, hd,
        native.f32p(qn_), native.f32p(kn_), qk, float(eps), float(rope_base), int(slot), int(cpos), nslots, layers,
        int(layer), native.f32p(kc), native.f32p(vc), S, native.f32p(ww), _opt(bi), native.f32p(rr), rr.shape[0],
        rr.shape[1], _opt(r0), N, int(kv0), int(pair), int(ilp), int(gen), int(pos0),
        None if xt is None else xt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), native.f32p(y), native.i32p(status)))
    fattn_wo.last_depth = int(status[0])  # the dispatched depth (chunks per wave; 0: not dispatchable)
    return y, kc, vc, bool(status[0]), int(status[1])


fattn_wo.last_depth = 0


def slow_attn_wo(qkv, nh, nkv, hd, slots, pos, kcache, vcache, rope_base, w, res, bias=None, qn=None, kn=None, eps=1e-6,
                 layer=0, fused=True, rp=2, gens=None, restore=True, xt_init=None, device=0):
    """fm_op_slow_attn_wo: the batch-1 slow layers' attention + wo at the (slots[i], pos[i]) pairs, one run after the
    other -- one launch each (fused) or attn_fd + row GEMV.  qkv (nrun, ld); w (N, nh*hd); res (N,).  restore: every
    run starts from the given caches (else from what the earlier runs left).  Returns (y (nrun, N), k_rows, v_rows
    (nrun, nkv, hd), ok, err): ok False with fused = not dispatchable, nothing was launched."""
    raw = np.ascontiguousarray(qkv, np.float32).reshape(-1, (nh + 2 * nkv) * hd)
    n = raw.shape[0]
    sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slots, np.int32), (n,)))
    ps = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, np.int32), (n,)))
    ge = np.ascontiguousarray(np.broadcast_to(np.asarray(1 if gens is None else gens, np.int32), (n,)))
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    ww = np.ascontiguousarray(w, np.float32)
    N = ww.shape[0]
    assert ww.shape == (N, nh * hd)
    rr = np.ascontiguousarray(res, np.float32).reshape(N)
    bi = None if bias is None else np.ascontiguousarray(bias, np.float32)
    xt = None if xt_init is None else np.ascontiguousarray(xt_init, np.uint32)
    assert xt is None or xt.shape == (nh * hd,)
    qk, qn_, kn_ = _norm_w(qn, kn, hd)
    y = np.zeros((n, N), np.float32)
    kr = np.zeros((n, nkv, hd), np.float32)
    vr = np.zeros((n, nkv, hd), np.float32)
    status = np.zeros(2, np.int32)
    native.check(native.lib().fm_op_slow_attn_wo(
        device, int(fused), int(rp), native.f32p(raw), nh, nkv, hd, native.f32p(qn_), native.f32p(kn_), qk, float(eps),
        float(rope_base), native.i32p(sl), native.i32p(ps), native.i32p(ge), n, int(restore), nslots, layers, int(layer),
        native.f32p(kc), native.f32p(vc), S, native.f32p(ww), _opt(bi), native.f32p(rr), N,
        None if xt is None else xt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), native.f32p(y), native.f32p(kr),
        native.f32p(vr), native.i32p(status)))
    return y, kr, vr, bool(status[0]), int(status[1])


def slow_attn_wo_q(qkv, nh, nkv, hd, slots, pos, kcache, vcache, rope_base, w, res, quant="int8", gs=128, bias=None,
                   qn=None, kn=None, eps=1e-6, layer=0, fused=True, rp=2, gens=None, restore=True, xt_init=None, device=0):
    """fm_op_slow_attn_wo_q: slow_attn_wo on weight-only codes -- w (N, nh*hd) is quantised on the device ("int8": row
    scales; "int4": groups of gs) and both compositions read the row-major codes.  Returns (y (nrun, N), k_rows, v_rows
    (nrun, nkv, hd), ok, err, q, scale, zero): q (N, K) int8 codes (int4: 0..15), scale (N,) / (N, K/gs), zero (N, K/gs)
    or None; ok False with fused = not dispatchable, nothing was launched (q, scale, zero are then zeros)."""
    raw = np.ascontiguousarray(qkv, np.float32).reshape(-1, (nh + 2 * nkv) * hd)
    n = raw.shape[0]
    sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slots, np.int32), (n,)))
    ps = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, np.int32), (n,)))
    ge = np.ascontiguousarray(np.broadcast_to(np.asarray(1 if gens is None else gens, np.int32), (n,)))
    kc, vc = _caches(kcache, vcache, nkv, hd)
    nslots, layers, _, S, _ = kc.shape
    ww = np.ascontiguousarray(w, np.float32)
    N, K = ww.shape[0], nh * hd
    assert ww.shape == (N, K)
    rr = np.ascontiguousarray(res, np.float32).reshape(N)
    bi = None if bias is None else np.ascontiguousarray(bias, np.float32)
    xt = None if xt_init is None else np.ascontiguousarray(xt_init, np.uint32)
    assert xt is None or xt.shape == (K,)
    qk, qn_, kn_ = _norm_w(qn, kn, hd)
    q4 = quant == "int4"
    assert quant in ("int8", "int4")
    y = np.zeros((n, N), np.float32)
    kr = np.zeros((n, nkv, hd), np.float32)
    vr = np.zeros((n, nkv, hd), np.float32)
    q = np.zeros((N, K), np.int8)
    ng = max(K // gs, 1) if q4 and gs > 0 else 1
    sc = np.zeros((N, ng) if q4 else (N,), np.float32)
    zr = np.zeros((N, ng), np.float32) if q4 else None
    status = np.zeros(2, np.int32)
    native.check(native.lib().fm_op_slow_attn_wo_q(
        device, 2 if q4 else 1, int(gs), int(fused), int(rp), native.f32p(raw), nh, nkv, hd, native.f32p(qn_),
        native.f32p(kn_), qk, float(eps), float(rope_base), native.i32p(sl), native.i32p(ps), native.i32p(ge), n,
        int(restore), nslots, layers, int(layer), native.f32p(kc), native.f32p(vc), S, native.f32p(ww), _opt(bi),
        native.f32p(rr), N, None if xt is None else xt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), native.f32p(y),
        native.f32p(kr), native.f32p(vr), native.i32p(status), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
        native.f32p(sc), None if zr is None else native.f32p(zr)))
    return y, kr, vr, bool(status[0]), int(status[1]), q, sc, zr


def embed(tok, emb, cbemb, num_codebooks, codebook_size, semantic_begin_id, semantic_end_id, scale,
          precision="bf16", device=0):
    """tok: (R, C+1) rows (row r = one position's [text/semantic token, codes...])."""
    t = np.ascontiguousarray(tok, np.int32)
    emb = np.ascontiguousarray(emb, np.float32)
    cbemb = np.ascontiguousarray(cbemb, np.float32)
    R, d = t.shape[0], emb.shape[1]
    x = np.zeros((R, d), np.float32)
    native.check(native.lib().fm_op_embed(device, _prec(precision), native.i32p(t), R, native.f32p(emb),
                                          emb.shape[0], native.f32p(cbemb), d, num_codebooks, codebook_size,
                                          semantic_begin_id, semantic_end_id, int(scale), native.f32p(x)))
    return x


def rope_table(seq_len, head_dim, base):
    out = np.zeros((seq_len, head_dim // 2, 2), np.float32)
    native.check(native.lib().fm_rope_table(seq_len, head_dim, float(base), native.f32p(out)))
    return out


def quant4(w, gs, x=None, device=0):
    """fm_op_quant4: (q [N][K] uint8, scale [N][K/gs], zero [N][K/gs], dequantised w [N][K]) from the
    device int4 quantizer, and with x ([R][K]) the decode GEMV on the dequantised bf16 weights and on
    the streamed 4-bit codes: (..., y_bf16 [R][N], y_q4 [R][N] or None)."""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    q = np.zeros((N, K), np.uint8)
    sc = np.zeros((N, K // gs), np.float32)
    zr = np.zeros((N, K // gs), np.float32)
    wd = np.zeros((N, K), np.float32)
    if x is None:
        native.check(native.lib().fm_op_quant4(device, native.f32p(w), N, K, gs,
                                               q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                               native.f32p(sc), native.f32p(zr), native.f32p(wd), None, 0, None, None))
        return q, sc, zr, wd
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    R = x.shape[0]
    yb = np.zeros((R, N), np.float32)
    y4 = np.zeros((R, N), np.float32) if (gs % 128 == 0 and K % 128 == 0) else None
    native.check(native.lib().fm_op_quant4(device, native.f32p(w), N, K, gs,
                                           q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), native.f32p(sc),
                                           native.f32p(zr), native.f32p(wd), native.f32p(x), R,
                                           native.f32p(y4) if y4 is not None else None, native.f32p(yb)))
    return q, sc, zr, wd, yb, y4


EPI_STORE, EPI_F32, EPI_SLAB, EPI_SWIGLU8 = 0, 3, 4, 7


def batched_linear_q8(w, x, epi, device=0):
    """fm_op_batched_linear_q8: the batched decode linear (8 < R <= 32 rows of x, bf16) on the device-
    quantised int8 form of w [N][K], once streaming the int8 codes and once their bf16 fragment copy.
    Returns (y_q8, y_bf16, kparts, q [N][K] int8, scale [N]); the outputs are [R][N] (EPI_STORE /
    EPI_F32), [R][N/2] (EPI_SWIGLU8) or the raw split-K slabs [kparts][R][N] (EPI_SLAB)."""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    R = x.shape[0]
    No = N // 2 if epi == EPI_SWIGLU8 else N
    cap = 8 if epi == EPI_SLAB else 1  # K parts at most (bsacc_plan)
    yq = np.zeros((cap, R, No), np.float32)
    yb = np.zeros((cap, R, No), np.float32)
    kp = np.zeros(1, np.int32)
    q = np.zeros((N, K), np.int8)
    sc = np.zeros(N, np.float32)
    native.check(native.lib().fm_op_batched_linear_q8(device, native.f32p(w), N, K, native.f32p(x), R, int(epi),
                                                      native.f32p(yq), native.f32p(yb), native.i32p(kp),
                                                      q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
                                                      native.f32p(sc)))
    k = int(kp[0])
    if epi == EPI_SLAB:
        return yq.reshape(-1)[:k * R * No].reshape(k, R, No), yb.reshape(-1)[:k * R * No].reshape(k, R, No), k, q, sc
    return yq[0], yb[0], k, q, sc


# ---- the decode linears (fm_op_linear .. fm_op_prompt_skinny; tests/test_gpu_linear_ops.py) ----------
# Kernel codes (csrc/fm_kernels.h)
EPI_RESID, EPI_SWIGLU, EPI_SLABFIN = 1, 2, 5
PRO_PLAIN, PRO_NORM, PRO_PRENORM = 0, 1, 3
ROW_FIN, ROW_NORM_STORE, ROW_NORM_SWIGLU, ROW_NORM_F32 = 0, 1, 2, 3


def _f(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _p(a):
    return None if a is None else native.f32p(a)


def _out(y):
    """An in/out array: the caller's pre-filled float32 C array itself (the hook writes into it)."""
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.flags.c_contiguous and y.flags.writeable
    return y


def linear(w, x, y, epi=EPI_STORE, w2=None, bias=None, res=None, precision="bf16", split=False, reps=1, device=0):
    """fm_op_linear: launch_linear on x [R][ldx >= K], w [N][K]; y [rows >= R][ldy >= N] is filled in place.
    Returns (ksb, dirty)."""
    w, w2, bias, x, res = _f(w), _f(w2), _f(bias), _f(x), _f(res)
    N, K = w.shape
    R, ldx = x.shape
    y = _out(y)
    ksb, dirty = np.zeros(1, np.int32), np.zeros(1, np.int32)
    native.check(native.lib().fm_op_linear(device, _prec(precision), int(epi), _p(w), _p(w2), _p(bias), _p(x), ldx,
                                           _p(res), 0 if res is None else res.shape[1], R, N, K, int(split), _p(y),
                                           y.shape[1], y.shape[0], int(reps), native.i32p(ksb), native.i32p(dirty)))
    return int(ksb[0]), int(dirty[0])


def linear_q(w, x, y_q, y_bf16, quant, epi=EPI_STORE, gs=128, bias=None, res=None, split=False, reps=1, device=0):
    """fm_op_linear_q: w [N][K] (bf16-valued) quantised on the device (quant "int8": per-channel; "int4": groups of
    gs), then launch_linear on x [R][ldx >= K] once from the packed bf16 fragments of the quantised weights
    (y_bf16) and once from the step-granular codes alone (y_q); both [rows >= R][ldy >= N], filled in place.
    Returns (ksb, dirty, q [N][K] int8 codes, scale, zero): scale [N] and zero None for int8, both [N][K / gs]
    for int4."""
    w, bias, x, res = _f(w), _f(bias), _f(x), _f(res)
    N, K = w.shape
    R, ldx = x.shape
    y_q, y_bf16 = _out(y_q), _out(y_bf16)
    assert y_q.shape == y_bf16.shape
    q4 = quant == "int4"
    ksb, dirty = np.zeros(1, np.int32), np.zeros(1, np.int32)
    q = np.zeros((N, K), np.int8)
    sc = np.zeros((N, K // gs) if q4 else N, np.float32)
    zr = np.zeros((N, K // gs), np.float32) if q4 else None
    native.check(native.lib().fm_op_linear_q(device, native.FM_QUANT_INT4 if q4 else native.FM_QUANT_INT8, int(gs),
                                             _p(w), N, K, _p(bias), _p(x), ldx, _p(res),
                                             0 if res is None else res.shape[1], R, int(epi), int(split), _p(y_q),
                                             _p(y_bf16), y_q.shape[1], y_q.shape[0], int(reps), native.i32p(ksb),
                                             native.i32p(dirty), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
                                             _p(sc), _p(zr)))
    return int(ksb[0]), int(dirty[0]), q, sc, zr


def gemv(w, x, y, pro=PRO_PLAIN, epi=EPI_STORE, ksb=1, R=None, w2=None, bias=None, nw=None, eps=1e-6, idx=None,
         idx_col=0, res=None, ss_gran=0, ss_out=None, precision="bf16", reps=1, device=0):
    """fm_op_gemv: launch_gemv.  x [R][ldx] (pro 1 with idx: the gathered table, R given), idx [R][idx_ld]
    int32 (x rows with pro 1, residual rows with epi 5; the table's row count is the clamp).  y (in/out):
    [rows][ldy]; epi 4: [ksb * R (+ spare)][ldy]; epi 5: the finalised rows, ss_out [N / 16][R] in/out.
    Returns dirty."""
    w, w2, bias, nw, x, res = _f(w), _f(w2), _f(bias), _f(nw), _f(x), _f(res)
    N, K = w.shape
    ldx = x.shape[1]
    idx_ld = idx_rows = 0
    if idx is not None:
        idx = np.ascontiguousarray(idx, np.int32).reshape(len(idx), -1)
        idx_ld = idx.shape[1]
        idx_rows = x.shape[0] if pro == PRO_NORM else res.shape[0]
        R = idx.shape[0]
    elif R is None:
        R = x.shape[0]
    y = _out(y)
    dirty = np.zeros(1, np.int32)
    native.check(native.lib().fm_op_gemv(device, _prec(precision), int(pro), int(epi), int(ksb), _p(w), _p(w2), _p(bias),
                                         _p(nw), float(eps), _p(x), ldx, None if idx is None else native.i32p(idx),
                                         idx_ld, int(idx_col), idx_rows, _p(res), 0 if res is None else res.shape[1],
                                         int(ss_gran), R, N, K, _p(y), y.shape[1], y.shape[0],
                                         None if ss_out is None else _p(_out(ss_out)), int(reps), native.i32p(dirty)))
    return int(dirty[0])


def rowgemv(w, x, y, kind, q8=False, bias=None, nw=None, eps=1e-6, res=None, idx=None, idx_col=0, reps=1, device=0):
    """fm_op_rowgemv: launch_rowgemv on one row.  x [x_rows][ldx] (one row unless gathered through
    idx[idx_col]; kind 0 gathers its residual res [res_rows][ldr] instead); y (in/out) a flat array of at
    least N (kind 2: N / 2) values.  Returns (q [N][K] int8, scale [N]) with q8, else None."""
    w, bias, nw, res = _f(w), _f(bias), _f(nw), _f(res)
    x = _f(x).reshape(-1, np.shape(x)[-1])
    if res is not None:
        res = res.reshape(-1, res.shape[-1])
    N, K = w.shape
    y = _out(y)
    if idx is not None:
        idx = np.ascontiguousarray(idx, np.int32).ravel()
    q = np.zeros((N, K), np.int8) if q8 else None
    sc = np.zeros(N, np.float32) if q8 else None
    native.check(native.lib().fm_op_rowgemv(device, int(kind), int(q8), _p(w), _p(bias), _p(nw), float(eps), _p(x),
                                            x.shape[0], x.shape[1], _p(res), 0 if res is None else res.shape[0],
                                            0 if res is None else res.shape[1],
                                            None if idx is None else native.i32p(idx), 0 if idx is None else idx.size,
                                            int(idx_col), N, K, _p(y), y.size, int(reps),
                                            q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)) if q8 else None, _p(sc)))
    return (q, sc) if q8 else None


def rowgemv_pair(w, x, y, kind, bias=None, nw=None, eps=1e-6, res0=None, res1=None, idx=None, idx_col=0, skip0=0,
                 device=0):
    """fm_op_rowgemv_pair: launch_rowgemv's two-row forms.  x [2][K]; kind 0: res0 [N] (row 0's residual), res1
    [res_rows][ldr] (row 1's, row idx[idx_col] of it); kind 1: skip0 rows of row 0 left out.  y (in/out) [2][ld]."""
    w, bias, nw, x, res0, res1 = _f(w), _f(bias), _f(nw), _f(x), _f(res0), _f(res1)
    N, K = w.shape
    assert x.shape == (2, K)
    if res1 is not None:
        res1 = res1.reshape(-1, res1.shape[-1])
    y = _out(y)
    assert y.ndim == 2 and y.shape[0] == 2
    if idx is not None:
        idx = np.ascontiguousarray(idx, np.int32).ravel()
    native.check(native.lib().fm_op_rowgemv_pair(device, int(kind), _p(w), _p(bias), _p(nw), float(eps), _p(x), _p(res0),
                                                 _p(res1), 0 if res1 is None else res1.shape[0],
                                                 0 if res1 is None else res1.shape[1],
                                                 None if idx is None else native.i32p(idx), 0 if idx is None else idx.size,
                                                 int(idx_col), int(skip0), N, K, _p(y), y.shape[1]))


def rowgemv_pair_q(w, x, y2, y1, kind, quant, gs=128, nw=None, eps=1e-6, res0=None, res1=None, idx=None, idx_col=0,
                   skip0=0, device=0):
    """fm_op_rowgemv_pair_q: the two-row forms on weight-only codes (fm_tune fast_pair_q).  w [N][K] is quantised on
    the device (quant "int8", or "int4" with groups of gs); the two-row launch fills y2 [2][ld], the one-row production
    launcher, once per row on the same device operands, y1 [2][ld] (both in/out).  kind 0 fin, 1 norm + store (skip0),
    2 norm + swiglu; operands as rowgemv_pair.  Returns (q [N][K] int8 codes, scale, zero): scale [N] and zero None
    for int8, both [N][K / gs] for int4."""
    w, nw, x, res0, res1 = _f(w), _f(nw), _f(x), _f(res0), _f(res1)
    N, K = w.shape
    assert x.shape == (2, K)
    if res1 is not None:
        res1 = res1.reshape(-1, res1.shape[-1])
    y2, y1 = _out(y2), _out(y1)
    assert y2.ndim == 2 and y2.shape[0] == 2 and y1.shape == y2.shape
    if idx is not None:
        idx = np.ascontiguousarray(idx, np.int32).ravel()
    q4 = quant == "int4"
    assert q4 or quant == "int8"
    q = np.zeros((N, K), np.int8)
    sc = np.zeros((N, K // gs) if q4 else N, np.float32)
    zr = np.zeros((N, K // gs), np.float32) if q4 else None
    native.check(native.lib().fm_op_rowgemv_pair_q(
        device, native.FM_QUANT_INT4 if q4 else native.FM_QUANT_INT8, int(gs), int(kind), _p(w), _p(nw), float(eps), _p(x),
        _p(res0), _p(res1), 0 if res1 is None else res1.shape[0], 0 if res1 is None else res1.shape[1],
        None if idx is None else native.i32p(idx), 0 if idx is None else idx.size, int(idx_col), int(skip0), N, K, _p(y2),
        _p(y1), y2.shape[1], q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), _p(sc), _p(zr)))
    return q, sc, zr


def gemv_pair_q(w, x, y2, y1, epi, nw, eps=1e-6, quant="int8", device=0):
    """fm_op_gemv_pair_q: the tile kernel's two-row ss_gran 1 form on int8 codes (fm_tune fast_pair_q).  w [N][K] is
    quantised and packed on the device; the R = 2 launch fills y2 [rows >= 2][ld], the R = 1 production launch, once per
    row on the same device operands, y1 [2][ld] (both in/out).  epi EPI_STORE or EPI_SWIGLU8.  Returns (q [N][K] int8,
    scale [N])."""
    w, nw, x = _f(w), _f(nw), _f(x)
    N, K = w.shape
    assert x.shape == (2, K) and quant == "int8"
    y2, y1 = _out(y2), _out(y1)
    assert y2.ndim == 2 and y1.ndim == 2 and y1.shape[0] == 2 and y1.shape[1] == y2.shape[1]
    q = np.zeros((N, K), np.int8)
    sc = np.zeros(N, np.float32)
    native.check(native.lib().fm_op_gemv_pair_q(device, native.FM_QUANT_INT8, int(epi), _p(w), _p(nw), float(eps), _p(x), N, K,
                                                _p(y2), y2.shape[0], _p(y1), y2.shape[1],
                                                q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), _p(sc)))
    return q, sc


PLAN_FIELDS = ("acc", "kparts", "nw", "spw", "tpi", "ntm", "grid")


def bstream(w, x, y, pro=PRO_PLAIN, epi=EPI_STORE, bias=None, nw=None, eps=1e-6, res=None, ss_out=None,
            precision="bf16", reps=1, device=0):
    """fm_op_bstream: launch_bstream on bstream_plan's geometry.  y (in/out) [rows][ldy]; epi 4: slabs
    [kparts * R (+ spare)][ldy] (kparts <= 8); epi 5: the finalised rows, ss_out [R][ceil(N / 16)] in/out.
    Returns (plan dict, dirty)."""
    w, bias, nw, x, res = _f(w), _f(bias), _f(nw), _f(x), _f(res)
    N, K = w.shape
    R, ldx = x.shape
    y = _out(y)
    plan, dirty = np.zeros(7, np.int32), np.zeros(1, np.int32)
    native.check(native.lib().fm_op_bstream(device, _prec(precision), int(pro), int(epi), _p(w), _p(bias), _p(nw),
                                            float(eps), _p(x), ldx, _p(res), 0 if res is None else res.shape[1], R, N, K,
                                            _p(y), y.shape[1], y.shape[0],
                                            None if ss_out is None else _p(_out(ss_out)), int(reps),
                                            native.i32p(plan), native.i32p(dirty)))
    return dict(zip(PLAN_FIELDS, (int(v) for v in plan))), int(dirty[0])


def finalize_norm(slab, res, x_out, d, bias=None, nw=None, wscale=None, xn_out=None, eps=1e-6, precision="bf16",
                  reps=1, device=0):
    """fm_op_finalize_norm: slab [kparts][R][lds] fp32, res [R][ldr]; x_out / xn_out in/out [rows][ld].
    Returns (split form ran, err word, dirty)."""
    slab, res, bias, nw, wscale = _f(slab), _f(res), _f(bias), _f(nw), _f(wscale)
    kparts, R, lds = slab.shape
    x_out = _out(x_out)
    split, err, dirty = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    native.check(native.lib().fm_op_finalize_norm(device, _prec(precision), _p(slab), kparts, lds, _p(bias), _p(res),
                                                  res.shape[1], _p(nw), _p(wscale), float(eps), int(d), R, _p(x_out),
                                                  x_out.shape[1], x_out.shape[0],
                                                  None if xn_out is None else _p(_out(xn_out)),
                                                  0 if xn_out is None else xn_out.shape[1],
                                                  0 if xn_out is None else xn_out.shape[0], int(reps),
                                                  native.i32p(split), native.i32p(err), native.i32p(dirty)))
    return bool(split[0]), int(err[0]), int(dirty[0])


def prompt_skinny_ks(N, K, target, device=0):
    """prompt_skinny_ks(N, K, target): the K slices the prompt path would use (0: K too short)."""
    ks = np.zeros(1, np.int32)
    native.check(native.lib().fm_op_prompt_skinny(device, None, None, 0, 0, int(N), int(K), int(target), 0, None, 0, 0,
                                                  1, native.i32p(ks)))
    return int(ks[0])


def prompt_skinny(w, x, out, target, act=False, reps=1, device=0):
    """fm_op_prompt_skinny: out (in/out) the fp32 slabs [ks * R (+ spare)][N], or with act the SwiGLU rows
    [rows >= R][ldo >= N / 2].  Returns ks."""
    w, x = _f(w), _f(x)
    N, K = w.shape
    R, ldx = x.shape
    out = _out(out)
    ks = np.zeros(1, np.int32)
    native.check(native.lib().fm_op_prompt_skinny(device, _p(w), _p(x), ldx, R, N, K, int(target), int(act), _p(out),
                                                  out.shape[0], out.shape[1], int(reps), native.i32p(ks)))
    return int(ks[0])


def prompt_skinny_q(w, x, y_q, y_bf16, quant, target, gs=128, act=False, reps=1, device=0):
    """fm_op_prompt_skinny_q: w [N][K] (bf16-valued) quantised on the device (quant "int8": per row; "int4": groups
    of gs), then launch_prompt_skinny on x [R][ldx >= K] once from the packed bf16 fragments of the quantised
    weights (y_bf16) and once from the step-granular codes alone (y_q); both shaped as prompt_skinny's out and
    filled in place.  Returns (ks, q [N][K] int8 codes, scale, zero): scale [N] and zero None for int8, both
    [N][K / gs] for int4."""
    w, x = _f(w), _f(x)
    N, K = w.shape
    R, ldx = x.shape
    y_q, y_bf16 = _out(y_q), _out(y_bf16)
    assert y_q.shape == y_bf16.shape
    q4 = quant == "int4"
    ks = np.zeros(1, np.int32)
    q = np.zeros((N, K), np.int8)
    sc = np.zeros((N, K // gs) if q4 else N, np.float32)
    zr = np.zeros((N, K // gs), np.float32) if q4 else None
    native.check(native.lib().fm_op_prompt_skinny_q(device, native.FM_QUANT_INT4 if q4 else native.FM_QUANT_INT8,
                                                    int(gs), _p(w), _p(x), ldx, R, N, K, int(target), int(act),
                                                    _p(y_q), _p(y_bf16), y_q.shape[0], y_q.shape[1], int(reps),
                                                    native.i32p(ks), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
                                                    _p(sc), _p(zr)))
    return int(ks[0]), q, sc, zr


GEMM_PLAN_FIELDS = ("kernel", "ksplit", "nseg", "epi", "seg_rows", "kernel_last")
CK_REG, CK_LDS6, CK_LDS8 = 0, 1, 2  # conv_plan's kernels: the register-tiled GEMM, the LDS-tiled one at 6 / 8 channel tiles


def prompt_gemm_q(w, x, y_q, y_bf16, quant, gs=128, bias=None, res=None, ksplit=1, reps=1, device=0):
    """fm_op_prompt_gemm_q: w [N][K] (bf16-valued) quantised on the device as prompt_skinny_q does, then the tiled
    prompt GEMM (launch_conv_gemm, bf16) on x [R][ldx >= K] once from the packed bf16 fragments of the quantised
    weights (y_bf16) and once from the step-granular codes alone (y_q): round(acc [* row scale] + bias), then
    round(res + y) with res [R][ldr >= N]; ksplit K slices.  Both outputs [rows >= R][ldo >= N] are filled in place.
    Returns (plan dict of GEMM_PLAN_FIELDS, q [N][K] int8 codes, scale, zero) -- the last three as prompt_skinny_q's."""
    w, x, bias, res = _f(w), _f(x), _f(bias), _f(res)
    N, K = w.shape
    R, ldx = x.shape
    y_q, y_bf16 = _out(y_q), _out(y_bf16)
    assert y_q.shape == y_bf16.shape and (res is None or res.shape[0] == R)
    q4 = quant == "int4"
    plan = np.zeros(6, np.int32)
    q = np.zeros((N, K), np.int8)
    sc = np.zeros((N, K // gs) if q4 else N, np.float32)
    zr = np.zeros((N, K // gs), np.float32) if q4 else None
    native.check(native.lib().fm_op_prompt_gemm_q(device, native.FM_QUANT_INT4 if q4 else native.FM_QUANT_INT8, int(gs),
                                                  _p(w), _p(bias), _p(x), ldx, R, N, K, _p(res),
                                                  0 if res is None else res.shape[1], int(ksplit), _p(y_q), _p(y_bf16),
                                                  y_q.shape[0], y_q.shape[1], int(reps), native.i32p(plan),
                                                  q.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), _p(sc), _p(zr)))
    return dict(zip(GEMM_PLAN_FIELDS, (int(v) for v in plan))), q, sc, zr


def batched_linear_q4(w, x, epi, gs=128, device=0):
    """fm_op_batched_linear_q4: the batched decode linear (8 < R <= 32 rows of x, bf16) on the device-
    quantised int4 form of w [N][K] (groups of gs along K; gs and K multiples of 128), once streaming
    the 4-bit codes + (scale, zero) words and once the bf16 fragments of the dequantised weights.
    Returns (y_q4, y_bf16, kparts, q [N][K] uint8, scale [N][K/gs], zero [N][K/gs], w_deq [N][K]);
    the outputs are shaped as batched_linear_q8's."""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    R = x.shape[0]
    No = N // 2 if epi == EPI_SWIGLU8 else N
    cap = 8 if epi == EPI_SLAB else 1  # K parts at most (bsacc_plan)
    y4 = np.zeros((cap, R, No), np.float32)
    yb = np.zeros((cap, R, No), np.float32)
    kp = np.zeros(1, np.int32)
    ng = max(K // gs, 1) if gs > 0 else 1
    q = np.zeros((N, K), np.uint8)
    sc = np.zeros((N, ng), np.float32)
    zr = np.zeros((N, ng), np.float32)
    wd = np.zeros((N, K), np.float32)
    native.check(native.lib().fm_op_batched_linear_q4(device, native.f32p(w), N, K, int(gs), native.f32p(x), R, int(epi),
                                                      native.f32p(y4), native.f32p(yb), native.i32p(kp),
                                                      q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                      native.f32p(sc), native.f32p(zr), native.f32p(wd)))
    k = int(kp[0])
    if epi == EPI_SLAB:
        return (y4.reshape(-1)[:k * R * No].reshape(k, R, No), yb.reshape(-1)[:k * R * No].reshape(k, R, No), k, q, sc,
                zr, wd)
    return y4[0], yb[0], k, q, sc, zr, wd


def sample(logits, Nl, row_slot, slots, cols, tap, slow, sb, se, im_end, cb, draw=0, col_idx=0, ras=None,
           ras_enable=False, force_cols=None, precision="bf16", device=0):
    """fm_op_sample: launch_sample_radix once on logits [R][ldl >= Nl] (fp32), row r with the parameters of
    slot row_slot[r].  slots: one dict per slot with temperature, top_p, top_k, mask_im_end, seed, step,
    force.  cols [R][ldc] int32 and tap [len(slots)][tap_ld >= Nl] float32 are in/out arrays, written in
    place; ras [len(slots)][10] and force_cols [len(slots)][ldc] int32 default to -1 / 0.  Returns the
    kernel that ran: 1 sample_fast_kernel, 0 sample_radix_kernel."""
    logits = _f(logits)
    R, ldl = logits.shape
    n = len(slots)
    row_slot = np.ascontiguousarray(row_slot, np.int32)
    assert row_slot.shape == (R,)
    for a, dt in ((cols, np.int32), (tap, np.float32)):
        assert isinstance(a, np.ndarray) and a.dtype == dt and a.ndim == 2 and a.flags.c_contiguous and a.flags.writeable
    assert cols.shape[0] == R and tap.shape[0] == n
    ldc = cols.shape[1]
    ras = np.full((n, 10), -1, np.int32) if ras is None else np.ascontiguousarray(ras, np.int32)
    force_cols = np.zeros((n, ldc), np.int32) if force_cols is None else np.ascontiguousarray(force_cols, np.int32)
    assert ras.shape == (n, 10) and force_cols.shape == (n, ldc)

    def col(key, dt):
        return np.ascontiguousarray([s[key] for s in slots], dt)

    t, p = col("temperature", np.float32), col("top_p", np.float32)
    k, m, st, fo = (col(key, np.int32) for key in ("top_k", "mask_im_end", "step", "force"))
    seed = col("seed", np.uint64)
    kernel = np.full(1, -1, np.int32)
    i32p = native.i32p
    native.check(native.lib().fm_op_sample(device, _prec(precision), int(bool(slow)), _p(logits), R, ldl, int(Nl),
                                           i32p(row_slot), n, _p(t), _p(p), i32p(k), i32p(m),
                                           seed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), i32p(st), i32p(fo),
                                           int(sb), int(se), int(im_end), int(cb), int(draw), int(col_idx), i32p(ras),
                                           int(bool(ras_enable)), i32p(force_cols), i32p(cols), ldc, _p(tap),
                                           tap.shape[1], i32p(kernel)))
    return int(kernel[0])


# ---- the codec kernels (fm_op_codec_*; tests/test_gpu_codec_ops.py) -----------------------------------
# conv_gemm epilogue flags (FM_CE_* of include/fishmi.h; bias and the Snake follow the operands)
CE_GELU, CE_RES, CE_GAMMA, CE_STORE, CE_TANH, CE_F32OUT, CE_SWIGLU, CE_ROPE, CE_NORM = 2, 4, 8, 16, 64, 128, 256, 512, 1024
CONV_KERNELS = ("conv_gemm", "conv_gemm2<6>", "conv_gemm2<8>")
CONV_EPILOGUES = ("gemm", "splitk_epi", "splitk_epi_norm")


def codec_conv(w, x, Lq, kind=0, stride=1, dil=1, strided=False, npre=0, flags=CE_STORE, bias=None, gamma=None,
               res=None, alpha2=None, normw=None, out=None, out2=None, ksplit=0, slab_rows=0, rope=None, norm_eps=1e-5,
               precision="bf16", reps=1, device=0):
    """fm_op_codec_conv: launch_conv_weight + launch_pack + launch_conv_gemm on w in torch layout (kind 0
    Conv1d [Co][Ci][k], 1 / 2 ConvTranspose1d [Ci][Co][2s] / [Ci][Co][s], 3 Linear [Co][Ci]) and x
    [npre + Lx][ldx]; out / out2 are filled in place.  rope = (pos0, nqk, hd, base) with CE_ROPE.
    Returns ({kernel, ksplit, segments, epilogue, changed, kernel_last}, dirty); kernel_last is the kernel of a
    shorter last row segment."""
    w, x, bias, gamma, res, alpha2, normw = _f(w), _f(x), _f(bias), _f(gamma), _f(res), _f(alpha2), _f(normw)
    d = native.CodecConvDesc()
    d.precision, d.kind, d.stride, d.dil, d.strided = _prec(precision), int(kind), int(stride), int(dil), int(bool(strided))
    if kind in (1, 2):
        d.Ci, d.Co, d.k = w.shape
    elif kind == 0:
        d.Co, d.Ci, d.k = w.shape
    else:
        (d.Co, d.Ci), d.k = w.shape, 1
    d.npre, d.Lx, d.ldx, d.Lq = int(npre), x.shape[0] - int(npre), x.shape[1], int(Lq)
    d.flags, d.ksplit, d.slab_rows, d.reps, d.norm_eps = int(flags), int(ksplit), int(slab_rows), int(reps), float(norm_eps)
    if rope is not None:
        d.rope_pos0, d.rope_nqk, d.rope_hd, d.rope_base = int(rope[0]), int(rope[1]), int(rope[2]), float(rope[3])
    if out is not None:
        d.out_rows, d.ldo = _out(out).shape
    if out2 is not None:
        d.out2_rows, d.ldo2 = _out(out2).shape
    if res is not None:
        d.res_rows, d.ldr = res.shape
    plan, dirty = np.zeros(6, np.int32), np.zeros(1, np.int32)
    native.check(native.lib().fm_op_codec_conv(device, ctypes.byref(d), _p(w), _p(bias), _p(x), _p(gamma), _p(res),
                                               _p(alpha2), _p(normw), _p(out), _p(out2), native.i32p(plan),
                                               native.i32p(dirty)))
    return dict(kernel=CONV_KERNELS[plan[0]], ksplit=int(plan[1]), segments=int(plan[2]),
                epilogue=CONV_EPILOGUES[plan[3]], changed=int(plan[4]), kernel_last=CONV_KERNELS[plan[5]]), int(dirty[0])


def codec_resunit(x, L, dil, w7, b7, a2, w1, b1, an, res, out2, npre=0, store_res=True, reps=1, device=0):
    """fm_op_codec_resunit: launch_resunit (bf16) on x [npre + L][C]; res and out2 are filled in place.
    Returns (taken, changed)."""
    x, w7, b7, a2, w1, b1, an = _f(x), _f(w7), _f(b7), _f(a2), _f(w1), _f(b1), _f(an)
    C = x.shape[1]
    taken, changed = np.zeros(1, np.int32), np.zeros(1, np.int32)
    native.check(native.lib().fm_op_codec_resunit(device, C, int(L), int(npre), int(dil), _p(x), _p(w7), _p(b7), _p(a2),
                                                  _p(w1), _p(b1), _p(an), _p(_out(res)), res.shape[0], int(store_res),
                                                  _p(_out(out2)), out2.shape[0], int(reps), native.i32p(taken),
                                                  native.i32p(changed)))
    return bool(taken[0]), int(changed[0])


def _reps(call, reps):
    """the trailing (reps, changed) of a codec hook -> the output words a repeated launch changed"""
    changed = np.zeros(1, np.int32)
    native.check(call(int(reps), native.i32p(changed)))
    return int(changed[0])


def codec_window_attn(qkv, Tn, H, hd, window, out, npre=0, precision="bf16", reps=1, device=0):
    """fm_op_codec_window_attn: qkv [npre + Tn][3 H hd], out [rows >= Tn][H hd] filled in place.  This and the hooks
    below return the number of output words a repeated launch (reps > 1) on the same scratch changed."""
    qkv = _f(qkv)
    L = native.lib()
    return _reps(lambda *r: L.fm_op_codec_window_attn(device, _prec(precision), _p(qkv), int(Tn), int(H), int(hd), int(window),
                                                      int(npre), _p(_out(out)), out.shape[0], *r), reps)


def codec_window_attn_seg(qkv, T, npre, gap, H, hd, window, state, out, precision="bf16", device=0):
    """fm_op_codec_window_attn_seg (the batched streamed decode's attention and K/V state refresh): segment i
    at row off[i] (off[i + 1] = off[i] + T[i] + gap) of qkv [span][3 H hd]; out [rows >= span][H hd] and state
    [n][rows >= window - 1][3 H hd] are filled in place."""
    qkv = _f(qkv)
    T, npre = np.ascontiguousarray(T, np.int32), np.ascontiguousarray(npre, np.int32)
    assert state.ndim == 3 and state.shape[0] == T.size == npre.size and qkv.shape[0] == int(T.sum()) + gap * (T.size - 1)
    native.check(native.lib().fm_op_codec_window_attn_seg(device, _prec(precision), int(T.size), native.i32p(T),
                                                          native.i32p(npre), int(gap), _p(qkv), int(H), int(hd), int(window),
                                                          _p(_out(state)), state.shape[1], _p(_out(out)), out.shape[0]))


def codec_rope_qk(qkv, Tn, H, hd, base, pos0=0, precision="bf16", reps=1, device=0):
    """fm_op_codec_rope_qk in place on qkv [rows >= Tn][3 H hd]"""
    L = native.lib()
    return _reps(lambda *r: L.fm_op_codec_rope_qk(device, _prec(precision), _p(_out(qkv)), qkv.shape[0], int(Tn), int(H), int(hd),
                                                  float(base), int(pos0), *r), reps)


def codec_dwconv_ln(x, L, dw, db, lw, lb, y, npre=0, precision="bf16", reps=1, device=0):
    """fm_op_codec_dwconv_ln: x [npre + L][D], y [rows >= L][D] filled in place"""
    x, dw, db, lw, lb = _f(x), _f(dw), _f(db), _f(lw), _f(lb)
    lib = native.lib()
    return _reps(lambda *r: lib.fm_op_codec_dwconv_ln(device, _prec(precision), _p(x), int(L), x.shape[1], int(npre), _p(dw),
                                                      _p(db), _p(lw), _p(lb), _p(_out(y)), y.shape[0], *r), reps)


def codec_rvq_decode(codes, cb_sem, cb, w, bias, z, precision="bf16", reps=1, device=0):
    """fm_op_codec_rvq_decode: codes [nq1][Tn], cb_sem [sem][cd], cb [nq1 - 1][cbs][cd], w [nq1][D][cd], bias
    [nq1][D]; z [rows >= Tn][D] filled in place"""
    codes = np.ascontiguousarray(codes, np.int32)
    cb_sem, cb, w, bias = _f(cb_sem), _f(cb), _f(w), _f(bias)
    nq1, Tn = codes.shape
    L = native.lib()
    return _reps(lambda *r: L.fm_op_codec_rvq_decode(device, _prec(precision), native.i32p(codes), Tn, nq1, cb_sem.shape[0],
                                                     cb.shape[1], cb_sem.shape[1], _p(cb_sem), _p(cb), _p(w), _p(bias),
                                                     w.shape[1], _p(_out(z)), z.shape[0], *r), reps)


def codec_snake(x, alpha, y, precision="bf16", reps=1, device=0):
    """fm_op_codec_snake: y[:x.size] = snake(x [L][C], alpha [C]) in place; returns (the fp32 reciprocals [C],
    changed)"""
    x, alpha = _f(x), _f(alpha)
    ia = np.zeros(alpha.size, np.float32)
    L = native.lib()
    changed = _reps(lambda *r: L.fm_op_codec_snake(device, _prec(precision), _p(x), alpha.size, x.size, _p(alpha), _p(_out(y)),
                                                   y.size, _p(ia), *r), reps)
    return ia, changed


def codec_silu_mul(g, y, precision="bf16", reps=1, device=0):
    """fm_op_codec_silu_mul: y[:g.size] = round(silu(g)) * y in place"""
    g = _f(g)
    L = native.lib()
    return _reps(lambda *r: L.fm_op_codec_silu_mul(device, _prec(precision), _p(g), _p(_out(y)), g.size, y.size, *r), reps)


def codec_wn_fold(g, v, w, reps=1, device=0):
    """fm_op_codec_wn_fold: w[:rows * per] = v [rows][per] * g / ||v|| in place"""
    g, v = _f(g), _f(v)
    L = native.lib()
    return _reps(lambda *r: L.fm_op_codec_wn_fold(device, _p(g), _p(v), v.shape[0], v.shape[1], _p(_out(w)), w.size, *r), reps)


def codec_vq_encode(r, wi, bi, cbs, wo, bo, reps=1, device=0):
    """fm_op_codec_vq_encode: r [Tn][D] updated in place; wi [nst][cd][D], bi [nst][cd], cbs a list of
    [cbn][cd] codebooks, wo [nst][D][cd], bo [nst][D].  Returns (the codes [nst][Tn], changed)."""
    wi, bi, wo, bo = _f(wi), _f(bi), _f(wo), _f(bo)
    nst, cd, D = wi.shape
    cb = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32) for c in cbs], 0), np.float32)
    cbn = np.array([len(c) for c in cbs], np.int32)
    Tn = r.shape[0]
    codes = np.zeros((nst, Tn), np.int32)
    L = native.lib()
    changed = _reps(lambda *a: L.fm_op_codec_vq_encode(device, _p(_out(r)), Tn, D, nst, cd, _p(wi), _p(bi), _p(cb),
                                                       native.i32p(cbn), _p(wo), _p(bo), native.i32p(codes), *a), reps)
    return codes, changed
