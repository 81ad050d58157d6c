"""float64 reference arithmetic for the linear-kernel tests (test_gpu_linear_ops.py, test_gpu_bstream_q8.py):
values carried with a per-element error bound through the kernels' documented rounding chains.  The
derivation of every term is in test_gpu_linear_ops.py's docstring."""
import numpy as np

from fishmi.synth import round_bf16

U8, U24 = 2.0 ** -8, 2.0 ** -24


def rb(prec):
    return round_bf16 if prec == "bf16" else (lambda a: np.asarray(a, np.float32))


def mk(rng, shape, prec, scale=1.0):
    return rb(prec)((rng.standard_normal(shape) * scale).astype(np.float32))


def rd(t, prec):
    """float64 -> the storage type's value (through fp32, as the kernel's fp32 registers are), as float64"""
    t32 = np.asarray(t, np.float64).astype(np.float32)
    return (round_bf16(t32) if prec == "bf16" else t32).astype(np.float64)


class V:
    """t: exact value; e: bound on |kernel's fp32 value - t|; r: the restatement (roundings applied)"""

    def __init__(self, t, e, r):
        self.t, self.e, self.r = np.asarray(t, np.float64), np.asarray(e, np.float64), np.asarray(r, np.float64)

    def __getitem__(self, ix):
        return V(self.t[ix], self.e[ix], self.r[ix])


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def v_acc(x, w, dx=None, extra=None):
    """x [R][K] . w [N][K]^T accumulated in fp32 in any order; dx: |kernel's x - x| elementwise at most"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    K = x64.shape[1]
    t = x64 @ w64.T
    ax = np.abs(x64) + (0 if dx is None else dx)
    e = 2 * K * U24 * (ax @ np.abs(w64).T if extra is None else extra(ax))
    if dx is not None:
        e = e + dx @ np.abs(w64).T
    return V(t, e, _f32(t))


def v_add(a, c):
    if c is None:
        return a
    t = a.t + c
    return V(t, a.e + U24 * (np.abs(t) + a.e), _f32(a.r + c))


def v_scale(a, s):
    t = a.t * s
    e = a.e * np.abs(s)
    return V(t, e + U24 * (np.abs(t) + e), _f32(a.r * s))


def v_rnd(a, prec):
    if prec != "bf16":
        return a
    return V(a.t, a.e + U8 * (np.abs(a.t) + a.e), rd(a.r, prec))


def _silu(g):
    return g / (1.0 + np.exp(-g))


def v_silu(a):
    t = _silu(a.t)
    g32 = a.r.astype(np.float32)
    r = (g32 / (np.float32(1) + np.exp(-g32))).astype(np.float64)
    return V(t, 1.1 * a.e + 4 * U24 * np.abs(t), r)


def v_mul(a, b):
    t = a.t * b.t
    e = np.abs(a.t) * b.e + np.abs(b.t) * a.e + a.e * b.e
    return V(t, e + U24 * (np.abs(t) + e), _f32(a.r * b.r))


def v_swiglu(g, u, prec):
    """round(silu(round(g))) * round(u), stored in the storage type"""
    return v_rnd(v_mul(v_rnd(v_silu(v_rnd(g, prec)), prec), v_rnd(u, prec)), prec)


def v_q8(a, scale, prec):
    """weight-only int8 output: round(round(acc) * scale)"""
    return v_rnd(v_scale(v_rnd(a, prec), scale), prec)


def norm_ref(x, nw, eps, prec):
    """RMSNorm prologue X' = round(round(x rs) w): (centre, dX') per the docstring's band on rs"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(nw, np.float64)
    K = x64.shape[-1]
    rs = 1.0 / np.sqrt((x64 ** 2).mean(-1, keepdims=True) + eps)
    band = ((K + 1) / 2 + 10) * U24

    def chain(s):
        a = x64 * s
        if prec == "bf16":
            return rd(rd(a, prec) * w64, prec)
        return a * w64

    c, lo, hi = chain(rs), chain(rs * (1 - band)), chain(rs * (1 + band))
    d = np.maximum(np.abs(hi - c), np.abs(lo - c))
    if prec != "bf16":
        d = d + 3 * U24 * np.abs(c)
    return c, d


def v_swiglu8(a, prec):
    """16-row tiles of 8 gate rows then the same 8 up rows -> N / 2 outputs"""
    R, N = a.t.shape
    g = a[:, np.arange(N).reshape(-1, 16)[:, :8].ravel()]
    u = a[:, np.arange(N).reshape(-1, 16)[:, 8:].ravel()]
    return v_swiglu(g, u, prec)
