"""float64 reference and per-element bounds of the codec kernels (test_gpu_codec_ops.py, test_codec_ref.py),
on the (t, e, r) triples of linear_ref.py: t the exact value with no rounding, e a bound on |kernel - t|,
r the restatement (the chain with every rounding applied to the float64 value).

Every reference is written from the operation's definition -- torch CPU float64 conv1d / conv_transpose1d
with left causal padding and the right crop, a plain LayerNorm, a plain causal window softmax,
x + sin^2(a x) / (a + 1e-9) -- and the rounding chains are the ones the kernel comments document
(fm_codec.h, fm_codec_kernels.hip).  The derivation of every term of e is in test_gpu_codec_ops.py's
docstring.  The cases of the GPU tests are built here too (conv_cases() ...), so the CPU test can run
deliberately wrong variants (the `mut` arguments) on the very same inputs.

Math-library limits: the HIP documentation shipped with ROCm states no ulp limits for the device math
functions, so the OpenCL full-profile limits ocml is built to are used: exp 3 ulp, erf 16 ulp, tanh 5 ulp
(sqrt 3, divide 2.5); 1 ulp <= 2 u24 relative.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from linear_ref import U24, V, _f32, mk, norm_ref, rb, v_acc, v_add, v_mul, v_rnd, v_scale, v_silu, v_swiglu

ULP = 2 * U24  # one fp32 ulp, relative (upper bound)
EXP_ULP, ERF_ULP, TANH_ULP, SQRT_ULP, DIV_ULP = 3, 16, 5, 3, 2.5
TWO_PI = 2 * math.pi

# The absolute error of the hardware sine (v_sin_f32) on [0, 1) revolutions.  Measured on the MI355X
# through the fp32 fm_op_codec_snake hook (test_gpu_codec_ops.test_snake_delta_sin); asserted with twice
# the measured value, and never above 2^-16 (see the docstring there).
DELTA_SIN_MEASURED = 8.642e-8  # 2^-23.46, at y = 0.53973055 (4 M arguments: 2^21 equally spaced, 2^21 uniform random)
DELTA_SIN = 2 * DELTA_SIN_MEASURED
DELTA_SIN_CAP = 2.0 ** -16

CE_GELU, CE_RES, CE_GAMMA, CE_STORE, CE_TANH, CE_F32OUT, CE_SWIGLU, CE_ROPE, CE_NORM = 2, 4, 8, 16, 64, 128, 256, 512, 1024


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


# ---- the convolution itself ------------------------------------------------------------------------------
def conv_def(x, w, kind, stride, dil, npre, Lq, strided=False, mut=None):
    """The layer's definition in float64 on x [npre + L][Ci] (time-major; rows [0, npre) are the carried
    context, everything before is causal zeros): output rows [0, Lq * stride) x Co.
    kind 0 Conv1d w [Co][Ci][k]: left pad (k - 1) dil.  strided: Conv1d k = 2s, stride s, left pad s, on the
    raw [npre s + Lq s][Ci] signal.  kind 1 ConvTranspose1d [Ci][Co][2s], stride s, right crop s.  kind 2
    ConvTranspose1d [Ci][Co][s].  kind 3 Linear [Co][Ci]."""
    x, w = _t(x), _t(w)
    if mut == "ctx_zero":  # the carried context rows read as zeros
        x = x.clone()
        x[:npre * (stride if strided else 1)] = 0
    xin = x.t()[None]  # [1][Ci][rows]
    if kind == 3:
        return (x[npre:npre + Lq] @ w.t()).numpy()
    if kind == 0:
        k = w.shape[2]
        if mut == "taps_rev":
            w = w.flip(2)
        if mut == "tap01":
            w = w.clone()
            w[:, :, [0, 1]] = w[:, :, [1, 0]]
        if mut == "dil+1":
            dil = dil + 1
        if mut == "dil-1":
            dil = max(dil - 1, 1) if dil > 1 else 2
        if strided:
            s = stride
            pad = F.pad(xin, (s, 0), mode="replicate" if mut == "zero_ctx" else "constant")
            return F.conv1d(pad, w, stride=s)[0].t()[npre:npre + Lq].numpy()
        P = (k - 1) * dil
        pad = F.pad(xin, (P, 0), mode="replicate" if mut == "zero_ctx" else "constant")  # zero_ctx: zeros read as data
        return F.conv1d(pad, w, dilation=dil)[0].t()[npre:npre + Lq].numpy()
    s = stride
    if mut == "phase_swap":
        w = torch.cat([w[:, :, :s].flip(2), w[:, :, s:].flip(2)], 2)
    if mut == "tap01" and kind == 1:
        w = torch.cat([w[:, :, s:], w[:, :, :s]], 2)
    if mut == "zero_ctx" and kind == 1:
        xin = F.pad(xin, (1, 0), mode="replicate")
        npre = npre + 1
    y = F.conv_transpose1d(xin, w, stride=s)[0].t()
    y = y[: xin.shape[2] * s]  # the causal right crop (kind 1: k - s samples; kind 2: none)
    return y[npre * s:(npre + Lq) * s].numpy()


def conv_acc(x, w, kind, stride, dil, npre, Lq, strided=False, dx=None, mut=None):
    """the fp32 accumulation as a V: E = 2 K u24 (|x| conv |w|), K = ntaps Ci, plus dx conv |w|"""
    if kind == 3 and mut is None:
        return v_acc(np.asarray(x, np.float64)[npre:npre + Lq], w, None if dx is None else np.broadcast_to(dx, np.shape(x))[npre:npre + Lq])
    t = conv_def(x, w, kind, stride, dil, npre, Lq, strided, mut)
    w64 = np.asarray(w, np.float64)
    if kind == 0:
        K = w64.shape[1] * w64.shape[2]
    elif kind == 3:
        K = w64.shape[1]
    else:
        K = w64.shape[0] * (2 if kind == 1 else 1)
    ax = np.abs(np.asarray(x, np.float64)) + (0 if dx is None else dx)
    e = 2 * K * U24 * conv_def(ax, np.abs(w64), kind, stride, dil, npre, Lq, strided)
    if dx is not None:
        e = e + conv_def(np.broadcast_to(dx, ax.shape), np.abs(w64), kind, stride, dil, npre, Lq, strided)
    return V(t, e, _f32(t))


# ---- elementwise epilogue steps ------------------------------------------------------------------------
def _erf(a):
    return torch.erf(_t(a)).numpy()


def v_gelu(a):
    """0.5 y (1 + erf(y / sqrt 2)) in fp32: Lipschitz <= 1.13; (1 + erf) is off by at most 16 ulp of erf, the
    argument's two roundings (2 u24 |arg| times erf' <= 2 / sqrt(pi) e^-arg^2, at most 1 u24) and the add's
    rounding (2 u24): 35 u24 absolute, times 0.5 |y|; then the product's rounding"""
    t = 0.5 * a.t * (1 + _erf(a.t / math.sqrt(2)))
    y32 = a.r.astype(np.float32)
    arg = (y32 * np.float32(0.70710678118654752)).astype(np.float32)
    r = (np.float32(0.5) * y32 * (np.float32(1) + _erf(arg).astype(np.float32))).astype(np.float32)
    ay = np.abs(a.t) + a.e
    return V(t, 1.13 * a.e + 0.5 * ay * (2 * ERF_ULP + 3) * U24 + 2 * U24 * (np.abs(t) + 1.13 * a.e), r.astype(np.float64))


def v_tanh(a):
    t = np.tanh(a.t)
    return V(t, a.e + TANH_ULP * ULP * np.abs(t) + TANH_ULP * ULP * a.e, _f32(np.tanh(a.r)))


def snake_def(y, alpha, mut=None):
    al = np.asarray(alpha, np.float64)
    s = np.sin(al * y)
    return y + (s if mut == "sin" else s * s) / (al + 1e-9)


def v_snake(a, alpha, mut=None):
    """y + ia sin^2(alpha y), ia = 1 / (alpha + 1e-9) in fp32; sin^2 as the hardware sine of fract(alpha y / 2 pi)."""
    al = np.asarray(alpha, np.float64)
    t = snake_def(a.t, al, mut)
    ia = 1.0 / (al + 1e-9)
    e_ia = ia * 3 * U24 + np.abs(1.0 / al - ia)  # the fp32 add may lose the 1e-9; divide, storage
    ay = np.abs(a.t) + a.e
    th = al * a.t
    s, s2 = np.abs(np.sin(th)), np.sin(th) ** 2
    # y's own error moves the angle by alpha e: |d sin^2| <= alpha e (|sin 2 theta| <= 1), so Lipschitz <= 1 + alpha ia <= 2;
    # the fp32 phase alpha y / 2 pi is off by <= 3 u24 |alpha y| / 2 pi revolutions (two products, the constant): 2 pi times that
    e_s2 = np.abs(al) * a.e + 3 * U24 * np.abs(al) * ay + 2 * np.minimum(s + np.abs(al) * a.e, 1) * DELTA_SIN + DELTA_SIN ** 2 \
        + U24 * s2 + TWO_PI * U24 * (2 * s + TWO_PI * U24)  # (fract's result is clamped below 1: 2^-24 revolutions)
    e = a.e + ia * e_s2 + e_ia * np.minimum(s2 + e_s2, 1) + U24 * ia * (s2 + e_s2) + U24 * (np.abs(t) + a.e + ia * e_s2)
    y32 = a.r.astype(np.float32)
    al32, ia32 = al.astype(np.float32), (np.float32(1) / (al.astype(np.float32) + np.float32(1e-9))).astype(np.float32)
    rev = ((al32 * y32).astype(np.float32) * np.float32(0.159154943091895336)).astype(np.float32)
    fr = (rev - np.floor(rev)).astype(np.float32)
    sn = np.sin(TWO_PI * fr.astype(np.float64)).astype(np.float32)
    r = (y32 + (ia32 * (sn * sn).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return V(t, e, r.astype(np.float64))


def v_rope(a, tab, pos0, nqk, hd):
    """(x0, x1) -> (x0 c - x1 s, x1 c + x0 s) on channels [0, nqk) at position t + pos0: two products and an add"""
    T_, C = a.t.shape
    half = hd // 2
    cs = np.asarray(tab, np.float64)[pos0:pos0 + T_]  # [T][half][2]
    t, e, r = a.t.copy(), a.e.copy(), a.r.copy()
    nh = nqk // hd
    c = np.tile(cs[:, :, 0], (1, nh))
    s = np.tile(cs[:, :, 1], (1, nh))
    x0, x1 = a[:, 0:nqk:2], a[:, 1:nqk:2]
    for (o, p, q, sg) in ((0, x0, x1, -1.0), (1, x1, x0, 1.0)):
        tt = p.t * c + sg * q.t * s
        ee = np.abs(c) * p.e + np.abs(s) * q.e
        ee = ee + U24 * (np.abs(p.t * c) + np.abs(q.t * s) + 2 * ee) + U24 * (np.abs(tt) + ee)
        rr = _f32(_f32(p.r * c) + sg * _f32(q.r * s))
        t[:, o:nqk:2], e[:, o:nqk:2], r[:, o:nqk:2] = tt, ee, rr
    return V(t, e, r)


def rope_table(S, hd, base):
    from fishmi import ops

    return ops.rope_table(S, hd, base)


def conv_ref(c, mut=None):
    """The whole call of a conv case (see conv_case) -> {"out": V, "out2": V} in output rows [Lq stride][Co']."""
    prec, fl, s = c["prec"], c["flags"], c["stride"] if c["kind"] in (1, 2) else 1
    mconv = mut if mut in ("taps_rev", "tap01", "dil+1", "dil-1", "ctx_zero", "zero_ctx", "phase_swap") else None
    a = conv_acc(c["x"], c["w"], c["kind"], c["stride"], c["dil"], c["npre"], c["Lq"], c["strided"], mut=mconv)
    rows = c["Lq"] * s
    if fl & CE_SWIGLU:
        h = c["Co"] // 2
        return {"out": v_swiglu(a[:, :h], a[:, h:], prec)}
    if c["bias"] is not None and mut != "no_bias":
        a = v_add(a, np.asarray(c["bias"], np.float64)[None])
    a = v_rnd(a, prec)
    if fl & CE_GELU:
        a = v_rnd(v_gelu(a), prec)
    if fl & CE_ROPE:
        pos0, nqk, hd, base = c["rope"]
        a = v_rnd(v_rope(a, rope_table(pos0 + c["Lq"] + 2, hd, base), pos0 + (1 if mut == "rope_pos" else 0), nqk, hd), prec)
    if fl & CE_RES:
        res = np.asarray(c["res"], np.float64)[:rows, :c["Co"]]
        if mut == "res_row":  # the residual taken from row t instead of t * stride + phase
            res = np.asarray(c["res"], np.float64)[np.arange(rows) // s, :c["Co"]]
        if fl & CE_GAMMA and mut != "no_gamma":
            a = v_rnd(v_scale(a, np.asarray(c["gamma"], np.float64)[None]), prec)
        a = v_rnd(v_add(a, res), prec)
    if fl & CE_TANH:
        a = v_tanh(a)
    out = {}
    if fl & CE_STORE:
        out["out"] = a
    if c["alpha2"] is not None:
        out["out2"] = v_rnd(v_snake(a, np.asarray(c["alpha2"], np.float64)[None], "sin" if mut == "snake_sin" else None), prec)
    return out


def norm_out2(got_out, c):
    """CE_NORM: out2 = round(round(y rs) w) of the rows the kernel stored -> (centre, bound)"""
    return norm_ref(got_out, c["normw"], c["norm_eps"], c["prec"])


# ---- cases ---------------------------------------------------------------------------------------------
SENT = 776.0  # the sentinel (bf16-exact)


def conv_case(name, prec, kind, Ci, Co, k, Lq, stride=1, dil=1, npre=0, flags=CE_STORE, bias=True, snake=False,
              strided=False, ksplit=0, slab_rows=0, rope=None, seed=0, plan=None, tune=None):
    rng = np.random.default_rng([seed, Ci, Co, k, Lq, stride, dil, npre, flags, kind])
    s_out = stride if kind in (1, 2) else 1
    ntaps = k if kind == 0 else (2 if kind == 1 else 1)
    K = ntaps * Ci
    wshape = {0: (Co, Ci, k), 1: (Ci, Co, k), 2: (Ci, Co, k), 3: (Co, Ci)}[kind]
    c = dict(name=name, prec=prec, kind=kind, Ci=Ci, Co=Co, k=k, Lq=Lq, stride=stride, dil=dil, npre=npre, flags=flags,
             strided=strided, ksplit=ksplit, slab_rows=slab_rows, rope=rope, plan=plan, tune=tune or {}, norm_eps=1e-5)
    c["w"] = mk(rng, wshape, prec, 1.0 / math.sqrt(K))
    raw_rows = (npre + Lq) * (stride if strided else 1)
    c["x"] = mk(rng, (raw_rows, Ci), prec)  # time-major; the strided view is x.reshape(npre + Lq, stride * Ci)
    c["bias"] = mk(rng, (Co,), prec, 0.5) if bias else None
    rows = Lq * s_out
    c["res"] = mk(rng, (rows + 3, Co + 8), prec) if flags & CE_RES else None
    c["gamma"] = mk(rng, (Co,), prec, 0.5) if flags & CE_GAMMA else None
    c["alpha2"] = rb(prec)(np.exp(rng.uniform(math.log(0.05), math.log(20.0), Co)).astype(np.float32)) if snake else None
    c["normw"] = rb(prec)((1 + 0.1 * rng.standard_normal(Co)).astype(np.float32)) if flags & CE_NORM else None
    return c


def _prod(**kw):
    import itertools

    keys = list(kw)
    return [dict(zip(keys, v)) for v in itertools.product(*kw.values())]


def conv_cases():
    """conv_gemm_kernel (the register kernel): both precisions, ragged tiles in both directions, every tap
    layout, context rows present / partly present / absent.  A pairwise-style cover: every value of every
    axis the issue lists occurs, the full product would be thousands of launches."""
    cases = []
    REG = dict(kernel="conv_gemm", ksplit=1, segments=1, epilogue="gemm")
    i = 0
    taps = [(7, 1), (7, 3), (7, 9), (3, 1), (1, 1)]
    for prec in ("bf16", "fp32"):
        for Lq, Co, Ci in zip((1, 63, 65, 130, 65, 130, 1, 63), (24, 40, 72, 24, 40, 72, 72, 24), (8, 48, 8, 48, 48, 8, 48, 8)):
            k, dil = taps[i % 5]
            full = (k - 1) * dil
            npre = (0, full, max(full - 2 * dil, 0) if full else 0)[i % 3]
            fl, snake = [(CE_STORE, False), (CE_STORE | CE_GELU, False), (CE_STORE | CE_RES, True), (0, True),
                         (CE_STORE | CE_RES | CE_GAMMA, False)][(i // 2) % 5]
            cases.append(conv_case(f"reg/{prec}/L{Lq}-Co{Co}-Ci{Ci}-k{k}d{dil}-n{npre}-f{fl}{'s' if snake else ''}", prec, 0,
                                   Ci, Co, k, Lq, dil=dil, npre=npre, flags=fl, snake=snake, bias=i % 4 != 3, plan=REG, seed=i))
            i += 1
        # every dilation with full, partial and no context at the K = 56 -> 64 padded shape
        for dil in (1, 3, 9):
            for npre in (0, 6 * dil, 2 * dil):
                cases.append(conv_case(f"reg/{prec}/k7-Ci8-d{dil}-n{npre}", prec, 0, 8, 40, 7, 65, dil=dil, npre=npre,
                                       flags=CE_STORE, snake=True, plan=REG, seed=100 + dil + npre))
        # the 1-channel output conv: tanh + fp32 out
        for Lq, npre in ((1, 0), (63, 6), (130, 2)):
            cases.append(conv_case(f"reg/{prec}/wave-L{Lq}-n{npre}", prec, 0, 48, 1, 7, Lq, npre=npre,
                                   flags=CE_STORE | CE_TANH | CE_F32OUT, plan=REG, seed=200 + Lq))
        # linear (one tap), k3
        cases.append(conv_case(f"reg/{prec}/linear", prec, 3, 48, 72, 1, 65, flags=CE_STORE | CE_GELU, plan=REG, seed=300))
    return cases


def tconv_cases():
    cases = []
    REG = dict(kernel="conv_gemm", ksplit=1, segments=1, epilogue="gemm")
    i = 0
    for prec in ("bf16", "fp32"):
        for kind, s in ((1, 2), (1, 8), (2, 2)):
            for Lq, npre in ((1, 0), (5, 1), (70, 0), (70, 1)):
                if kind == 2 and npre:
                    continue  # one tap: no context row is read
                fl, snake = [(CE_STORE, True), (CE_STORE | CE_RES, True), (CE_STORE | CE_RES | CE_GAMMA, False)][i % 3]
                cases.append(conv_case(f"tconv/{prec}/kind{kind}-s{s}-L{Lq}-n{npre}-f{fl}", prec, kind, 48, 40, 2 * s if kind == 1 else s,
                                       Lq, stride=s, npre=npre, flags=fl, snake=snake, plan=REG, seed=400 + i))
                i += 1
    return cases


def strided_cases():
    REG = dict(kernel="conv_gemm", ksplit=1, segments=1, epilogue="gemm")
    cases = []
    for prec in ("bf16", "fp32"):
        for s in (2, 8):
            for Lq, npre in ((1, 0), (70, 1), (65, 0)):
                cases.append(conv_case(f"strided/{prec}/s{s}-L{Lq}-n{npre}", prec, 0, 8, 40, 2 * s, Lq, stride=s, npre=npre,
                                       flags=CE_STORE, snake=True, strided=True, plan=REG, seed=500 + s + Lq))
    return cases


def conv2_cases():
    """conv_gemm2_kernel: a ragged last 128-row tile past 4096 rows (NCO 6 and 8), the 256-block route at a
    smaller Lq with wide Co, the epilogues of the register cases; each also with fm_tune conv2 = 0."""
    L6 = dict(kernel="conv_gemm2<6>", ksplit=1, segments=1, epilogue="gemm")
    L8 = dict(kernel="conv_gemm2<8>", ksplit=1, segments=1, epilogue="gemm")
    REG = dict(kernel="conv_gemm", ksplit=1, segments=1, epilogue="gemm")
    cases = []
    for prec in ("bf16", "fp32"):
        spec = [
            ("k7d9-96", dict(kind=0, Ci=96, Co=96, k=7, Lq=4096 + 37, dil=9, npre=18, flags=CE_STORE | CE_RES, snake=True, ksplit=1), L6),
            ("k7d9-96-nostore", dict(kind=0, Ci=96, Co=96, k=7, Lq=4096 + 37, dil=9, npre=54, flags=0, snake=True, ksplit=1), L6),
            ("k1-128", dict(kind=0, Ci=32, Co=128, k=1, Lq=4096 + 37, flags=CE_STORE | CE_GELU), L8),
            ("k1-128-gamma", dict(kind=3, Ci=32, Co=128, k=1, Lq=4096 + 37, flags=CE_STORE | CE_RES | CE_GAMMA), L8),
            ("blocks256-Co2048", dict(kind=3, Ci=32, Co=2048, k=1, Lq=2048 - 19, flags=CE_STORE | CE_GELU), L8),
            ("tconv-s8-Co112", dict(kind=1, Ci=32, Co=112, k=16, Lq=4096 + 5, stride=8, npre=1, flags=CE_STORE, snake=True), L6),
        ]
        for nm, kw, plan in spec:
            if prec == "fp32" and nm in ("k7d9-96-nostore", "blocks256-Co2048"):
                continue
            cases.append(conv_case(f"conv2/{prec}/{nm}", prec, plan=plan, seed=600, **kw))
            cases.append(conv_case(f"conv2off/{prec}/{nm}", prec, plan=REG, tune={"conv2": 0}, seed=600, **kw))
    return cases


def splitk_cases():
    def P(ks, seg=1, epi="splitk_epi", kernel="conv_gemm"):
        return dict(kernel=kernel, ksplit=ks, segments=seg, epilogue=epi)

    cases = []
    for prec in ("bf16", "fp32"):
        i = 0
        # K = 512: small_m gives 2 slices; 1024: 4; 2048: 8.  Two Latin squares: over the three Lq every width meets
        # every epilogue and every slice count
        for a, Lq in enumerate((1, 17, 100)):
            for b, Co in enumerate((16, 40, 512)):
                fl, snake = [(CE_STORE | CE_GELU, False), (CE_STORE | CE_RES | CE_GAMMA, False), (CE_STORE, True)][(a + b) % 3]
                Ci = (512, 2048, 1024)[(a + 2 * b) % 3]
                ks = {512: 2, 1024: 4, 2048: 8}[Ci]
                cases.append(conv_case(f"splitk/{prec}/L{Lq}-Co{Co}-K{Ci}-f{fl}", prec, 3, Ci, Co, 1, Lq, flags=fl, snake=snake,
                                       bias=i % 2 == 0, plan=P(ks), seed=700 + i))
                i += 1
        # k7 conv with context rows, Co % 16 == 8
        cases.append(conv_case(f"splitk/{prec}/k7-Co40-n4", prec, 0, 96, 40, 7, 100, dil=3, npre=4, flags=CE_STORE | CE_RES,
                               snake=True, plan=P(2), seed=720))
        # transposed conv (the decoder's first block: ks forced to 2)
        cases.append(conv_case(f"splitk/{prec}/tconv-s8", prec, 1, 64, 40, 16, 17, stride=8, npre=1, flags=CE_STORE, snake=True,
                               ksplit=2, plan=P(2), seed=721))
        # SwiGLU over [W1 | W3]
        for Lq in (1, 17, 100):
            cases.append(conv_case(f"splitk/{prec}/swiglu-L{Lq}", prec, 3, 512, 2 * 40, 1, Lq, flags=CE_STORE | CE_SWIGLU, bias=False,
                                   plan=P(2), seed=730 + Lq))
        # RoPE on q, k of a wqkv output, pos0 > 0
        for Lq, hd, pos0 in ((1, 32, 1000), (17, 64, 7), (100, 32, 1000)):
            cases.append(conv_case(f"splitk/{prec}/rope-L{Lq}-hd{hd}", prec, 3, 512, 3 * 2 * hd, 1, Lq, flags=CE_STORE | CE_ROPE,
                                   bias=False, rope=(pos0, 2 * 2 * hd, hd, 10000.0), plan=P(2), seed=740 + Lq))
        # norm epilogue: rows not a multiple of rpb (512: 4 rows per block, 1024: 2)
        for Co, Lq in ((512, 17), (1024, 17), (512, 1), (1024, 99)):
            cases.append(conv_case(f"splitk/{prec}/norm-Co{Co}-L{Lq}", prec, 3, 512, Co, 1, Lq,
                                   flags=CE_STORE | CE_RES | CE_GAMMA | CE_NORM, bias=False, plan=P(2, epi="splitk_epi_norm"),
                                   seed=750 + Co + Lq))
        # three row segments (workspace of 64 rows at Lq = 150): RoPE positions and context rows move with them
        cases.append(conv_case(f"splitk/{prec}/seg-rope", prec, 3, 512, 3 * 2 * 32, 1, 150, flags=CE_STORE | CE_ROPE, bias=False,
                               rope=(1000, 2 * 2 * 32, 32, 10000.0), slab_rows=64, plan=P(2, seg=3), seed=760))
        cases.append(conv_case(f"splitk/{prec}/seg-k7-n12", prec, 0, 96, 40, 7, 150, dil=3, npre=12, flags=CE_STORE | CE_RES, snake=True,
                               slab_rows=64, plan=P(2, seg=3), seed=761))
        cases.append(conv_case(f"splitk/{prec}/seg-tconv", prec, 1, 256, 40, 4, 150, stride=2, npre=1, flags=CE_STORE | CE_RES, snake=True,
                               slab_rows=64, plan=P(2, seg=3), seed=762))
        # conv_gemm2_kernel's own slab store (>= 256 blocks over tiles x slices): NCO 8 with a ragged last tile, NCO 6
        # past 4096 rows; and two row segments of which the shorter last one falls back to the register kernel
        cases.append(conv_case(f"splitk/{prec}/lds8", prec, 3, 512, 512, 1, 1024 - 31, flags=CE_STORE | CE_RES | CE_GAMMA,
                               ksplit=8, plan=P(8, kernel="conv_gemm2<8>"), seed=780))
        cases.append(conv_case(f"splitk/{prec}/lds6", prec, 3, 256, 112, 1, 4096 + 37, flags=CE_STORE, snake=True,
                               ksplit=8, plan=P(8, kernel="conv_gemm2<6>"), seed=781))
        cases.append(conv_case(f"splitk/{prec}/lds8-seg", prec, 3, 512, 512, 1, 1024 + 100, flags=CE_STORE | CE_GELU, ksplit=8,
                               slab_rows=1024, plan=dict(P(8, seg=2, kernel="conv_gemm2<8>"), kernel_last="conv_gemm"), seed=782))
        # forced factors
        for ks in (2, 8):
            cases.append(conv_case(f"splitk/{prec}/forced{ks}", prec, 0, 48, 40, 7, 65, dil=1, npre=6, flags=CE_STORE, snake=True,
                                   ksplit=ks, plan=P(ks), seed=770 + ks))
    return cases


def resunit_case(C, dil, npre, store_res, seed=0, cfg=None, L=None):
    """one ResidualUnit (bf16): L = one tile of the width's variant + 37"""
    BM = {64: 256, 96: 128, 128: 128, 192: 64, 256: 64, 384: 64, 512: 64, 48: 64}[C]
    if cfg is not None:
        BM = {(96, 0): 256, (96, 1): 128, (96, 2): 128, (192, 0): 128, (192, 1): 64, (192, 2): 128}[(C, cfg)]
    L = L or BM + 37
    rng = np.random.default_rng([seed, C, dil, npre, int(store_res)])
    al = lambda: rb("bf16")(np.exp(rng.uniform(math.log(0.05), math.log(20.0), C)).astype(np.float32))
    return dict(name=f"resunit/C{C}-d{dil}-n{npre}-s{int(store_res)}-cfg{cfg}", C=C, L=L, dil=dil, npre=npre, store_res=store_res,
                cfg=cfg, x=mk(rng, (npre + L, C), "bf16"), w7=mk(rng, (C, C, 7), "bf16", 1 / math.sqrt(7 * C)),
                b7=mk(rng, (C,), "bf16", 0.5), a2=al(), w1=mk(rng, (C, C, 1), "bf16", 1 / math.sqrt(C)),
                b1=mk(rng, (C,), "bf16", 0.5), an=al(), res=mk(rng, (L, C), "bf16"))


def resunit_ref(c, mut=None):
    """h = round(snake_a2(round(conv7(x) + b7))); y = round(res + round(conv1(h) + b1)); out2 = round(snake_an(y))"""
    p = "bf16"
    mconv = mut if mut in ("taps_rev", "tap01", "dil+1", "dil-1", "ctx_zero", "zero_ctx") else None
    a = conv_acc(c["x"], c["w7"], 0, 1, c["dil"], c["npre"], c["L"], mut=mconv)
    if mut != "no_bias":
        a = v_add(a, np.asarray(c["b7"], np.float64)[None])
    h = v_rnd(v_snake(v_rnd(a, p), np.asarray(c["a2"], np.float64)[None], "sin" if mut == "snake_sin" else None), p)
    w1 = np.asarray(c["w1"], np.float64)[:, :, 0]
    b = conv_acc(h.t, c["w1"], 0, 1, 1, 0, c["L"], dx=h.e)  # the kernel's h is within h.e of h.t
    b = V(b.t, b.e, _f32(h.r @ w1.T))
    y = v_rnd(v_add(v_rnd(v_add(b, np.asarray(c["b1"], np.float64)[None]), p), np.asarray(c["res"], np.float64)), p)
    return {"res": y, "out2": v_rnd(v_snake(y, np.asarray(c["an"], np.float64)[None]), p)}


# ---- the other kernels -----------------------------------------------------------------------------------
def attn_ref(qkv, Tn, H, hd, window, npre, prec, mut=None):
    """causal window softmax attention of rows [0, Tn) over keys [max(t - window + 1, -npre), t] -> V [Tn][H hd]"""
    x = np.asarray(qkv, np.float64).reshape(npre + Tn, 3, H, hd)
    t_, e_, r_ = (np.zeros((Tn, H, hd)) for _ in range(3))
    scale = 1.0 / math.sqrt(hd)
    sc32 = np.float32(1) / np.sqrt(np.float32(hd))
    if mut == "win+1":
        window += 1
    if mut == "win-1":
        window -= 1
    for t in range(Tn):
        j0 = t - window + 1
        if mut == "no_clamp":  # keys before the carried rows: zeros, but counted
            lo = j0
        else:
            lo = max(j0, -npre)
        idx = np.arange(lo, t + 1) + npre
        ok = idx >= 0
        kk = np.where(ok[:, None, None], x[np.clip(idx, 0, None), 1], 0.0)  # [nj][H][hd]
        vv = np.where(ok[:, None, None], x[np.clip(idx, 0, None), 2], 0.0)
        q = x[npre + t, 0]  # [H][hd]
        nj = len(idx)
        s = np.einsum("hd,jhd->hj", q, kk) * scale
        es = 2 * hd * U24 * np.einsum("hd,jhd->hj", np.abs(q), np.abs(kk)) * scale + 4 * U24 * np.abs(s)
        m = s.max(1, keepdims=True)
        delta = es.max(1, keepdims=True) + U24 * np.abs(s - m).max(1, keepdims=True)
        p = np.exp(s - m)
        w = p / p.sum(1, keepdims=True)
        eta = np.exp(2 * delta) * (1 + (4 * EXP_ULP + 2) * U24) - 1
        av = np.einsum("hj,jhd->hd", w, np.abs(vv))
        t_[t] = np.einsum("hj,jhd->hd", w, vv)
        # weights within w (1 +- eta); the fp32 sums of o and of l (nj terms each); the divide
        e_[t] = (eta + (2 * nj + 4) * U24) * av
        q32, k32, v32 = q.astype(np.float32), kk.astype(np.float32), vv.astype(np.float32)
        s32 = (np.einsum("hd,jhd->hj", q32, k32).astype(np.float32) * sc32).astype(np.float32)
        p32 = np.exp(s32 - s32.max(1, keepdims=True)).astype(np.float32)
        r_[t] = (np.einsum("hj,jhd->hd", p32, v32).astype(np.float32) / p32.sum(1, keepdims=True).astype(np.float32))
    return v_rnd(V(t_.reshape(Tn, H * hd), e_.reshape(Tn, H * hd), r_.reshape(Tn, H * hd)), prec)


def rope_ref(qkv, Tn, H, hd, tab, pos0, prec, mut=None):
    """rope_qk_kernel: RoPE on the q and k heads (channels [0, 2 H hd)) of rows [0, Tn), v untouched"""
    x = np.asarray(qkv, np.float64)[:Tn]
    a = v_rope(V(x, np.zeros_like(x), x), tab, pos0 + (1 if mut == "rope_pos" else 0), 2 * H * hd, hd)
    out = v_rnd(a, prec)
    out.e[:, 2 * H * hd:] = 0
    out.r[:, 2 * H * hd:] = x[:, 2 * H * hd:]
    return out


def dwconv_ln_ref(x, L, D, npre, dw, db, lw, lb, prec, mut=None):
    """depthwise causal k7 conv (left pad 6) + bias, rounded; LayerNorm(eps 1e-6) over D; one output rounding"""
    xt = _t(x).t()[None]
    w = _t(dw).reshape(D, 1, 7)
    if mut == "dw_rev":
        w = w.flip(2)
    if mut == "ctx_zero":
        xt = xt.clone()
        xt[:, :, :npre] = 0
    mode = "replicate" if mut == "zero_ctx" else "constant"  # zero_ctx: rows below lo read as data, not causal zeros
    conv = lambda a, ww: F.conv1d(F.pad(a, (6, 0), mode=mode), ww, groups=D)[0].t()[npre:npre + L].numpy()
    b64 = np.asarray(db, np.float64)[None]
    acc = conv(xt, w) + b64
    ea = 2 * 8 * U24 * (conv(xt.abs(), w.abs()) + np.abs(b64))
    v = v_rnd(V(acc, ea, _f32(acc)), prec)
    lw64, lb64 = np.asarray(lw, np.float64)[None], np.asarray(lb, np.float64)[None]

    def ln(vals, dmu=0.0, srs=1.0):
        mu = vals.mean(1, keepdims=True)
        var = ((vals - mu) ** 2).mean(1, keepdims=True)
        return (vals - (mu + dmu)) * (srs / np.sqrt(var + 1e-6)) * lw64 + lb64

    t = ln(v.t)
    mu = v.t.mean(1, keepdims=True)
    var = ((v.t - mu) ** 2).mean(1, keepdims=True)
    rs = 1 / np.sqrt(var + 1e-6)
    # the mean: D terms in any order plus the divide, and the inputs' own errors; the variance: D positive terms,
    # moved by the mean's error (second order) and by the inputs' errors (first order, <= 2 sqrt(var) rms(e))
    e_mu = (D + 2) * U24 * np.abs(v.t).mean(1, keepdims=True) + v.e.mean(1, keepdims=True)
    rms_e = np.sqrt((v.e ** 2).mean(1, keepdims=True))
    band = ((D + 1) / 2 + 2 * SQRT_ULP + 2 * DIV_ULP + 4) * U24 + (0.5 * e_mu ** 2 + (np.sqrt(var) + rms_e) * (rms_e + e_mu)) * rs ** 2
    dev = np.abs(v.t - mu)
    e = (v.e + e_mu) * rs * (1 + band) * np.abs(lw64) + dev * rs * band * np.abs(lw64) + 5 * U24 * (np.abs(t) + np.abs(lb64))
    v32 = v.r.astype(np.float32)
    mu32 = v32.mean(1, keepdims=True, dtype=np.float32)
    var32 = ((v32 - mu32) ** 2).mean(1, keepdims=True, dtype=np.float32)
    r = ((v32 - mu32) * (np.float32(1) / np.sqrt(var32 + np.float32(1e-6))) * lw64.astype(np.float32) + lb64.astype(np.float32))
    return v_rnd(V(t, e, r.astype(np.float64)), prec)


def rvq_ref(codes, cb_sem, cb, w, bias, prec):
    """z[t] = sum_q (W_q cb_q[min(code, size - 1)] + b_q): the semantic stage, then the sum of the residual stages"""
    codes = np.asarray(codes)
    nq1, Tn = codes.shape
    w64, b64 = np.asarray(w, np.float64), np.asarray(bias, np.float64)
    cd = w64.shape[2]
    t = np.zeros((Tn, w64.shape[1]))
    e = np.zeros_like(t)
    rs, rr = np.zeros(t.shape, np.float32), np.zeros(t.shape, np.float32)
    for q in range(nq1):
        book = np.asarray(cb_sem if q == 0 else cb[q - 1], np.float64)
        rows = book[np.minimum(codes[q], len(book) - 1)]  # [Tn][cd]
        a = rows @ w64[q].T + b64[q][None]
        ea = 2 * (cd + 1) * U24 * (np.abs(rows) @ np.abs(w64[q]).T + np.abs(b64[q])[None])
        t += a
        e += ea + 2 * U24 * np.abs(a)  # its add into the stage sums, and the final add
        if q == 0:
            rs = a.astype(np.float32)
        else:
            rr = (rr + a.astype(np.float32)).astype(np.float32)
    e += (nq1 + 1) * U24 * np.abs(t)
    return v_rnd(V(t, e, (rs + rr).astype(np.float64)), prec)


def silu_mul_ref(g, y, prec):
    g64, y64 = np.asarray(g, np.float64), np.asarray(y, np.float64)
    z = np.zeros_like
    return v_rnd(v_mul(v_rnd(v_silu(V(g64, z(g64), g64)), prec), V(y64, z(y64), y64)), prec)


def wn_fold_ref(g, v):
    """w = v g / ||v|| per row: the sum of `per` squares in any order ((per + 1) u24 relative, halved by the
    root), sqrt 3 ulp, divide 2.5 ulp, the product"""
    g64, v64 = np.asarray(g, np.float64), np.asarray(v, np.float64)
    per = v64.shape[1]
    t = v64 * (g64[:, None] / np.sqrt((v64 ** 2).sum(1, keepdims=True)))
    band = ((per + 1) / 2 + 2 * SQRT_ULP + 2 * DIV_ULP + 2) * U24
    v32 = v64.astype(np.float32)
    f = g64.astype(np.float32)[:, None] / np.sqrt((v32 * v32).sum(1, keepdims=True, dtype=np.float32))
    return V(t, band * np.abs(t), (v32 * f.astype(np.float32)).astype(np.float64))


def snake_ref(x, alpha, prec, mut=None):
    x64 = np.asarray(x, np.float64)
    return v_rnd(v_snake(V(x64, np.zeros_like(x64), x64), np.asarray(alpha, np.float64)[None], mut), prec)


def snake_case(prec, seed=0, L=512, C=64):
    """|alpha x| from 1e-3 to 300 (log-uniform), alpha from 0.05 to 20, both signs of x"""
    rng = np.random.default_rng([seed, L, C])
    alpha = rb(prec)(np.exp(rng.uniform(math.log(0.05), math.log(20.0), C)).astype(np.float32))
    ax = np.exp(rng.uniform(math.log(1e-3), math.log(300.0), (L, C)))
    x = rb(prec)((ax / alpha[None].astype(np.float64) * rng.choice([-1.0, 1.0], (L, C))).astype(np.float32))
    return x, alpha


def delta_sin_from(y, got):
    """The hardware sine's absolute error from an fp32 Snake run with alpha = 1 on fp32 y in [0, 2 pi):
    1 / (1 + 1e-9f) and 1 * y are exact, the phase r = fl(y * fl(1 / 2 pi)) and its fract are known exactly, and
    got = fl(y + fl(s^2)), s = sin(2 pi r) + d.  The two roundings (u24 s^2, u24 |got|) are taken off
    |got - y - sin^2(2 pi r)|; what is left, D, satisfies D <= 2 |s| |d| + d^2, so |d| >= sqrt(s^2 + D) - |s|."""
    y32 = np.asarray(y, np.float32)
    rev = (y32 * np.float32(0.159154943091895336)).astype(np.float32)
    fr = (rev - np.floor(rev)).astype(np.float32).astype(np.float64)
    s = np.sin(TWO_PI * fr)
    g = np.asarray(got, np.float64)
    D = np.abs(g - y32.astype(np.float64) - s * s) - U24 * (s * s) - U24 * np.abs(g)
    D = np.maximum(D, 0.0)
    return np.sqrt(s * s + D) - np.abs(s)


# ---- residual VQ encode (fp32) ---------------------------------------------------------------------------
def vq_case(cbn, seed, Tn=24, D=200, cd=8):
    """nst = len(cbn) stages on Tn frames of a D-wide residual; seeds are chosen (test_codec_ref.py) so that the
    reference alone shows at most 2 % of the (frame, stage) pairs undecided"""
    rng = np.random.default_rng([seed, Tn, D, cd] + list(cbn))
    nst = len(cbn)
    return dict(cbn=list(cbn), Tn=Tn, D=D, cd=cd, r=mk(rng, (Tn, D), "fp32"), wi=mk(rng, (nst, cd, D), "fp32", 1 / math.sqrt(D)),
                bi=mk(rng, (nst, cd), "fp32", 0.1), cbs=[mk(rng, (n, cd), "fp32") for n in cbn],
                wo=mk(rng, (nst, D, cd), "fp32", 1 / math.sqrt(cd)), bo=mk(rng, (nst, D), "fp32", 0.1))


# (codebook sizes, seed): 32 rows (fewer than the block's threads), 1024, and 1024 then 32s; 10 stages each
VQ_CASES = [((32,) * 10, 0), ((1024,) * 10, 1), ((1024,) + (32,) * 9, 0)]
VQ_UNDECIDED_CAP = 0.02


def vq_ref(c, nst=None, got_codes=None):
    """The chain z_e = in_proj(r); nearest l2-normalised codebook row to the l2-normalised z_e (float64 argmin of
    the squared distance); r -= out_proj(codebook[idx]).  A candidate is acceptable when its float64 distance is
    within the derived fp32 error of the best one's (e_d of both); a (frame, stage) with more than one acceptable
    candidate is undecided.  With got_codes the chain continues from the kernel's choice.
    Returns (codes [nst][Tn] float64 argmin, ok [nst][Tn]: got acceptable, undecided [nst][Tn], residual V)."""
    nst = nst or len(c["cbn"])
    Tn, D, cd = c["Tn"], c["D"], c["cd"]
    r = np.asarray(c["r"], np.float64)
    r = V(r, np.zeros_like(r), r)
    nb = ((cd + 1) / 2 + 2 * SQRT_ULP + 2 * DIV_ULP + 1) * U24  # a normalised component, relative
    codes, ok, und = (np.zeros((nst, Tn), a) for a in (np.int64, bool, bool))
    for q in range(nst):
        wi, bi = np.asarray(c["wi"][q], np.float64), np.asarray(c["bi"][q], np.float64)[None]
        cb = np.asarray(c["cbs"][q], np.float64)
        wo, bo = np.asarray(c["wo"][q], np.float64), np.asarray(c["bo"][q], np.float64)[None]
        ze = r.t @ wi.T + bi
        e_ze = 2 * (D + 1) * U24 * ((np.abs(r.t) + r.e) @ np.abs(wi).T + np.abs(bi)) + r.e @ np.abs(wi).T
        nrm = np.linalg.norm(ze, axis=1, keepdims=True)
        en = ze / nrm
        e_en = e_ze / nrm + np.abs(en) * (np.linalg.norm(e_ze, axis=1, keepdims=True) / nrm + nb)
        cn = cb / np.linalg.norm(cb, axis=1, keepdims=True)
        e_cn = np.abs(cn) * nb
        dist = ((en[:, None, :] - cn[None]) ** 2).sum(2)  # [Tn][cbn]
        e_dot = e_en @ np.abs(cn).T + np.abs(en) @ e_cn.T + 2 * cd * U24 * (np.abs(en) @ np.abs(cn).T)
        e_c2 = (2 * np.abs(cn) * e_cn + 2 * cd * U24 * cn * cn).sum(1)[None]
        e_d = 2 * e_dot + e_c2 + 7 * U24  # |e|^2 is one number for every candidate of a frame; two adds of values <= 4
        best = dist.argmin(1)
        ar = np.arange(Tn)
        accept = dist - dist[ar, best][:, None] <= e_d + e_d[ar, best][:, None]
        codes[q], und[q] = best, accept.sum(1) > 1
        pick = best if got_codes is None else np.asarray(got_codes)[q]
        ok[q] = accept[ar, pick]
        zq = cb[pick]
        e_zq = U24 * (2 * np.abs(zq) + np.abs(ze) + e_ze)
        acc = zq @ wo.T + bo
        e_acc = 2 * (cd + 1) * U24 * (np.abs(zq) @ np.abs(wo).T + np.abs(bo)) + e_zq @ np.abs(wo).T
        t = r.t - acc
        r = V(t, r.e + e_acc + U24 * (np.abs(t) + r.e + e_acc), _f32(r.r - _f32(acc)))
    return codes, ok, und, r
