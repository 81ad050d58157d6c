"""float64 reference of the attention kernels, the operand families of tests/test_gpu_attn_ops.py, and the
bounds both test files hold the kernels (and the reference's own wrong variants) to.  numpy only; the RoPE
table is the project's own bf16-valued one (ops.rope_table, built on the host).

THE OPERATION (llama.py:861-975).  A row carries a raw projection [q heads | k heads | v heads], a slot and a
position pos.  q heads and the new k head get QK-norm (x / rms(x) * w, one rounding to the storage type) and
RoPE at pos from the bf16-valued table (one rounding); the new k / v go to row pos of the row's slot and layer
of the cache [nslots][layers][nkv][S][hd]; q head h attends kv head h // (nh / nkv) over rows 0..pos of that
slot and layer: o = softmax(q K^T / sqrt(hd)) V.  q, k and v are TENSORS of the model, stored in the storage
type, so their two roundings belong to the definition (tests/test_gpu_ops.py pins them per element: 1 bf16 ulp,
4 fp32 ulp, QK_ROPE_ULPS); everything after them is what the two forms differ in:

  exact      no intermediate rounding: float64 scores, softmax and P V
  fast path  the roundings the fast decoder's kernels document (fm_attn_dev.h, llama.py:947-975):
             s = round(round(q.k) * scale), p = round(softmax(s)), o = round(p V)

BOUNDS.  Slow path (attn_fd, attn_decode2, attn_dec3, split + combine, attn_prefill_kernel): the bounds of
tests/test_gpu_ops.py as they stand, relative to the row's max |o| per head: fp32 2e-5; bf16 2^-8 (one
rounding of the output: half an ulp, at most 2^-8 of the value) + 2e-3 (decode: the
kernel's q may differ from the reference's by an ulp in an element) or + 4e-3 (attn_prefill_kernel rounds P
to bf16 for its MFMA).

Fast path, bf16, per element, against the exact form (fast_bound).  With u = 2^-8 (bf16's unit roundoff: half an ulp, relative to the value):
  * round(q.k) then round(. * scale): the score moves by at most d_j = |s_j| (2u + u^2) + 1e-6 |s_j| (the
    fp32 dot product and multiply under them).  A probability is largest when its own score is up by d_j and
    every other down by d_k, smallest the other way round; D_j is the larger distance of the two from p_j,
    computed exactly per key (at most 63 keys).
  * round(p): at most u (p_j + D_j) more.
  * P V in fp32, then the store's rounding: u (|o| + the above) more, plus 1e-6 sum p |v| for the fp32 sum.
  E = sum_j (D_j + u (p_j + D_j)) |v_j|, bound = E + u (|o| + E) + 1e-6 sum_j p_j |v_j|.
In fp32 none of these roundings exists and the slow path's 2e-5 holds.

fp32, the `large` family (fp32_large_tol).  The 2e-5 above was set for scores of a few units.  At |s| = 100 fp32
itself does not reach it: half an ulp of such a score is 4e-6, and an hd-term fp32 dot product of that size carries
more.  float32_restatement evaluates the definition in plain float32, one key and one dimension after the other (no
kernel involved), and lands at 1.6e-5 .. 3.8e-5 on these inputs.  So this one family is held, in fp32, to
2e-5 + 4 E_r of the head's max |o|, E_r the restatement's own worst error on the very case: at most 1.8e-4 here, and
a kernel has to be about as good as a sequential fp32 sum.  bf16 keeps the slow bound for `large`, as every other
family does in both precisions.

Nothing here was tuned on kernel output.  An omitted fast-path rounding does NOT separate: the bound is the sum of the roundings, so a kernel
that skips one is closer to the exact form, not further (test_attn_ref.py asserts exactly that).

OPERAND FAMILIES (make_case; seeded, rounded to the storage type).  Scores are steered through
u_kv = sqrt(hd) pinv(Q) 1, the least-norm vector with q_h . u_kv / sqrt(hd) = 1 for every q head h of the kv
group (Q = the group's q heads AFTER QK-norm and RoPE), so a key t u_kv scores t for the whole group.  The
new key of row pos goes through QK-norm and RoPE itself: its raw row is the inverse rotation of the wanted key.
  diffuse  N(0,1) raw rows and cache, QK-norm weights 1 + 0.1 N(0,1): today's operands
  peaked   one key at position `peak` scores PEAK above the others' few units (asserted: margin >= 30, p >= 0.999)
  rising   s_j = -step (pos - j): the running maximum rises with every position; step = min(3, 280 / pos), so
           several units per position in a short context, several per pass in a long one, |s| <= 280
  falling  s_j = -step j: the first position sets the maximum for good
  large    s_j uniform in [60, 100] (+ a unit of noise): from 89 on exp(s) overflows fp32 without the max
           subtraction, and the few keys near the top share the weight
  tied     every key 0: o is the mean of V over 0..pos exactly
QK-norm is on for diffuse only (a normalised new key cannot be scaled to a wanted score).  Every cache word
the kernel must not read is NaN: rows > pos, the stale row pos itself, every other slot and layer.
"""
import numpy as np

from fishmi import ops
from fishmi.synth import round_bf16

U = 2.0 ** -8  # bf16 unit roundoff: 8 significant bits, half an ulp is at most 2^-8 of the value
SLOW_TOL = {"fp32": 2e-5, "bf16": 2.0 ** -8 + 2e-3, "bf16_flash": 2.0 ** -8 + 4e-3}
QK_ROPE_ULPS = {"bf16": 1, "fp32": 4}  # tests/test_gpu_ops.py _check
PEAK = 100.0
FAMILIES = ("diffuse", "peaked", "rising", "falling", "large", "tied")


def rb(precision):
    return round_bf16 if precision == "bf16" else (lambda a: np.asarray(a, np.float32))


_TABLES = {}


def rope(S, hd, base):
    key = (S, hd, base)
    if key not in _TABLES:
        _TABLES[key] = ops.rope_table(S, hd, base).astype(np.float64)  # [S][hd/2][2] cos, sin
    return _TABLES[key]


def prep(x, w, cs, rnd, norm_eps=1e-6):
    """QK-norm (w None: off) + RoPE with (cos, sin) rows cs [hd/2][2] of heads x [..., hd]; both rounded."""
    x = np.asarray(x, np.float64)
    if w is not None:
        x = rnd(x / np.sqrt((x * x).mean(-1, keepdims=True) + norm_eps) * np.asarray(w, np.float64)).astype(np.float64)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    c, s = cs[:, 0], cs[:, 1]
    y = np.empty_like(x)
    y[..., 0::2] = x0 * c - x1 * s
    y[..., 1::2] = x1 * c + x0 * s
    return rnd(y).astype(np.float64)


def prep_unit(x, w, y, precision, rnd, norm_eps=1e-6):
    """the unit the QK_ROPE_ULPS bound of y = prep(x, w, ..) counts in.  bf16: an ulp of the element, as
    tests/test_gpu_ops.py has it.  fp32: an ulp of the larger of the element and the rotation's operands (the pair's
    normed values): y0 = x0 c - x1 s cancels, so an fp32 evaluation is exact to ulps of its terms, not of a small
    result -- the goldens of test_gpu_ops.py never cancel far enough to show it, the steered keys here do."""
    if precision == "bf16":
        return ulp(y, precision)
    x = np.asarray(x, np.float64)
    if w is not None:
        x = rnd(x / np.sqrt((x * x).mean(-1, keepdims=True) + norm_eps) * np.asarray(w, np.float64)).astype(np.float64)
    m = np.repeat(np.maximum(np.abs(x[..., 0::2]), np.abs(x[..., 1::2])), 2, axis=-1)
    return ulp(np.maximum(m, np.abs(y)), precision)


def unrope(y, cs):
    """raw row whose rotation by cs is y (the bf16-valued (cos, sin) are not exactly on the unit circle)"""
    y0, y1 = y[..., 0::2], y[..., 1::2]
    c, s = cs[:, 0], cs[:, 1]
    n = c * c + s * s
    x = np.empty_like(y)
    x[..., 0::2] = (y0 * c + y1 * s) / n
    x[..., 1::2] = (y1 * c - y0 * s) / n
    return x


def softmax_pv(s, V):
    p = np.exp(s - s.max())
    p /= p.sum()
    return p @ V, p


def attend(q, K, V, rnd=None, fast=False, mut=None, tile=64, split=256):
    """o [hd] of one q head over keys K [n][hd], values V [n][hd].  fast: the fast path's roundings (rnd).
    mut: a deliberately wrong variant --
      no_rescale   online softmax over tiles of `tile` keys whose accumulator is not rescaled when the maximum rises
      drop_split   the combine leaves out the last split of `split` keys (nothing to drop with one split)
      no_round_s / no_round_p / no_round_o   one fast-path rounding omitted"""
    hd = q.shape[-1]
    scale = 1.0 / np.sqrt(hd)
    if fast:
        r = lambda a: rnd(a).astype(np.float64)
        s = K @ q
        s = s * scale if mut == "no_round_s" else r(r(s) * np.float64(np.float32(scale)))
        p = np.exp(s - s.max())
        p = p / p.sum()
        if mut != "no_round_p":
            p = r(p)
        o = p @ V
        return o if mut == "no_round_o" else r(o)
    s = (K @ q) * scale
    if mut == "drop_split" and len(s) > split:
        keep = (len(s) - 1) // split * split
        s, V = s[:keep], V[:keep]
    if mut == "no_rescale":
        m, l, o = -np.inf, 0.0, np.zeros(hd)
        for j0 in range(0, len(s), tile):
            sj = s[j0:j0 + tile]
            m = max(m, sj.max())
            p = np.exp(sj - m)
            l, o = l + p.sum(), o + p @ V[j0:j0 + tile]
        return o / l
    return softmax_pv(s, V)[0]


def score_bound(s, p, o, V, d, tail):
    """bound [hd] on |o' - o| when score j may move by d_j: a probability is largest with its own score up by d_j and
    every other down by d_k, smallest the other way round; D_j is the larger distance of the two from p_j.  tail(E):
    what the roundings after the scores add to E = sum_j D_j |v_j|."""
    up, dn = np.exp(s + d - s.max()), np.exp(s - d - s.max())
    pmax = up / (up + (dn.sum() - dn))
    pmin = dn / (dn + (up.sum() - up))
    return tail(np.maximum(pmax - p, p - pmin))


def fast_bound(q, K, V):
    """(o exact [hd], bound [hd]) of the bf16 fast path for one q head: the derivation in the module docstring"""
    s = (K @ q) / np.sqrt(q.shape[-1])
    o, p = softmax_pv(s, V)
    aV = np.abs(V)

    def tail(D):
        E = (D + U * (p + D)) @ aV
        return E + U * (np.abs(o) + E) + 1e-6 * (p @ aV)
    return o, score_bound(s, p, o, V, np.abs(s) * (2 * U + U * U + 1e-6), tail)


# ---- cases ------------------------------------------------------------------------------------------------
def make_case(family, nh, nkv, hd, pos, S, precision="bf16", row_slot=None, nslots=None, layers=1, layer=0, peak=None,
              seed=0, rope_base=10000.0):
    """A decode case: R = len(pos) rows, row r in slot row_slot[r] (default r) at pos[r].  Returns a dict with the raw
    rows `qkv`, the poisoned caches `kc` / `vc` [nslots][layers][nkv][S][hd] (float32, NaN where no kernel may read),
    the QK-norm weights (None: off) and the geometry."""
    rnd = rb(precision)
    pos = np.atleast_1d(np.asarray(pos, np.int32))
    R, g = len(pos), nh // nkv
    row_slot = np.arange(R, dtype=np.int32) if row_slot is None else np.asarray(row_slot, np.int32)
    nslots = int(row_slot.max()) + 1 if nslots is None else nslots
    rng = np.random.default_rng([seed, FAMILIES.index(family), nh, nkv, hd, int(pos.sum()), R])
    norm = family == "diffuse"
    qn = rnd(1.0 + 0.1 * rng.standard_normal(hd)) if norm else None
    kn = rnd(1.0 + 0.1 * rng.standard_normal(hd)) if norm else None
    tab = rope(S, hd, rope_base)
    ld = (nh + 2 * nkv) * hd
    qkv = rnd(rng.standard_normal((R, ld))).astype(np.float32)
    kc = np.full((nslots, layers, nkv, S, hd), np.nan, np.float32)
    vc = np.full_like(kc, np.nan)
    peaks = np.broadcast_to(np.asarray(pos if peak is None else peak, np.int32), (R,)).copy()
    for r in range(R):
        n = int(pos[r])  # cached rows 0..n-1, the new row n
        vc[row_slot[r], layer, :, :n] = rnd(rng.standard_normal((nkv, n, hd)))
        K = rng.standard_normal((nkv, n + 1, hd))  # wanted keys incl. the new one (diffuse: the cached ones only)
        if family != "diffuse":
            q = prep(qkv[r, : nh * hd].reshape(nkv, g, hd), None, tab[n], rnd)
            j = np.arange(n + 1, dtype=np.float64)
            if family == "peaked":
                t, noise = np.zeros(n + 1), 0.5
                t[peaks[r]] = PEAK
            elif family == "rising":
                t, noise = -min(3.0, 280.0 / max(n, 1)) * (n - j), 0.0
            elif family == "falling":
                t, noise = -min(3.0, 280.0 / max(n, 1)) * j, 0.0
            elif family == "large":
                t, noise = rng.uniform(60.0, 100.0, n + 1), 1.0
            else:
                t, noise = np.zeros(n + 1), 0.0
            for kv in range(nkv):
                u = np.sqrt(hd) * np.linalg.pinv(q[kv]) @ np.ones(g)  # q_h . u / sqrt(hd) = 1 for the group
                K[kv] = t[:, None] * u[None, :] + noise * K[kv]
            # the new key is what QK-norm (off) + RoPE make of the raw row
            qkv[r, nh * hd:(nh + nkv) * hd] = rnd(unrope(K[:, n], tab[n])).reshape(-1)
        kc[row_slot[r], layer, :, :n] = rnd(K[:, :n])
    return dict(family=family, nh=nh, nkv=nkv, hd=hd, R=R, S=S, pos=pos, row_slot=row_slot, nslots=nslots, layers=layers,
                layer=layer, qkv=qkv, kc=kc, vc=vc, qn=qn, kn=kn, precision=precision, rope_base=rope_base, peak=peaks)


def reference(c, fast=False, mut=None, bound=False, **kw):
    """(out [R][nh][hd], new k [R][nkv][hd], new v [R][nkv][hd]) of case c in float64; bound: fast_bound's
    per-element bound as a fourth array.
    mut: a wrong variant -- attend()'s, or
      mask+1 / mask-1   rows 0..pos+1 / 0..pos-1 attended
      stale_row         the cache's stale row pos used, not the new k / v
      no_slot           row r reads slot r, not row_slot[r]
      no_layer          layer 0 read, not the case's layer
      kv_head           q head h uses kv head h % nkv
      rope+1 / rope-1   q and the new k rotated for position pos +- 1
    kw: attend()'s tile / split (the pass and split sizes of the kernel the variant mimics)"""
    rnd = rb(c["precision"])
    nh, nkv, hd, R = c["nh"], c["nkv"], c["hd"], c["R"]
    g = nh // nkv
    tab = rope(c["S"], hd, c["rope_base"])
    out = np.zeros((R, nh, hd))
    bnd = np.zeros((R, nh, hd))
    knew, vnew = np.zeros((R, nkv, hd)), np.zeros((R, nkv, hd))
    for r in range(R):
        n = int(c["pos"][r])
        rp = min(max(n + (1 if mut == "rope+1" else -1 if mut == "rope-1" else 0), 0), c["S"] - 1)
        raw = c["qkv"][r].astype(np.float64)
        q = prep(raw[: nh * hd].reshape(nh, hd), c["qn"], tab[rp], rnd)
        knew[r] = prep(raw[nh * hd:(nh + nkv) * hd].reshape(nkv, hd), c["kn"], tab[rp], rnd)
        vnew[r] = raw[(nh + nkv) * hd:].reshape(nkv, hd)
        slot = r if mut == "no_slot" else c["row_slot"][r]
        layer = 0 if mut == "no_layer" else c["layer"]
        K = c["kc"][slot, layer].astype(np.float64)
        V = c["vc"][slot, layer].astype(np.float64)
        if mut != "stale_row":
            K[:, n], V[:, n] = knew[r], vnew[r]
        hi = min(n + 1 + (1 if mut == "mask+1" else -1 if mut == "mask-1" else 0), c["S"])
        for h in range(nh):
            kv = h % nkv if mut == "kv_head" else h // g
            if hi == 0:
                out[r, h] = np.nan  # (mask-1 at position 0: nothing left to attend)
                continue
            if bound:
                out[r, h], bnd[r, h] = fast_bound(q[h], K[kv, :hi], V[kv, :hi])
            else:
                out[r, h] = attend(q[h], K[kv, :hi], V[kv, :hi], rnd, fast, mut, **kw)
    return (out, knew, vnew, bnd) if bound else (out, knew, vnew)


def probs(c):
    """float64 probabilities [R][nh] -> array over 0..pos, of case c"""
    rnd = rb(c["precision"])
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    tab = rope(c["S"], hd, c["rope_base"])
    res = []
    for r in range(c["R"]):
        n = int(c["pos"][r])
        raw = c["qkv"][r].astype(np.float64)
        q = prep(raw[: nh * hd].reshape(nh, hd), c["qn"], tab[n], rnd)
        K = c["kc"][c["row_slot"][r], c["layer"]].astype(np.float64)
        K[:, n] = prep(raw[nh * hd:(nh + nkv) * hd].reshape(nkv, hd), c["kn"], tab[n], rnd)
        row = []
        for h in range(nh):
            s = K[h // (nh // nkv), : n + 1] @ q[h] / np.sqrt(hd)
            p = np.exp(s - s.max())
            row.append((s, p / p.sum()))
        res.append(row)
    return res


def rel_err(got, ref):
    """max over elements of |got - ref| / (the head's max |ref|); NaN anywhere counts as infinite"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not (np.isfinite(got).all() and np.isfinite(ref).all()):
        return np.inf
    return float((np.abs(got - ref) / np.abs(ref).max(axis=-1, keepdims=True)).max())


def ulp(v, precision):
    a = np.maximum(np.abs(np.asarray(v, np.float32)), np.float32(2.0 ** -126))
    return np.exp2(np.floor(np.log2(a)) - 7).astype(np.float32) if precision == "bf16" else np.spacing(a)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the GPU tests' inputs (tests/test_gpu_attn_ops.py runs them, tests/test_attn_ref.py shows they bite) ----------
FD_NSP = 16   # fm_kernels.h: most attn_fd splits per (row, kv head); the hook reports it and the GPU test compares
ATT3_CH = 64  # fm_attn.hip: positions per attn_dec3 block


def fd_split(npos, cap, nsp_max=FD_NSP):
    """(splits, positions per split) attn_fd cuts npos positions into, as the kernel computes them from pos;
    attn_decode2 does the same with no limit on the splits (nsp_max None); attn_dec3 (nsp_max 0) walks fixed blocks
    of cap = ATT3_CH positions"""
    if nsp_max == 0:
        return -(-npos // cap), cap
    nsp = -(-npos // cap) if nsp_max is None else min(nsp_max, -(-npos // cap))
    chunk = (-(-npos // nsp) + 15) & ~15
    return -(-npos // chunk), chunk


def fd_positions(nw, cap, S, nsp_max=FD_NSP):
    """the positions of the issue's list for a kernel of 16 nw positions per pass and splits of >= cap positions"""
    tile, full = 16 * nw, (nsp_max or FD_NSP) * cap
    ps = {0, tile - 1, tile, cap - 1, cap, cap + 1, 2 * cap, full - 1, full, S - 1}
    # one position whose last split holds a single row (the smallest past two splits)
    ps.add(next(n - 1 for n in range(2 * cap, S + 1) if n - (fd_split(n, cap, nsp_max)[0] - 1) * fd_split(n, cap, nsp_max)[1] == 1))
    return sorted(p for p in ps if 0 <= p < S)


def peak_places(pos, nw, cap, nsp_max=FD_NSP):
    """where the peaked key goes: position 0, the last row of a split, the first of the next, a pass boundary,
    pos - 1, pos"""
    nsp, chunk = fd_split(pos + 1, cap, nsp_max)
    ps = {0, chunk - 1, chunk, 16 * nw - 1, 16 * nw, pos - 1, pos}
    if nsp > 2:
        ps |= {(nsp - 1) * chunk - 1, (nsp - 1) * chunk}
    return sorted(p for p in ps if 0 <= p <= pos)


def form_nsp_max(kernel):
    """fd_split's nsp_max of a hook kernel: attn_fd FD_NSP splits, attn_decode2 any number, attn_dec3 fixed blocks"""
    return {"fd": FD_NSP, "slow": None, "slow3": 0}[kernel]


# slow decode launch forms: name -> (hook kernel, nwb, cap, S, [(nh, nkv, hd)]); S a little past FD_NSP * cap
SLOW_FORMS = {
    "fd4": ("fd", 4, 32, 16 * 32 + 72, [(4, 1, 128), (3, 1, 64), (2, 2, 32)]),
    "fd8": ("fd", 8, 32, 16 * 32 + 72, [(4, 1, 64), (6, 2, 128), (1, 1, 32)]),
    "fd16": ("fd", 16, 48, 16 * 48 + 40, [(4, 1, 32), (3, 1, 128), (2, 2, 64)]),
    "decode2": ("slow", 4, 32, 16 * 32 + 72, [(5, 1, 32), (8, 2, 128), (3, 1, 64)]),
    "dec3": ("slow3", 4, ATT3_CH, 16 * 32 + 72, [(6, 1, 128), (4, 2, 64), (1, 1, 32)]),
}


def slow_form_cases(form, precision, shape):
    """every (family, position) case of one launch form and shape: peaked at every position of the list (the peak
    walking through peak_places), the other five families at every position"""
    kernel, nw, cap, S, _ = SLOW_FORMS[form]
    nsp_max = form_nsp_max(kernel)
    nh, nkv, hd = shape
    out = []
    for i, pos in enumerate(fd_positions(nw, cap, S, nsp_max)):
        places = peak_places(pos, nw, cap, nsp_max)
        out.append(make_case("peaked", nh, nkv, hd, [pos], S, precision, peak=places[i % len(places)], seed=1))
        for fam in ("diffuse", "rising", "falling", "large", "tied"):
            out.append(make_case(fam, nh, nkv, hd, [pos], S, precision, seed=1))
    return out


def peak_walk_cases(form, precision, shape):
    """the peaked key at every place of peak_places, at a position deep in the last split and at 2 cap"""
    kernel, nw, cap, S, _ = SLOW_FORMS[form]
    nsp_max = form_nsp_max(kernel)
    nh, nkv, hd = shape
    return [make_case("peaked", nh, nkv, hd, [pos], S, precision, peak=pk, seed=2)
            for pos in (2 * cap, S - 7) for pk in peak_places(pos, nw, cap, nsp_max)]


def slot_cases(form, precision, shape):
    """R = 1, 3, 9 rows in shuffled, non-contiguous slots of a two-layer cache, layer 1; positions across the splits"""
    kernel, nw, cap, S, _ = SLOW_FORMS[form]
    nh, nkv, hd = shape
    S = 6 * cap + 24
    out = []
    for R, fam in ((1, "peaked"), (3, "rising"), (3, "diffuse"), (9, "peaked"), (9, "large")):
        rng = np.random.default_rng(100 + R)
        slots = rng.permutation(R + 4)[:R]
        pos = [int(v) for v in rng.permutation([0, 1, cap - 1, cap, 2 * cap + 1, 3 * cap, 5 * cap + 7, S - 1, 17])[:R]]
        out.append(make_case(fam, nh, nkv, hd, pos, S, precision, row_slot=slots, nslots=R + 4, layers=2, layer=1,
                             peak=[max(p - 1, 0) for p in pos], seed=3))
    return out


def frame_cases(R, cap, precision):
    """R rows as a frame holds them (slot r), positions around the frame's own cap; S just past FD_NSP * cap for one row"""
    S = FD_NSP * cap + 40 if R == 1 else 2 * cap + 40
    hd = 128 if R == 1 else 64
    if R == 1:
        return [make_case(fam, 4, 1, hd, [pos], S, precision, peak=pk, seed=4)
                for fam, pos, pk in (("peaked", cap - 1, 0), ("peaked", cap, cap - 1), ("rising", 2 * cap, None),
                                     ("peaked", FD_NSP * cap - 1, FD_NSP * cap - 2), ("peaked", FD_NSP * cap, cap),
                                     ("falling", S - 1, None), ("tied", cap + 1, None), ("diffuse", 3 * cap + 5, None))]
    pos = [0, cap - 1, cap, cap + 1, 2 * cap, S - 1, 17, 2 * cap + 1, 130][:R]
    return [make_case(fam, 4, 2, hd, pos, S, precision, peak=[max(p - 1, 0) for p in pos], seed=4)
            for fam in ("peaked", "rising", "diffuse")]


FAST_SHAPES = [(4, 4, 64), (4, 2, 128), (4, 1, 64), (2, 1, 256)]  # g = 1, 2, 4; hd 64, 128, 256
FAST_FAMILIES = ("diffuse", "peaked", "rising", "large", "tied")


def fast_cases(shape, precision, cpos, S, R=1):
    """the fast decoder's cases at codebook position cpos of S: every row of a frame sits at the same position"""
    nh, nkv, hd = shape
    slots = np.random.default_rng(7 + R).permutation(R + 2)[:R]
    return [make_case(fam, nh, nkv, hd, [cpos] * R, S, precision, row_slot=slots, nslots=R + 2, layers=2, layer=1,
                      peak=[(cpos * (r + 1)) // 3 for r in range(R)], seed=5)
            for fam in FAST_FAMILIES]


def slab_form(c, kp, with_bias, seed=6):
    """(slab [kp][R][ld] fp32, bias [ld] or None, the same operands as a qkv row): K-part slabs whose
    round(sum + bias), summed in fp32 in the kernels' order (part 0, 1, .., then the bias), is the returned qkv"""
    rng = np.random.default_rng([seed, kp, int(with_bias)])
    rnd = rb(c["precision"])
    R, ld = c["qkv"].shape
    slab = (rng.standard_normal((kp, R, ld)) / np.sqrt(kp)).astype(np.float32)
    bias = rnd(0.25 * rng.standard_normal(ld)).astype(np.float32) if with_bias else None
    acc = slab[0].copy()
    for q in range(1, kp):
        acc = acc + slab[q]
    if with_bias:
        acc = acc + bias[None, :]
    return slab, bias, rnd(acc).astype(np.float32)


def prompt_from_decode(c):
    """case c as the prompt path sees it after qk_rope_cache: (q [R][nh * hd], kc, vc with row pos written)"""
    rnd = rb(c["precision"])
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    tab = rope(c["S"], hd, c["rope_base"])
    _, knew, vnew = reference(c)
    kc, vc = c["kc"].copy(), c["vc"].copy()
    q = np.zeros((c["R"], nh * hd), np.float32)
    for r in range(c["R"]):
        n = int(c["pos"][r])
        q[r] = prep(c["qkv"][r, : nh * hd].astype(np.float64).reshape(nh, hd), c["qn"], tab[n], rnd).reshape(-1)
        kc[c["row_slot"][r], c["layer"], :, n] = knew[r]
        vc[c["row_slot"][r], c["layer"], :, n] = vnew[r]
    return q, kc, vc


def make_prompt_case(family, nh, nkv, hd, R, pos0, S, precision="bf16", slot=0, nslots=1, layers=1, layer=0, seed=0):
    """R prompt rows at positions pos0 .. pos0 + R - 1 of one slot, as launch_attn gets them: q [R][nh * hd] after
    QK-norm and RoPE, caches holding every row <= pos0 + R - 1 (NaN elsewhere).  Row i attends rows 0 .. pos0 + i.
      diffuse  N(0,1)
      peaked   row i's own key (position pos0 + i) scores PEAK for row i: a causal mask one short loses it
      rising   every row's q is one direction + 10 % noise, s_j ~ -step (P - j) with P the last position: for each
               row the maximum rises up to its own last key"""
    rnd = rb(precision)
    g, P = nh // nkv, pos0 + R  # P rows in the cache
    rng = np.random.default_rng([seed, 50 + FAMILIES.index(family), nh, nkv, hd, R, pos0])
    q = rng.standard_normal((R, nkv, g, hd))
    K = rng.standard_normal((nkv, P, hd))
    if family == "rising":
        q = q[:1] + 0.1 * q
    q = rnd(q).astype(np.float64)
    if family == "peaked":
        K *= 0.5
        for i in range(R):
            for kv in range(nkv):
                K[kv, pos0 + i] += PEAK * np.sqrt(hd) * np.linalg.pinv(q[i, kv]) @ np.ones(g)
    elif family == "rising":
        t = -min(3.0, 280.0 / max(P - 1, 1)) * (P - 1 - np.arange(P))
        for kv in range(nkv):
            K[kv] = t[:, None] * (np.sqrt(hd) * np.linalg.pinv(q[0, kv]) @ np.ones(g))[None, :]
    kc = np.full((nslots, layers, nkv, S, hd), np.nan, np.float32)
    vc = np.full_like(kc, np.nan)
    kc[slot, layer, :, :P] = rnd(K)
    vc[slot, layer, :, :P] = rnd(rng.standard_normal((nkv, P, hd)))
    return dict(family=family, nh=nh, nkv=nkv, hd=hd, R=R, S=S, pos0=pos0, slot=slot, nslots=nslots, layers=layers,
                layer=layer, q=q.reshape(R, nh * hd).astype(np.float32), kc=kc, vc=vc, precision=precision)


def prompt_reference(c, mut=None):
    """out [R][nh][hd] of a make_prompt_case case; mut "mask-1" / "mask+1": the causal mask one key off"""
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    K = c["kc"][c["slot"], c["layer"]].astype(np.float64)
    V = c["vc"][c["slot"], c["layer"]].astype(np.float64)
    q = c["q"].astype(np.float64).reshape(c["R"], nh, hd)
    out = np.zeros((c["R"], nh, hd))
    for i in range(c["R"]):
        hi = min(c["pos0"] + i + 1 + (1 if mut == "mask+1" else -1 if mut == "mask-1" else 0), c["S"])
        for h in range(nh):
            out[i, h] = attend(q[i, h], K[h // (nh // nkv), :hi], V[h // (nh // nkv), :hi]) if hi > 0 else np.nan
    return out


PROMPT_CHUNKS = [(1, 0), (15, 0), (16, 0), (17, 0), (37, 0), (16, 45), (37, 101)]  # (R, pos0): ragged blocks, prefixes not a multiple of 32


def float32_restatement(c):
    """out [R][nh][hd]: the definition evaluated in float32, one key and one dimension after the other -- no kernel,
    no trick, only the format (q, the new k and v are the reference's storage-typed tensors)"""
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    _, knew, vnew = reference(c)
    tab = rope(c["S"], hd, c["rope_base"])
    out = np.zeros((c["R"], nh, hd))
    for r in range(c["R"]):
        n = int(c["pos"][r])
        q = prep(c["qkv"][r, : nh * hd].astype(np.float64).reshape(nh, hd), c["qn"], tab[n], rb(c["precision"])).astype(np.float32)
        K, V = c["kc"][c["row_slot"][r], c["layer"]].copy(), c["vc"][c["row_slot"][r], c["layer"]].copy()
        K[:, n], V[:, n] = knew[r], vnew[r]
        for h in range(nh):
            kv = h // (nh // nkv)
            acc = np.zeros(n + 1, np.float32)
            for e in range(hd):
                acc = acc + K[kv, : n + 1, e] * q[h, e]
            s = acc * np.float32(1 / np.sqrt(hd))
            p = np.exp(s - s.max())
            out[r, h] = (p @ V[kv, : n + 1]) / p.sum(dtype=np.float32)
    return out


def fp32_large_tol(c):
    """the fp32 `large` family's tolerance relative to the head's max |o|: 2e-5 + 4 x the float32 restatement's own
    worst error on this case (module docstring)"""
    return SLOW_TOL["fp32"] + 4 * rel_err(float32_restatement(c), reference(c)[0])


def slow_share(c, out, tol=None):
    """the worst error of a slow-path output as a share of its tolerance (<= 1 passes), relative to the head's max |o|:
    SLOW_TOL (or tol); fp32_large_tol for the fp32 `large` family"""
    if tol is None:
        tol = fp32_large_tol(c) if c["precision"] == "fp32" and c["family"] == "large" else SLOW_TOL[c["precision"]]
    return rel_err(out, reference(c)[0]) / tol
