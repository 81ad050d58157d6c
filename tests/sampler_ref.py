"""Reference for the decode sampler's per-op tests: a numpy port of the oracle's orc_logits_to_probs +
orc_sample (oracle/fishmi_oracle.c) with a decidedness test, and the launches (logit rows + per-slot
parameters) that tests/test_sampler_ref.py checks on the CPU and tests/test_gpu_sampler_ops.py runs
through fm_op_sample.

The port works on an oracle row indexed by token id.  A fast-head row is its own oracle row (column
i is code i).  A slow-head row of Nl columns is scattered to ids SB .. SB + Nl - 2 and IM_END, -inf
elsewhere: IM_END < SB, so im_end comes first in id order although it is the last column, which is
the order the kernels' tok_of implies.

Decidedness.  The kernels' expf / logf, their fp32 division and the block-order sums behind `den`
and `d2` differ from libm and from the oracle's sequential sums by a few fp32 ulps, so a draw whose
outcome hangs on the last bits has no single right answer.  Every draw is therefore evaluated at
both ends of an interval around the oracle's values (and at the oracle's values themselves):
  * the oracle adds den and d2 one term at a time in fp32.  The port also adds the same terms in
    float64, which is exact to 2^-53, so it knows the oracle's own summation error exactly.
  * a kernel adds them as a tree: at most 32 terms per thread, 6 wave steps and 4 waves.  A sum of
    non-negative fp32 terms added along a tree of depth d is within d * 2^-24 (relative) of the exact
    sum, here d <= 42.  expf, logf and the division are good to about an ulp (2^-24) each; 22 ulps
    are left to them.  So E = 64 * 2^-24 = 2^-18 around the exact sum covers a kernel.
  * den and d2 therefore range over the hull of {the oracle's fp32 sum, exact sum * (1 -+ E)}, and
    -log(u) over its fp32 value * (1 -+ E).
  (A fixed 2^-20 around the oracle's sum would not do: the one-by-one sum's own error bound is 2^-12 at
  4097 finite logits, and its random-walk estimate sqrt(n) * 2^-25 = 2^-19 is already past 2^-20.)
  All roundings and fp32 additions are monotone, so the values a kernel may legitimately compute lie
  between the two end evaluations.
A draw is decided when (a) the kept prefix (top-k / top-p) has the same length at both ends, and (b)
the winner's lowest score beats every other kept candidate's highest score, or the two tie in a way
no implementation can break: the same scaled logit and the same uniform (identical inputs give
identical scores), or both score intervals collapsed to the same single value (bf16 rounding); such
ties go to the lower id, as in orc_sample.  An undecided draw may give any id kept at either end.
At f = 1 the port reproduces orc_sample (tests/test_sampler_ref.py holds it to that on every launch).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

SB, IM_END = 16, 5          # synthetic vocabulary of the slow head: semantic ids start at SB, im_end below them
ROW_SLOT = (3, 1, 0, 2)     # row r of every launch samples with slot ROW_SLOT[r]
LDC, FAST_COL, FAST_DRAW = 10, 3, 3
F32 = np.float32
NINF = F32(-np.inf)


def bf16r(x):
    """round-to-nearest-even to bf16 (the oracle's bf16r), float32 in / out"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    r = np.where(nan, (u | np.uint32(0x00400000)) & np.uint32(0xFFFF0000), r)
    return r.astype(np.uint32).view(F32)


_M64 = (1 << 64) - 1


def rng_uniform_bf16(seed, step, draw, ids):
    """the sampler's counter RNG: splitmix64 (without the initial add) of the key, 24 mantissa bits,
    truncated to bf16"""
    base = (seed * 0xD1B54A32D192ED03 + (step * 64 + draw) * 0x9E3779B97F4A7C15) & _M64
    with np.errstate(over="ignore"):
        z = np.uint64(base) + np.asarray(ids, np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    m = (z >> np.uint64(40)).astype(np.uint32)
    u = m.astype(F32) * F32(1.0 / 16777216.0)
    return (u.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def _exp(x):
    with np.errstate(invalid="ignore"):
        return np.exp(x.astype(np.float64)).astype(F32)


def _seqsum(x):
    return np.cumsum(x, dtype=F32)[-1] if x.size else F32(0)


E = 64 * 2.0 ** -24


def _hull(terms, total):
    """(low, 1, high) factors on the oracle's fp32 sum `total` of `terms` that span it and the exact sum
    * (1 -+ E)"""
    ratio = float(terms.astype(np.float64).sum()) / float(total)
    return min(1.0, ratio * (1 - E)), 1.0, max(1.0, ratio * (1 + E))


def _scale(x, f):
    return (np.asarray(x, np.float64) * f).astype(F32)


@dataclass(frozen=True)
class Draw:
    token: int          # orc_sample's answer (f = 1)
    decided: bool
    allowed: frozenset  # ids an implementation may return when the draw is undecided (else {token})


def draw(lg, temperature, top_p, top_k, bf16, seed, step, drw):
    """one orc_sample on the id-indexed row lg (no NaN), with the decidedness test"""
    lg = np.ascontiguousarray(lg, F32)
    n = lg.size
    rb = bf16r if bf16 else (lambda v: np.asarray(v, F32))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        order = np.argsort(-lg, kind="stable")  # value desc, ties by id (kv_cmp; -0.0 == +0.0)
        sv = lg[order]
        t, p = rb(F32(temperature)), rb(F32(top_p))
        e = np.where(sv == NINF, F32(0), _exp(sv - sv[0]))
        den = _seqsum(e)
        rank_ok = np.arange(n) < top_k
        keeps = []
        for f in _hull(e, den):
            pr = rb(e / _scale(den, f))
            cr = rb(np.cumsum(pr, dtype=F32))
            k = ~(cr > p) & rank_ok
            k[0] = True
            km = np.zeros(n, bool)
            km[order[k]] = True
            keeps.append(km)
        k_lo, keep, k_hi = keeps  # f < 1: larger probabilities, shorter prefix
        tt = max(t, F32(1e-5))
        l = np.where(keep, rb(lg / tt), NINF)
        m2 = l.max()
        e2 = np.where(l == NINF, F32(0), _exp(l - m2))
        d2 = _seqsum(e2)
        ids = np.arange(n)
        u = rng_uniform_bf16(seed, step, drw, ids)
        q = (-np.log(u.astype(np.float64))).astype(F32)
        sc = []
        for f, g in zip(_hull(e2, d2)[::-1], (1 + E, 1.0, 1 - E)):  # lowest, oracle, highest score
            prob = np.where(l == NINF, F32(0), rb(e2 / _scale(d2, f)))
            sc.append((prob, rb(prob / rb(_scale(q, g)))))
        (_, lo), (prob, mid), (_, hi) = sc
    cand = keep & (prob > 0)
    w = int(np.argmax(np.where(cand, mid, F32(-1))))  # first maximum: the lowest id
    others = keep.copy()
    others[w] = False
    structural = (l == l[w]) & (u == u[w])
    collapsed = (lo == hi) & (lo == lo[w]) & (hi == hi[w])
    beaten = (hi < lo[w]) | ((structural | collapsed) & (ids > w))
    decided = bool(np.array_equal(k_lo, k_hi) and beaten[others].all())
    allowed = frozenset([w]) if decided else frozenset(np.flatnonzero(k_lo | k_hi | keep).tolist())
    return Draw(w, decided, allowed)


# ---- launches ------------------------------------------------------------------------------------
@dataclass
class Launch:
    name: str
    slow: bool
    logits: np.ndarray            # [4][Nl] float32
    slots: list                   # 4 dicts: temperature, top_p, top_k, mask_im_end, seed, step, force
    ras: np.ndarray = None        # [4][10] int32
    ras_enable: bool = False
    force_cols: np.ndarray = None
    fragile: frozenset = frozenset()   # rows whose fp32 draw may be undecided (see the family)
    compare: tuple = (True, True, True, True)  # rows compared with the oracle (NaN rows are not)
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def Nl(self):
        return self.logits.shape[1]

    @property
    def se(self):
        return SB + self.Nl - 2

    @property
    def cb(self):
        return max(self.Nl - 1, 1) if self.slow else self.Nl

    def oracle_row(self, r):
        """row r in token-id order, as the oracle sees it"""
        row, sp = self.logits[r], self.slots[ROW_SLOT[r]]
        if not self.slow:
            return row.copy()
        o = np.full(SB + self.Nl - 1, NINF, F32)
        o[SB:SB + self.Nl - 1] = row[:-1]
        o[IM_END] = NINF if sp["mask_im_end"] else row[-1]
        return o

    def draws(self, r, bf16):
        """the orc_sample calls row r makes: [(temperature, top_p, top_k, seed, step, draw)]"""
        sp = self.slots[ROW_SLOT[r]]
        first = (sp["temperature"], sp["top_p"], sp["top_k"], sp["seed"], sp["step"], 0 if self.slow else FAST_DRAW)
        return [first, (1.0, 0.9, sp["top_k"], sp["seed"], sp["step"], 1)] if self.slow else [first]

    def expect(self, r, bf16):
        """(cols the row must write {index: value}, decided, allowed values of the first of them)"""
        key = (r, bool(bf16))
        if key not in self._cache:
            self._cache[key] = self._expect(r, bf16)
        return self._cache[key]

    def _expect(self, r, bf16):
        slot = ROW_SLOT[r]
        sp = self.slots[slot]
        if sp["force"]:
            fc = self.force_cols[slot]
            out = {0: int(fc[0]), 1: int(fc[1])} if self.slow else {FAST_COL: int(fc[FAST_COL])}
            return out, True, frozenset([out[min(out)]])
        row = self.oracle_row(r)
        ds = [draw(row, t, p, k, bf16, seed, step, d) for (t, p, k, seed, step, d) in self.draws(r, bf16)]
        if not self.slow:
            d0 = ds[0]
            return {FAST_COL: d0.token}, d0.decided, d0.allowed
        d0, d1 = ds
        win = set(self.ras[slot].tolist()) if (self.ras_enable and self.ras is not None) else set()

        def redrawn(tok):
            return tok in win and SB <= tok <= self.se

        tok = d1.token if redrawn(d0.token) else d0.token
        decided = d0.decided and (d1.decided or not redrawn(d0.token))
        allowed = set()
        for t0 in d0.allowed:
            allowed |= set(d1.allowed) if redrawn(t0) else {t0}
        return {0: tok, 1: self.code(tok)}, decided, frozenset(allowed)

    def code(self, tok):
        return int(min(max(tok - SB, 0), self.cb - 1))


def slot_table(top_k, temperature=(0.7, 1.0, 1.3, 0.1), top_p=(0.9, 0.5, 0.99, 0.9), seed0=1000, step0=3, mask=0):
    """four slots with different seeds and steps, so a slot / row mix-up changes the draws"""
    bc = lambda v: v if isinstance(v, (tuple, list)) else (v,) * 4  # noqa: E731
    return [dict(temperature=float(bc(temperature)[i]), top_p=float(bc(top_p)[i]), top_k=int(bc(top_k)[i]),
                 mask_im_end=int(bc(mask)[i]), seed=int(seed0 + 77 * i), step=int(step0 + 5 * i), force=0)
            for i in range(4)]


def _normal(rng, Nl, sigma):
    return (rng.standard_normal((4, Nl)) * sigma).astype(F32)


LENGTHS = (1, 5, 63, 64, 65, 255, 257, 4096, 4097, 4352, 4353, 8192)


@functools.lru_cache(None)
def lengths():
    """every row length around a wave, the candidate cap, the tie list and the fast kernel's width, with
    top_k in {0, 1, 2, 63, 64, 65, 100, Nl, Nl + 7} (K > Nl included); 4353 and 8192 are radix by width"""
    rng = np.random.default_rng(100)
    out = []
    for Nl in LENGTHS:
        for j, ks in enumerate(((0, 1, 2, 63), (64, 65, 100, Nl), (Nl + 7, 30, 100, 64))):
            slow = (j + Nl) % 2 == 0 if Nl > 4097 else None
            for s in ((True, False) if slow is None else (slow,)):
                out.append(Launch(f"len{Nl}_k{j}_{'slow' if s else 'fast'}", s, _normal(rng, Nl, 3.0),
                                  slot_table(ks, seed0=2000 + Nl, step0=j)))
    return out


def _tie_rows(rng, Nl, ks, leader):
    rows = np.minimum(_normal(rng, Nl, 1.0), F32(2.5)) + F32(0.5)
    for r in range(4):
        K = ks[ROW_SLOT[r]]
        free = rng.permutation(Nl - 1)
        tie, above = [Nl - 1, int(free[0]), int(free[1])], free[2:K]
        rows[r, above] = F32(5.0) + F32(0.01) * np.arange(1, K - 1, dtype=F32)
        rows[r, tie] = F32(5.0)
        if leader:
            rows[r, above[0]] = F32(8.0)
    return rows


@functools.lru_cache(None)
def kth_ties():
    """three equal values straddle rank K at scattered columns (the last one, im_end on the slow head,
    among them): two are taken, by the lower id.  The K - 2 values above them are barely larger and the
    rest of the row carries half the mass, so the tied entries are drawn often and top-p never cuts.
    The `leader` launches give rank 0 a clear lead and draw at temperature 0.1: rank 0 must come out
    whatever the tie pick does at rank K - 1 (top_k 64 fills the candidate arrays to their last entry)."""
    rng = np.random.default_rng(12)
    out = []
    for Nl in (300, 1100):
        for slow in (True, False):
            ks = (2, 30, 64, 100)
            out.append(Launch(f"kth_tie{Nl}_{'slow' if slow else 'fast'}", slow, _tie_rows(rng, Nl, ks, False),
                              slot_table(ks, temperature=(1.0, 1.3, 1.0, 1.3), top_p=0.99, seed0=31 + Nl)))
            ks = (64, 63, 64, 30)
            out.append(Launch(f"kth_tie_leader{Nl}_{'slow' if slow else 'fast'}", slow, _tie_rows(rng, Nl, ks, True),
                              slot_table(ks, temperature=0.1, top_p=0.99, seed0=32 + Nl)))
    return out


@functools.lru_cache(None)
def wave_overflow():
    """100 equal maxima in columns tid + 256 i with tid < 64: all of them are values of wave 0 of the fast
    kernel, so that wave counts 100 candidates >= its threshold (the maximum itself), more than SF_CAP =
    64, and the block takes the overflow scan; top_k 30 keeps the 30 lowest ids"""
    rng = np.random.default_rng(13)
    out = []
    for slow, Nl in ((True, 4097), (False, 4096), (False, 1500)):
        rows = _normal(rng, Nl, 1.0) - F32(4.0)
        for r in range(4):
            cols = np.array([t + 256 * i for t in range(64) for i in range(17) if t + 256 * i < Nl - 1])
            rows[r, rng.choice(cols, 100, replace=False)] = F32(1.5)
        out.append(Launch(f"overflow{Nl}_{'slow' if slow else 'fast'}", slow, rows,
                          slot_table((30, 30, 64, 30), temperature=(1.0, 1.3, 0.7, 1.0), top_p=(0.9, 0.99, 0.9, 0.5),
                                     seed0=77)))
    return out


@functools.lru_cache(None)
def massive_ties():
    """a 600-way tie at the top of a 1024-wide row and all-equal rows of 4097 / 4096: radix's nt > 256 scan
    and fast's overflow scan at top_k 30 / 64, the sort's stability at top_k 100"""
    rng = np.random.default_rng(14)
    out = []
    for slow in (True, False):
        rows = _normal(rng, 1024, 1.0) - F32(6.0)
        for r in range(4):
            rows[r, rng.choice(1024, 600, replace=False)] = F32(0.25)
        out.append(Launch(f"tie600_{'slow' if slow else 'fast'}", slow, rows,
                          slot_table((30, 64, 100, 30), top_p=(0.9, 0.5, 0.9, 0.5), seed0=5)))
        Nl = 4097 if slow else 4096
        out.append(Launch(f"equal{Nl}", slow, np.full((4, Nl), F32(-1.75)),
                          slot_table((30, 64, 100, 64), top_p=(0.9, 0.5, 0.9, 0.5), seed0=6)))
    return out


@functools.lru_cache(None)
def few_finite():
    """-inf everywhere but 1 or 2 columns (top_k 30 and 100 reach into the -inf entries), and im_end
    holding the maximum while mask_im_end = 1"""
    out = []
    for slow in (True, False):
        rows = np.full((4, 257), NINF)
        rows[0, 100] = 1.0
        rows[1, [3, 256]] = (0.5, 0.75)
        rows[2, 256] = -2.0
        rows[3, [64, 65]] = (2.0, 2.0)
        out.append(Launch(f"few_finite_{'slow' if slow else 'fast'}", slow, rows,
                          slot_table((30, 100, 100, 30), temperature=1.0, top_p=0.99, seed0=8)))
    rows = np.random.default_rng(15).standard_normal((4, 300)).astype(F32)
    rows[:, 299] = 9.0  # im_end far ahead, masked in slots 0 and 2
    out.append(Launch("masked_im_end", True, rows, slot_table((30, 100, 100, 30), mask=(1, 0, 1, 0), seed0=9)))
    rows = np.full((4, 70), NINF)
    rows[:, 69] = 3.0
    rows[:, 11] = 1.0
    out.append(Launch("masked_im_end_one_left", True, rows, slot_table((30, 100, 1, 64), mask=1, seed0=10)))
    return out


@functools.lru_cache(None)
def signed_zeros():
    """-0.0 and +0.0 are one value to the oracle (kv_cmp compares floats), so the lower id ranks first:
    the row maximum -0.0 at column 2 and +0.0 at column 5 with top_k 1 gives column 2; and with the
    probabilities 0.6 / 0.2 / 0.2 at columns 9 / 3 (-0.0) / 7 (+0.0) and top_p 0.9, column 3 is kept and
    column 7 is cut"""
    out = []
    for slow in (True, False):
        rows = np.full((4, 40), F32(-3.0))
        rows[:, 2], rows[:, 5] = F32(-0.0), F32(0.0)
        rows[1, 2], rows[1, 5] = F32(0.0), F32(-0.0)
        out.append(Launch(f"zeros_top1_{'slow' if slow else 'fast'}", slow, rows,
                          slot_table((1, 1, 1, 100), top_p=(0.9, 0.9, 0.9, 1e-3), seed0=21)))
        for j in range(3):
            rows = np.full((4, 40), NINF)
            rows[:, 9], rows[:, 3], rows[:, 7] = F32(np.log(3.0)), F32(-0.0), F32(0.0)
            out.append(Launch(f"zeros_top_p{j}_{'slow' if slow else 'fast'}", slow, rows,
                              slot_table((30, 100, 3, 64), temperature=1.3, top_p=0.9, seed0=22 + j, step0=j)))
    return out


@functools.lru_cache(None)
def peaked_flat():
    """one dominant logit and a nearly flat row, at temperature 0.0 (clamped to 1e-5), 0.1, 1.3 and top_p
    0.5 / 0.9 / 0.99 / 1.0.  fp32 rows of the peaked launch are fragile: the leader's probability
    rounds to 1.0 and the tail's running sum sits on top_p = 1.0 itself."""
    rng = np.random.default_rng(16)
    out = []
    for slow in (True, False):
        for kind in ("peaked", "flat"):
            rows = _normal(rng, 300, 1.0 if kind == "peaked" else 0.01)
            if kind == "peaked":
                rows[np.arange(4), rng.choice(299, 4)] = 20.0
            for j, ks in enumerate(((30, 100, 30, 100), (100, 30, 64, 2))):
                out.append(Launch(f"{kind}{j}_{'slow' if slow else 'fast'}", slow, rows,
                                  slot_table(ks, temperature=((0.0, 0.1, 1.3, 0.0), (1.3, 0.0, 0.1, 1.3))[j],
                                             top_p=((0.5, 0.9, 0.99, 1.0), (1.0, 0.99, 0.5, 0.9))[j], seed0=40 + j),
                                  fragile=frozenset(range(4)) if kind == "peaked" else frozenset()))
    return out


@functools.lru_cache(None)
def ras():
    """slow head, ras_enable: the first draw's token (of either precision) sits in the slot's window, so
    the second draw (temperature 1.0, top_p 0.9, draw 1) is emitted; narrow and wide path.  Controls:
    im_end in the window is not replaced (rows built so that im_end wins), and with ras_enable = 0
    nothing is replaced."""
    rng = np.random.default_rng(100)
    out = []
    for ks in ((30, 30, 64, 2), (100, 100, 65, 5000)):
        rows = _normal(rng, 500, 2.0)
        base = Launch("ras_base", True, rows, slot_table(ks, seed0=50 + ks[0]))
        win = np.full((4, 10), -1, np.int32)
        for r in range(4):
            toks = sorted({base.expect(r, b)[0][0] for b in (True, False)})
            win[ROW_SLOT[r], 3:3 + len(toks)] = toks
        for en in (True, False):
            out.append(Launch(f"ras_k{ks[0]}_{'on' if en else 'off'}", True, rows, slot_table(ks, seed0=50 + ks[0]),
                              ras=win, ras_enable=en))
        rows = rows.copy()
        rows[:, -1] = 12.0
        win = np.full((4, 10), -1, np.int32)
        win[:, 7] = IM_END
        out.append(Launch(f"ras_k{ks[0]}_im_end", True, rows, slot_table(ks, seed0=50 + ks[0]), ras=win, ras_enable=True))
    return out


@functools.lru_cache(None)
def forcing():
    """slot 1 (row 1) is teacher-forced: it emits force_cols and taps its logits row, -0.0 included; the
    other rows of the launch sample normally"""
    rng = np.random.default_rng(18)
    out = []
    for slow, ks in ((True, 30), (False, 30), (True, 100), (False, 100)):
        rows = _normal(rng, 321, 2.0)
        rows[:, 17] = F32(-0.0)
        slots = slot_table(ks, seed0=60)
        slots[1]["force"] = 1
        fc = np.arange(4 * LDC, dtype=np.int32).reshape(4, LDC) + 100
        out.append(Launch(f"force_k{ks}_{'slow' if slow else 'fast'}", slow, rows, slots, force_cols=fc))
    return out


@functools.lru_cache(None)
def nan_rows():
    """row 0 holds one quiet NaN, row 1 is all NaN (not compared with the oracle: the emitted value must
    only be in range); rows 2 and 3 of the same launch are ordinary"""
    rng = np.random.default_rng(19)
    out = []
    for slow in (True, False):
        for Nl in (50, 700):
            for ks in ((30, 1, 64, 2), (100, 100, 65, 5000)):
                rows = _normal(rng, Nl, 2.0)
                rows[0, Nl // 3] = np.nan
                rows[1, :] = np.nan
                out.append(Launch(f"nan{Nl}_k{ks[0]}_{'slow' if slow else 'fast'}", slow, rows, slot_table(ks, seed0=70),
                                  compare=(False, False, True, True)))
    return out


RANDOM_TOPK = {"narrow": (1, 2, 30, 63, 64), "wide": (65, 100, 5000)}


@functools.lru_cache(None)
def random_launches(path, n=15, seed=2024):
    """n launches (4 n draws) per path: N(0, sigma) rows, sigma in {0.3, 3, 8}, the lengths, top_p and
    temperatures of the oracle's own sampling range"""
    rng = np.random.default_rng(seed + len(path))
    out = []
    for i in range(n):
        Nl = int(rng.choice((5, 63, 64, 65, 257, 1024, 4097)))
        slow = bool(rng.integers(2)) or Nl == 4097
        pick = lambda vals: tuple(vals[j] for j in rng.integers(len(vals), size=4))  # noqa: E731
        out.append(Launch(f"rand_{path}{i}", slow, _normal(rng, Nl, float(rng.choice((0.3, 3.0, 8.0)))),
                          slot_table(pick(RANDOM_TOPK[path]), temperature=pick((0.1, 0.7, 1.0, 1.3)),
                                     top_p=pick((0.5, 0.9, 0.99)), seed0=int(rng.integers(1 << 40)),
                                     step0=int(rng.integers(1000)))))
    return out


def random_all():
    return random_launches("narrow") + random_launches("wide")


FAMILIES = {"lengths": lengths, "kth_ties": kth_ties, "wave_overflow": wave_overflow, "massive_ties": massive_ties,
            "few_finite": few_finite, "signed_zeros": signed_zeros, "peaked_flat": peaked_flat, "ras": ras,
            "forcing": forcing, "nan_rows": nan_rows}
