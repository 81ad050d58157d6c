"""Per-op tests of the decode samplers (sample_fast_kernel, sample_radix_kernel and their shared wide
path, top_k > 64) through fm_op_sample, against the numpy port of the oracle's orc_sample in
tests/sampler_ref.py.  Every launch has R = 4 rows with row_slot = [3, 1, 0, 2] and four slots of
different parameters, seeds and steps.  A decided draw (sampler_ref's decidedness test) must equal the
reference; an undecided one must lie in the union of the kept sets at the ends of its interval."""
import numpy as np
import pytest

import sampler_ref as sr
from parity_util import knob, tuned  # noqa: F401  (knob is a fixture)

pytestmark = pytest.mark.gpu

SENT = -12345                   # cols entries a row must not touch
TAP_SENT = np.float32(-777.25)  # tap entries a launch must not touch
PAD = 5                         # spare logits columns (ldl = Nl + PAD), filled with a value that would win if read
CONFIGS = {"fast_kth0": dict(sampler_fast=1, sampler_kth=0), "fast_kth1": dict(sampler_fast=1, sampler_kth=1),
           "radix": dict(sampler_fast=0, sampler_kth=1)}
PRECISIONS = ["bf16", "fp32"]
FAST_MAX = 4352                 # widest row of sample_fast_kernel


def run(L, prec):
    from fishmi import ops

    logits = np.full((4, L.Nl + PAD), 1e30, np.float32)
    logits[:, :L.Nl] = L.logits
    cols = np.full((4, sr.LDC), SENT, np.int32)
    tap = np.full((4, L.Nl + 3), TAP_SENT, np.float32)
    kid = ops.sample(logits, L.Nl, sr.ROW_SLOT, L.slots, cols, tap, L.slow, sr.SB, L.se, sr.IM_END, L.cb,
                     draw=sr.FAST_DRAW, col_idx=sr.FAST_COL, ras=L.ras, ras_enable=L.ras_enable,
                     force_cols=L.force_cols, precision=prec)
    return cols, tap, kid


def check(L, prec, cfg, out):
    cols, tap, kid = out
    bf16 = prec == "bf16"
    tag = (L.name, prec, cfg)
    assert kid == (1 if CONFIGS[cfg]["sampler_fast"] and L.Nl <= FAST_MAX else 0), tag
    written = (0, 1) if L.slow else (sr.FAST_COL,)
    untouched = [c for c in range(sr.LDC) if c not in written]
    assert (cols[:, untouched] == SENT).all(), (tag, cols)
    for r in range(4):
        slot = sr.ROW_SLOT[r]
        got = {c: int(cols[r, c]) for c in written}
        forced = bool(L.slots[slot]["force"])
        if forced:  # the tap row is the logits row bit for bit (its -0.0 too), the spare columns stay
            assert np.array_equal(tap[slot, :L.Nl].view(np.uint32), L.logits[r].view(np.uint32)), (tag, r)
            assert (tap[slot, L.Nl:] == TAP_SENT).all(), (tag, r)
        else:
            assert (tap[slot] == TAP_SENT).all(), (tag, r)
        if not L.compare[r]:  # NaN rows: any value in range
            if L.slow:
                assert sr.SB <= got[0] <= L.se or got[0] == sr.IM_END, (tag, r, got)
                assert 0 <= got[1] < L.cb, (tag, r, got)
            else:
                assert 0 <= got[sr.FAST_COL] < L.cb, (tag, r, got)
            continue
        want, decided, allowed = L.expect(r, bf16)
        if decided:
            assert got == want, (tag, r, L.slots[slot], got, want)
        else:
            assert got[written[0]] in allowed, (tag, r, got, sorted(allowed))
            if L.slow:
                assert got[1] == L.code(got[0]), (tag, r, got)


def run_family(launches, cfg, prec):
    with tuned(**CONFIGS[cfg]):
        for L in launches:
            check(L, prec, cfg, run(L, prec))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("family", [f for f in sr.FAMILIES if f != "wave_overflow"])
def test_family(family, cfg, prec):
    """lengths (row widths 1 .. 8192 around every threshold, top_k 0 .. Nl + 7; 4353 and 8192 are radix by
    width, checked through the returned kernel id), ties at the K-th rank, massive ties, rows with few
    finite entries, signed zeros, peaked and flat rows, RAS, forcing and NaN rows: sampler_ref's
    docstrings say what each launch is built to reach"""
    run_family(sr.FAMILIES[family](), cfg, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_wave_overflow(cfg, prec):
    """100 equal row maxima sit in columns tid + 256 i with tid < 64, which are all values of wave 0 of
    sample_fast_kernel.  That wave's threshold is the maximum's key, 100 of its keys reach it, and 100 >
    SF_CAP = 64 candidates per wave, so the block must flag the overflow and take wave 0's exact scan:
    with top_k 30 the 30 lowest ids of the 100 are kept (the radix kernel reaches the same rows through
    its tie list)."""
    run_family(sr.wave_overflow(), cfg, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("path", ["narrow", "wide"])
def test_random_rows(path, cfg, prec):
    run_family(sr.random_launches(path), cfg, prec)


def _sample_of_launches():
    return (sr.kth_ties() + sr.wave_overflow() + sr.massive_ties() + sr.signed_zeros() + sr.ras() +
            sr.random_launches("narrow")[:6] + sr.random_launches("wide")[:6])


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_repeatable(cfg, prec):
    """the same launch three times gives the same cols"""
    with tuned(**CONFIGS[cfg]):
        for L in _sample_of_launches():
            first = run(L, prec)[0]
            for _ in range(2):
                assert np.array_equal(run(L, prec)[0], first), (L.name, cfg, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_fast_equals_radix_on_decided_rows(prec):
    launches = [L for make in sr.FAMILIES.values() for L in make()] + sr.random_all()
    with tuned(**CONFIGS["fast_kth1"]):
        fast = [run(L, prec)[0] for L in launches]
    with tuned(**CONFIGS["radix"]):
        radix = [run(L, prec)[0] for L in launches]
    n = 0
    for L, f, x in zip(launches, fast, radix):
        for r in range(4):
            if L.compare[r] and L.expect(r, prec == "bf16")[1]:
                assert np.array_equal(f[r], x[r]), (L.name, prec, r, f[r], x[r])
                n += 1
    assert n > 500


def test_refuses_a_row_too_wide_for_lds():
    """16385 columns need a 32768-entry sort (256 KiB of keys): an error return, not an abort"""
    from fishmi import native

    L = sr.Launch("wide", False, np.zeros((4, 16385), np.float32), sr.slot_table(30))
    with pytest.raises(native.FishMIError):
        run(L, "bf16")
