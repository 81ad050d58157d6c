"""CPU checks of tests/sampler_ref.py, the reference of the sampler's per-op GPU tests: the numpy port
equals the C oracle's orc_sample on every launch the GPU tests use, and the launches are decided
often enough for those tests to mean something (conditions on the inputs: a launch that breaks a cap
is changed, never the cap)."""
import numpy as np
import pytest

import sampler_ref as sr

PRECISIONS = [("bf16", True), ("fp32", False)]


def _oracle():
    import oracle as orc

    return orc


def _all_launches():
    return [(fam, L) for fam, make in sr.FAMILIES.items() for L in make()] + [("random", L) for L in sr.random_all()]


@pytest.mark.parametrize("prec,bf16", PRECISIONS)
def test_port_equals_c_oracle(prec, bf16):
    orc = _oracle()
    n = 0
    for fam, L in _all_launches():
        for r in range(4):
            if not L.compare[r] or L.slots[sr.ROW_SLOT[r]]["force"]:
                continue
            row = L.oracle_row(r)
            for (t, p, k, seed, step, d) in L.draws(r, bf16):
                want = orc.sample(row, t, p, k, seed, step, d, bf16=bf16)
                got = sr.draw(row, t, p, k, bf16, seed, step, d).token
                assert got == want, (L.name, r, d, got, want)
                n += 1
    print(f"{prec}: {n} draws equal orc_sample")
    assert n > 500


def test_rng_and_rounding_match_oracle_probs():
    """orc_logits_to_probs's kept set through the port's eyes: the ids with a non-zero probability are
    ids the port keeps (bf16, a few launches)"""
    orc = _oracle()
    for L in sr.kth_ties() + sr.signed_zeros():
        for r in range(4):
            sp = L.slots[sr.ROW_SLOT[r]]
            row = L.oracle_row(r)
            probs = orc.logits_to_probs(row, sp["temperature"], sp["top_p"], sp["top_k"], bf16=True)
            d = sr.draw(row, sp["temperature"], sp["top_p"], sp["top_k"], True, sp["seed"], sp["step"], 0)
            assert d.token in set(np.flatnonzero(probs > 0).tolist())


@pytest.mark.parametrize("prec,bf16", PRECISIONS)
def test_random_launches_mostly_decided(prec, bf16):
    ls = sr.random_all()
    und = [(L.name, r) for L in ls for r in range(4) if not L.expect(r, bf16)[1]]
    total = 4 * len(ls)
    print(f"{prec}: {len(und)} of {total} random draws undecided {und}")
    assert total >= 100 and len(und) <= 0.02 * total


@pytest.mark.parametrize("family", [f for f in sr.FAMILIES if f != "nan_rows"])
def test_family_decided(family):
    """every handcrafted row is decided in bf16, and in fp32 unless its family marks it fragile"""
    und32 = []
    for L in sr.FAMILIES[family]():
        for r in range(4):
            assert L.expect(r, True)[1], (L.name, r, "bf16 undecided")
            if not L.expect(r, False)[1]:
                und32.append((L.name, r))
                assert r in L.fragile, (L.name, r, "fp32 undecided and not marked fragile")
    print(f"{family}: fp32 undecided (marked fragile) {und32}")


def test_nan_rows_ordinary_rows_decided():
    for L in sr.nan_rows():
        for r in (2, 3):
            assert L.expect(r, True)[1] and L.expect(r, False)[1], (L.name, r)


def test_signed_zero_rows_expect_the_lower_id():
    """the issue's row: maximum -0.0 at column 2, +0.0 at column 5, top_k 1 -> column 2"""
    for L in sr.signed_zeros():
        if "top1" not in L.name:
            continue
        for r in range(3):
            cols, decided, _ = L.expect(r, True)
            assert decided and cols[min(cols)] == (sr.SB + 2 if L.slow else 2), (L.name, r, cols)


def test_ras_launches_redraw():
    """in the RAS launches the first draw is in the window (so the expected token is the second draw),
    except in the controls"""
    for L in sr.ras():
        for r in range(4):
            for bf16 in (True, False):
                d0 = sr.draw(L.oracle_row(r), *L.draws(r, bf16)[0][:3], bf16, *L.draws(r, bf16)[0][3:])
                inwin = d0.token in set(L.ras[sr.ROW_SLOT[r]].tolist())
                if L.name.endswith("_im_end"):
                    assert d0.token == sr.IM_END and inwin and L.expect(r, bf16)[0][0] == sr.IM_END
                else:
                    assert inwin and sr.SB <= d0.token <= L.se
                    d1 = sr.draw(L.oracle_row(r), *L.draws(r, bf16)[1][:3], bf16, *L.draws(r, bf16)[1][3:])
                    assert L.expect(r, bf16)[0][0] == (d1.token if L.ras_enable else d0.token)
