"""fm_tune fd_hpb: at R <= 8 rows an attn_fd block computes 1, 2 or all (4) of a kv head's q heads.
A head's scores, softmax, PV, wave fold and split combine never meet another head's values, so the change claims
bit identity and every comparison here is array_equal on bit patterns: the per-op hook on attn_ref's poisoned
caches (every family, the positions of fd_positions, g = 4, 3, 2, 1 with a ragged last head group, 8- and 4-wave
blocks), shuffled slots of a two-layer cache with R = 1, 3 and 9 rows (past 8 rows the knob is inert), a repeated
launch on the larger ticket array, and whole frames of an S2-Pro-width model whose positions cross fd_min16.  The
all-heads result is additionally held to everything tests/test_gpu_attn_ops.py asks of a launch (the float64
reference's bound, the new row, every other cache word untouched, tickets 0, guard intact).
Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

import attn_ref as ar
from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_attn_ops import _check_decode, _decode
from test_gpu_llm import _cfg

pytestmark = pytest.mark.gpu

CAP, S = 32, 16 * 32 + 72
SHAPES = [(4, 1, 128), (6, 2, 128), (4, 2, 64), (2, 2, 32)]  # g = 4, 3 (groups of 2 + 1), 2, 1
HPB = (4, 1, 2)  # the first is the reference form: every q head of the kv head in one block


def _same_bits(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("out", "kc", "vc")):
        np.testing.assert_array_equal(ar.bits(x), ar.bits(y), err_msg=f"{what}: {name}")


def _clean(info):
    assert info["tickets"] == 0 and info["guard_ok"] == 1 and info["fd_nsp"] == ar.FD_NSP, info


def _cases(nh, nkv, hd, nwb, precision):
    """peaked at pos, pos - 1, 0 and a split's first row (those of peak_places), diffuse, large and tied, at every
    position of fd_positions: one split, a pass boundary and the row before it, cap +- 1, two splits, FD_NSP splits,
    a last split of a single row"""
    out = []
    for pos in ar.fd_positions(nwb, CAP, S):
        chunk = ar.fd_split(pos + 1, CAP)[1]
        for pk in (p for p in ar.peak_places(pos, nwb, CAP) if p in (0, chunk, pos - 1, pos)):
            out.append(ar.make_case("peaked", nh, nkv, hd, [pos], S, precision, peak=pk, seed=21))
        for fam in ("diffuse", "large", "tied"):
            out.append(ar.make_case(fam, nh, nkv, hd, [pos], S, precision, seed=21))
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("nwb", [8, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_heads_per_block_leave_every_bit(shape, nwb, precision, knob):
    """Output and both caches under fd_hpb 1 and 2 are the bits of fd_hpb 4; each launch leaves no ticket and an
    intact guard, and the fd_hpb 4 result passes test_gpu_attn_ops' checks of a launch (finite, inside the bound,
    row pos written, every other cache word -- NaN poison included -- unchanged)."""
    nh, nkv, hd = shape
    worst, splits = 0.0, set()
    for c in _cases(nh, nkv, hd, nwb, precision):
        res = {}
        for v in HPB:
            knob("fd_hpb", v)
            res[v] = _decode(c, "fd", nwb, CAP)
            info = res[v][3]
            assert (info["kernel"], info["nwb"], info["cap"]) == ("fd", nwb, CAP), info
            assert np.isfinite(res[v][0]).all(), (v, c["family"], c["pos"].tolist())
            _clean(info)
        worst = max(worst, _check_decode(c, res[4]))
        for v in HPB[1:]:
            _same_bits(res[4], res[v], f"fd_hpb {v} vs 4, {c['family']} pos {c['pos'].tolist()} peak {c['peak'].tolist()}")
        splits.add(ar.fd_split(int(c["pos"][0]) + 1, CAP)[0])
    assert {1, 2, ar.FD_NSP} <= splits
    print(f"\nfd_hpb {shape} nwb {nwb} {precision}: 1 = 2 = 4 bit for bit; worst rel err {worst:.3g} "
          f"(bound {ar.SLOW_TOL[precision]:.3g}); splits {sorted(splits)}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(4, 1, 128), (6, 2, 128)])
def test_heads_per_block_slots_and_repeats(shape, precision, knob):
    """R = 1, 3, 9 rows in shuffled, non-contiguous slots of a two-layer cache, read at layer 1: the same bits under
    the three values (9 rows: the knob is inert), and a second launch on the same, larger ticket array and the same
    partials repeats the first one's bits under each value."""
    assert {c["R"] for c in ar.slot_cases("fd8", precision, shape)} == {1, 3, 9}
    for c in ar.slot_cases("fd8", precision, shape):
        res = {}
        for v in HPB:
            knob("fd_hpb", v)
            res[v] = _decode(c, "fd", 8, CAP)
            two = _decode(c, "fd", 8, CAP, reps=2)
            _same_bits(res[v], two, f"fd_hpb {v}: second launch, R {c['R']}")
            _clean(res[v][3])
            _clean(two[3])
        _check_decode(c, res[4])
        for v in HPB[1:]:
            _same_bits(res[4], res[v], f"fd_hpb {v} vs 4, R {c['R']} {c['family']}")


def _wide():
    """S2-Pro widths at 2 slow + 1 fast layers (tests/golden/llm_wide), room for a 250-token prompt and 12 frames"""
    base = _cfg("llm_wide")
    cfg = dataclasses.replace(base, max_seq_len=320)
    cfg.im_end_id = base.im_end_id
    return cfg


def test_whole_frames_identical(knob):
    """A 250-token prompt, then frames at positions 250 .. 261: below fd_min16 (256) one split per kv head, past it
    two and their combine.  Teacher-forced slow and fast logits and emitted columns, and a sampled stream
    (temperature 0.8), eager and graph-replayed, are the same arrays under fd_hpb 1, 2 and 4."""
    from fishmi import native
    from fishmi.llm import DualARModel

    assert native.tune_get("fd_min16") == 256 and native.tune_get("fd_nw") == 8 and native.tune_get("attn_fd") == 1
    cfg = _wide()
    assert (cfg.n_layer, cfg.n_fast_layer, cfg.n_head, cfg.n_local_heads, cfg.head_dim) == (2, 1, 32, 8, 128)
    rng = np.random.default_rng(31)
    C1, T, NF = cfg.num_codebooks + 1, 250, 12
    prompt = np.zeros((C1, T), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, T)
    cols = np.zeros((C1, NF), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, NF)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, NF))
    greedy = DualARModel.sampling(top_k=1)
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=1234, mask_im_end=True)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    try:
        out = {}
        for v in HPB:
            knob("fd_hpb", v)
            for graph in (False, True):
                m.use_graph(graph)  # (re-)captured under the knob
                sl, fl, em = [], [], []
                try:
                    for k in range(NF):
                        m.force(0, cols[:, k])
                        em.append(m.prefill(0, prompt, greedy) if k == 0 else m.decode([0])[0])
                        s, f = m.read_logits(0)
                        sl.append(s)
                        fl.append(f)
                finally:
                    m.force(0, None)
                first = m.prefill(0, prompt, sp)
                stream = np.concatenate([first[None], m.decode_frames([0], NF)[:, 0]])
                out[v, graph] = (np.stack(sl), np.stack(fl), np.stack(em), stream)
        ref = out[4, False]
        # (masked slow logits are -inf by design) no NaN; a sampled stream, not one repeated code
        assert not np.isnan(ref[0]).any() and np.isfinite(ref[1]).all() and len(np.unique(ref[3][:, 1:])) > 8
        for key, got in out.items():
            for a, b, name in zip(ref, got, ("slow logits", "fast logits", "columns", "sampled stream")):
                np.testing.assert_array_equal(a, b, err_msg=f"(fd_hpb, graph) {key}: {name}")
    finally:
        m.use_graph(True)
        m.close()
