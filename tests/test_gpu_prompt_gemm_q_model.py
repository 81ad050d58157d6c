"""Weight-only int8 / int4 handles on the tiled prompt GEMMs (fm_tune prompt_gemm_q; linears of more than 64 rows),
model level, on test_gpu_prompt_q_model's layout (dim 512, 8 / 2 heads x 64, 2 + 2 layers, int4 groups of 128) with
max_seq_len raised to 256.  The code forms rebuild the bf16 copy's bits and keep mode 0's plan and epilogues (int8:
the row scales in whichever epilogue the plan runs), so every handle kind -- bf16 copy only, bf16 copy or codes of a
12-slot handle, compact -- must give the same bits; against the old routing (prompt_gemm_q 0: the 16-row tile kernel)
only the order of the fp32 sums differs, which is held to parity_util's bf16 bound with the handle's own fp32-mode run
as the truth.  Every test sets the knob itself.  Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

from parity_util import bf16_vs_reference, knob  # noqa: F401  (knob: fixture)
from test_gpu_fast_deadwork import _variant_cfg
from test_gpu_quant_compact import GS, NS, QUANTS, _batched, _equal, _forced, _tokens

pytestmark = pytest.mark.gpu


def _cfg():
    return dataclasses.replace(_variant_cfg("b"), max_seq_len=256)


def _open(cfg, quant, max_slots=1, compact=False, precision="bf16"):
    from fishmi.llm import DualARModel

    return DualARModel.synthetic(cfg, 11, 5, 0, precision, max_slots, quant=quant, groupsize=GS, compact=compact)


def _counts(m, prompt):
    """(quantised linears on the tiled route, code-streaming skinny launches) of one prefill"""
    from fishmi.llm import DualARModel

    m.profile(True)
    try:
        m.prefill(0, prompt, DualARModel.sampling(top_k=1))
        return m.profile_read("prompt_gq")[1], m.profile_read("prompt_q")[1]
    finally:
        m.profile(False)


@pytest.mark.parametrize("T", [65, 100, 200])
@pytest.mark.parametrize("quant", QUANTS)
def test_every_handle_kind_every_bit(quant, T, knob):
    """Teacher-forced prefill + 3 frames: (1) a 1-slot handle (no step-granular copy: mode 0 on the bf16 copy, int8
    with the row scales in the epilogues), (2) a 12-slot handle on its bf16 copy (knob 1), (3) the same handle on its
    codes (knob 2), (4) a compact handle -- equal slow logits, fast logits and columns.  The "prompt_gq" class counts
    the four linears of every slow layer on all of them under 1 and 2; under 0 on the compact handle alone, which
    ignores it; "prompt_q" (the skinny GEMM's class) stays 0 at these row counts."""
    cfg = _cfg()
    one, twelve, compact = _open(cfg, quant), _open(cfg, quant, 12), _open(cfg, quant, 1, True)
    hs = (one, twelve, compact)
    prompt, cols = _tokens(cfg, T, 4, 500 + T)
    sem = slice(cfg.semantic_begin_id, cfg.semantic_end_id + 1)
    n = 4 * cfg.n_layer
    try:
        knob("prompt_gemm_q", 1)
        base = _forced(one, prompt, cols)
        assert np.isfinite(base[1]).all() and np.isfinite(base[0][:, sem]).all()
        _equal(_forced(twelve, prompt, cols), base, f"{quant} T={T}: bf16 copy (12 slots)")
        _equal(_forced(compact, prompt, cols), base, f"{quant} T={T}: compact")
        assert [_counts(m, prompt) for m in hs] == [(n, 0)] * 3
        knob("prompt_gemm_q", 2)
        _equal(_forced(twelve, prompt, cols), base, f"{quant} T={T}: codes (12 slots)")
        _equal(_forced(one, prompt, cols), base, f"{quant} T={T}: 1 slot, no codes to prefer")
        assert [_counts(m, prompt) for m in hs] == [(n, 0)] * 3
        knob("prompt_gemm_q", 0)
        _equal(_forced(compact, prompt, cols), base, f"{quant} T={T}: compact ignores 0")
        assert [_counts(m, prompt) for m in hs] == [(0, 0), (0, 0), (n, 0)]
    finally:
        for m in hs:
            m.close()


@pytest.mark.parametrize("T", [100, 200])
def test_new_route_against_old_route(T, knob):
    """int8: the tiled route and the old routing differ by reordered fp32 sums only.  Truth: the same int8 model in
    fp32 compute; the tiled route's error against it is held to 1.5 x the old routing's own (RMS and max), with the
    argmax equal wherever the truth's top-2 margin exceeds twice the larger error (parity_util)."""
    cfg = _cfg()
    prompt, cols = _tokens(cfg, T, 4, 600 + T)
    f32, m = _open(cfg, "int8", precision="fp32"), _open(cfg, "int8", 12)
    try:
        ts, tf, _ = _forced(f32, prompt, cols)
        knob("prompt_gemm_q", 0)
        rs, rf, _ = _forced(m, prompt, cols)
        assert _counts(m, prompt) == (0, 0)
        knob("prompt_gemm_q", 1)
        slow, fast, _ = _forced(m, prompt, cols)
        assert _counts(m, prompt) == (4 * cfg.n_layer, 0)
        out = bf16_vs_reference(slow, fast, rs, rf, ts, tf)
        assert out["top1_checked"] > 0
    finally:
        f32.close()
        m.close()


def test_batched_prefill_138_rows(knob):
    """prefill_batch of 12 prompts of 6 .. 17 tokens (138 rows in ragged segments), then one batched frame, every slot
    teacher-forced: the compact int8 handle (its codes) equals the non-compact one (its bf16 copy), and both ran
    the four linears of every slow layer on the tiled route."""
    from fishmi.llm import DualARModel

    cfg = _cfg()
    ref, cmp_ = _open(cfg, "int8", NS), _open(cfg, "int8", NS, True)
    toks = [_tokens(cfg, 6 + s, 2, 40 + s) for s in range(NS)]
    prompts, cols = [t[0] for t in toks], [t[1] for t in toks]
    slots = list(range(NS))
    try:
        knob("prompt_gemm_q", 1)
        a = _batched(ref, cfg, prompts, cols)
        assert np.isfinite(a[1]).all()
        _equal(_batched(cmp_, cfg, prompts, cols), a, "138-row batched prefill: compact vs non-compact")
        for m in (ref, cmp_):
            m.profile(True)
            try:
                m.prefill_batch(slots, prompts, [DualARModel.sampling(top_k=1) for _ in slots])
                assert m.profile_read("prompt_gq")[1] == 4 * cfg.n_layer
            finally:
                m.profile(False)
    finally:
        ref.close()
        cmp_.close()


def test_decode_written_kv_rows_int8(knob):
    """test_gpu_engine.test_decode_written_kv_rows on the int8 handle at 80 positions: the K / V rows ten decode
    frames wrote after a 70-token prompt against the rows one 80-row prompt pass (the tiled route) writes -- at most
    1 % of the elements differ, by at most 2 bf16 ulps (that test's bound: the K order of the accumulation differs
    between the one-row kernels and any prompt GEMM)."""
    cfg = _cfg()
    T, n = 70, 11
    prompt, cols = _tokens(cfg, T, n, 800)
    m = _open(cfg, "int8", 12)
    sp = m.sampling(top_k=1)
    knob("prompt_gemm_q", 1)
    try:
        for i in range(n):
            m.force(0, cols[:, i])
            if i == 0:
                m.prefill(0, prompt, sp)
            else:
                m.decode([0])
        dec = [m.read_cache(l) for l in range(cfg.n_layer)]
        m.force(0, cols[:, n - 1])
        assert _counts(m, np.concatenate([prompt, cols[:, : n - 1]], axis=1)) == (4 * cfg.n_layer, 0)
        m.force(0, None)
        pro = [m.read_cache(l) for l in range(cfg.n_layer)]
    finally:
        m.close()
    d = [(x[:, T:T + n - 1], y[:, T:T + n - 1]) for a, b in zip(dec, pro) for x, y in zip(a, b)]
    cnt = sum(int((x != y).sum()) for x, y in d)
    ulp = max(int((np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64)) >> 16).max()) for x, y in d)
    tot = sum(x.size for x, _ in d)
    print(f"int8, tiled route: {cnt} of {tot} decode-written elements differ (max {ulp} ulp)")
    assert all(np.abs(x).max() > 0 for x, _ in d)
    assert cnt <= tot // 100 and ulp <= 2
