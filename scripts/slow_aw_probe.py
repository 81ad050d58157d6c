"""Timeline of the fused slow attention + wo launch (fm_rowgemv.hip slow_attn_wo_kernel) from its debug_ts records,
beside scripts/fw_probe.py for the fast one: attention blocks (0xFFFC: start, rows ready, passes done, folded,
output or partial stored; 0xFFFB: the combiner's end) and the wo groups' first waves (0xFFF8: start, weights issued,
x words current, dot products done, end; aux = full reads of x | one-word polls << 16), per launch, relative to the launch's first block start
(us), at several context lengths.

usage: [QUANT=int8|int4] python scripts/slow_aw_probe.py [slow_attn_wo value, default 2] [context ...  default 64 180 280 600]
(QUANT: a weight-only handle, the value is slow_attn_wo_q's, GROUPSIZE default 128; the wait knobs slow_aw_cheap / slow_aw_delay / slow_aw_sleep as in force: their defaults, or FISHMI_TUNE's)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

KNOB = int(sys.argv[1]) if len(sys.argv) > 1 else 2
CTX = [int(a) for a in sys.argv[2:]] or [64, 180, 280, 600]
cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
QUANT = os.environ.get("QUANT") or None
KEY = "slow_attn_wo_q" if QUANT else "slow_attn_wo"
native.tune(KEY, KNOB)
print(f"fm_tune {KEY} {KNOB}" + (f" (weight-only {QUANT})" if QUANT else ""))
m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=1, quant=QUANT,
                          groupsize=int(os.environ.get("GROUPSIZE", "128")))
names = ["att rows ready(max)", "att passes done(max)", "att stored(max)", "wo last start", "wo weights issued",
         "wo x current", "wo x current(max)", "wo dots done", "wo end(mean)", "wo end(max)", "wo reads of x",
         "wo reads of x(max)", "wo one-word polls", "wo one-word polls(max)"]
for ctx in CTX:
    p = np.zeros((cfg.num_codebooks + 1, ctx - 8), np.int32)
    p[0] = np.random.default_rng(1).integers(16, cfg.semantic_begin_id, ctx - 8)
    m.use_graph(True)
    m.prefill(0, p, DualARModel.sampling(mask_im_end=True))
    m.decode_frames([0], 8)
    m.use_graph(False)
    native.tune("debug_ts", 1)
    m.decode_frames([0], 2)
    rec = native.debug_ts_read().astype(np.int64)
    native.tune("debug_ts", 0)
    tag = rec[:, 0] >> 32
    att, comb, wo = rec[tag == 0xFFFC], rec[tag == 0xFFFB], rec[tag == 0xFFF8]
    att = att[np.argsort(att[:, 1])]
    cut = np.where(np.diff(att[:, 1]) > 1000)[0] + 1  # launches: attention block starts more than 10 us apart
    rows = []
    for g in np.split(att, cut):
        t0 = g[:, 1].min()
        w = wo[(wo[:, 1] >= t0 - 100) & (wo[:, 1] < t0 + 3000)]
        c = comb[(comb[:, 1] >= t0 - 100) & (comb[:, 1] < t0 + 3000)]
        if not len(w):
            continue
        T = lambda x: (x - t0) / 100.0
        stored = max(g[:, 5].max(), c[:, 7].max() if len(c) else 0)
        reads, cheap = w[:, 0] & 0xFFFF, (w[:, 0] >> 16) & 0xFFFF  # full reads of x; one-word polls ahead of them
        rows.append([T(g[:, 2].max()), T(g[:, 7].max()), T(stored), T(w[:, 1].max()), T(w[:, 2]).mean(), T(w[:, 3]).mean(),
                     T(w[:, 3]).max(), T(w[:, 4]).mean(), T(w[:, 5]).mean(), T(w[:, 5]).max(), reads.mean(), reads.max(), cheap.mean(), cheap.max()])
    r = np.array(rows)
    print(f"context {ctx}: {len(r)} fused launches ({len(att)} attention blocks, {len(comb)} combiners); "
          f"mean / max over the launches (us from the launch's first block start):")
    if not len(r):
        continue
    for n, v, x in zip(names, r.mean(axis=0), r.max(axis=0)):
        print(f"  {n:22s} {v:7.2f} {x:7.2f}")
m.close()
