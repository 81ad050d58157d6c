"""A/B of the fused fast attention + wo launch's attention chain (fm_tune fattn_ilp: q / k
prep side by side, score / softmax / PV over a compile-time position count)
in ONE process: S2-Pro synthetic weights as bench.py makes them, batch 1, graph-replayed frames
from a 64-token prompt, knob off and on interleaved (A B A B ...).  Prints ms per frame per
repetition, the median per setting, the baseline's own max - min (the spread a gain has to clear
three times over) and the median gain.

usage: python scripts/fattn_chain_ab.py [repetitions >= 3] [frames >= 200]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 200
SETTINGS = (0, 1)  # fattn_ilp; 0: the early-exit loops
BASE = SETTINGS[0]

cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
t0 = time.perf_counter()
m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=1)
print(f"model ready in {time.perf_counter() - t0:.1f} s")
p = np.zeros((cfg.num_codebooks + 1, 64), np.int32)
p[0] = np.random.default_rng(1).integers(16, cfg.semantic_begin_id, 64)
sp = DualARModel.sampling(mask_im_end=True)


def run(s, frames):
    native.tune("fattn_ilp", s)
    m.use_graph(True)  # re-capture under the knobs
    m.prefill(0, p, sp)
    m.decode_frames([0], 8)  # capture + warm-up
    t = time.perf_counter()
    cols = m.decode_frames([0], frames)
    return (time.perf_counter() - t) * 1e3 / frames, cols


ref = None
for s in SETTINGS:  # warm-up round, and the streams must be the same stream
    ms, cols = run(s, FRAMES)
    ref = cols if ref is None else ref
    print(f"warm-up fattn_ilp {s}: {ms:.4f} ms/frame, columns equal to {BASE}'s: {bool(np.array_equal(cols, ref))}")
res = {s: [] for s in SETTINGS}
for r in range(REPS):
    for s in SETTINGS:
        res[s].append(run(s, FRAMES)[0])
    print(f"rep {r}: " + "  ".join(f"{s}: {res[s][-1]:.4f}" for s in SETTINGS), flush=True)
native.tune("fattn_ilp", 1)
med = {s: float(np.median(res[s])) for s in SETTINGS}
spread = max(res[BASE]) - min(res[BASE])
print(f"baseline {BASE} spread max - min: {spread * 1e3:.1f} us; keep a part only above 3x = {3 * spread * 1e3:.1f} us")
for s in SETTINGS:
    gain = med[BASE] - med[s]
    print(f"fattn_ilp {s}: median {med[s]:.4f} ms/frame, gain over {BASE} {gain * 1e3:7.1f} us ({100 * gain / med[BASE]:.2f} %)"
          + ("" if s == BASE else f"  -> {'clears' if gain > 3 * spread else 'does NOT clear'} 3x spread"))
m.close()
