"""A/B of the paired fast pass (fm_tune fast_pair: codebook positions 0 and 1 of the fast decoder as
one two-row pass) in ONE process: S2-Pro synthetic weights as bench.py makes them, batch 1,
graph-replayed frames from a 64-token prompt, knob off and on interleaved (A B A B ...).  Prints ms
per frame per repetition, each setting's mean and its own max - min, and whether the gain clears
three times the baseline's spread (this project's bar for keeping a default).

usage: python scripts/fast_pair_ab.py [repetitions >= 3] [frames >= 200]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 400
SETTINGS = (0, 1)  # fast_pair; 0: the one-row passes
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
    native.tune("fast_pair", s)
    m.use_graph(True)  # re-capture under the knob
    m.prefill(0, p, sp)
    m.decode_frames([0], 8)  # capture + warm-up
    t = time.perf_counter()
    cols = m.decode_frames([0], frames)
    return (time.perf_counter() - t) * 1e3 / frames, cols


ref = None
for s in SETTINGS:  # warm-up round, and the streams must be the same stream
    ms, cols = run(s, FRAMES)
    ref = cols if ref is None else ref
    print(f"warm-up fast_pair {s}: {ms:.4f} ms/frame, columns equal to {BASE}'s: {bool(np.array_equal(cols, ref))}")
res = {s: [] for s in SETTINGS}
for r in range(REPS):
    for s in SETTINGS:
        res[s].append(run(s, FRAMES)[0])
    print(f"rep {r}: " + "  ".join(f"{s}: {res[s][-1]:.4f}" for s in SETTINGS), flush=True)
native.tune("fast_pair", 1)
mean = {s: float(np.mean(res[s])) for s in SETTINGS}
spread = {s: max(res[s]) - min(res[s]) for s in SETTINGS}
print(f"baseline {BASE} spread max - min: {spread[BASE] * 1e3:.1f} us; keep a default only above 3x = {3 * spread[BASE] * 1e3:.1f} us")
for s in SETTINGS:
    gain = mean[BASE] - mean[s]
    print(f"fast_pair {s}: mean {mean[s]:.4f} ms/frame, max - min {spread[s] * 1e3:.1f} us, gain over {BASE} {gain * 1e3:7.1f} us "
          f"({100 * gain / mean[BASE]:.2f} %)" + ("" if s == BASE else f"  -> {'clears' if gain > 3 * spread[BASE] else 'does NOT clear'} 3x spread"))
m.close()
