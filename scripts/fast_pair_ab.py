"""A/B of the paired fast pass (fm_tune fast_pair: codebook positions 0 and 1 of the fast decoder as
one two-row pass) in ONE process: S2-Pro synthetic weights as bench.py makes them, batch 1,
graph-replayed frames from a 64-token prompt, knob off and on interleaved (A B A B ...).  Prints ms
per frame per repetition, each setting's mean and its own max - min, and whether the gain clears
three times the baseline's spread (this project's bar for keeping a default).  With --quant int8 | int4 the model
is a weight-only handle (int4: group size 128) and the knob is fast_pair_q, 0 against the mode's bit.

usage: python scripts/fast_pair_ab.py [--quant int8|int4] [repetitions >= 3] [frames >= 200]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

ARGS = sys.argv[1:]
QUANT = None
if "--quant" in ARGS:
    i = ARGS.index("--quant")
    QUANT = ARGS[i + 1]
    assert QUANT in ("int8", "int4"), "--quant int8 | int4"
    del ARGS[i:i + 2]
REPS = int(ARGS[0]) if len(ARGS) > 0 else 6
FRAMES = int(ARGS[1]) if len(ARGS) > 1 else 400
KNOB = "fast_pair_q" if QUANT else "fast_pair"
SETTINGS = (0, {None: 1, "int8": 1, "int4": 2}[QUANT])  # 0: the one-row passes
BASE = SETTINGS[0]
DEFAULT = native.tune_get(KNOB)

cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
t0 = time.perf_counter()
m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=1,
                          **({"quant": QUANT, "groupsize": 128} if QUANT else {}))
print(f"{QUANT or 'bf16'} model ready in {time.perf_counter() - t0:.1f} s; knob {KNOB}")
p = np.zeros((cfg.num_codebooks + 1, 64), np.int32)
p[0] = np.random.default_rng(1).integers(16, cfg.semantic_begin_id, 64)
sp = DualARModel.sampling(mask_im_end=True)


def run(s, frames):
    native.tune(KNOB, s)
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
    print(f"warm-up {KNOB} {s}: {ms:.4f} ms/frame, columns equal to {BASE}'s: {bool(np.array_equal(cols, ref))}")
res = {s: [] for s in SETTINGS}
for r in range(REPS):
    for s in SETTINGS:
        res[s].append(run(s, FRAMES)[0])
    print(f"rep {r}: " + "  ".join(f"{s}: {res[s][-1]:.4f}" for s in SETTINGS), flush=True)
native.tune(KNOB, DEFAULT)
mean = {s: float(np.mean(res[s])) for s in SETTINGS}
spread = {s: max(res[s]) - min(res[s]) for s in SETTINGS}
print(f"baseline {BASE} spread max - min: {spread[BASE] * 1e3:.1f} us; keep a default only above 3x = {3 * spread[BASE] * 1e3:.1f} us")
for s in SETTINGS:
    gain = mean[BASE] - mean[s]
    print(f"{KNOB} {s}: mean {mean[s]:.4f} ms/frame, max - min {spread[s] * 1e3:.1f} us, gain over {BASE} {gain * 1e3:7.1f} us "
          f"({100 * gain / mean[BASE]:.2f} %)" + ("" if s == BASE else f"  -> {'clears' if gain > 3 * spread[BASE] else 'does NOT clear'} 3x spread"))
m.close()
