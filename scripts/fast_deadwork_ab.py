"""A/B of the fast decoder's two removals (fm_tune rowgemv bit 5: first-layer QKV table; bit 6:
K / V only at codebook 0) in ONE process: S2-Pro synthetic weights as bench.py makes them, batch 1,
graph-replayed frames from a 64-token prompt, settings 27 / 59 / 91 / 123 interleaved
(A B C D A B C D ...).  Prints ms per frame per repetition, the median per setting, the baseline's
own max - min (the spread a gain has to clear three times over) and each setting's median gain.

usage: python scripts/fast_deadwork_ab.py [repetitions >= 5] [frames >= 200]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 200
SETTINGS = (27, 59, 91, 123)

cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
t0 = time.perf_counter()
m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=1)
print(f"model ready in {time.perf_counter() - t0:.1f} s (finalize builds the QKV table under the default knob)")
p = np.zeros((cfg.num_codebooks + 1, 64), np.int32)
p[0] = np.random.default_rng(1).integers(16, cfg.semantic_begin_id, 64)
sp = DualARModel.sampling(mask_im_end=True)


def run(v, frames):
    native.tune("rowgemv", v)
    m.use_graph(True)  # re-capture under the knob
    t = time.perf_counter()
    m.prefill(0, p, sp)  # (rebuilds the table when bit 5 is on: not timed below)
    build = time.perf_counter() - t
    m.decode_frames([0], 8)  # capture + warm-up
    t = time.perf_counter()
    cols = m.decode_frames([0], frames)
    return (time.perf_counter() - t) * 1e3 / frames, cols, build


ref = None
for v in SETTINGS:  # warm-up round, and the streams must be the same stream
    ms, cols, build = run(v, FRAMES)
    ref = cols if ref is None else ref
    print(f"warm-up rowgemv {v:3d}: {ms:.4f} ms/frame, prefill call {build * 1e3:.1f} ms, "
          f"columns equal to 27's: {bool(np.array_equal(cols, ref))}")
res = {v: [] for v in SETTINGS}
for r in range(REPS):
    for v in SETTINGS:
        res[v].append(run(v, FRAMES)[0])
    print(f"rep {r}: " + "  ".join(f"{v}: {res[v][-1]:.4f}" for v in SETTINGS))
native.tune("rowgemv", 123)
med = {v: float(np.median(res[v])) for v in SETTINGS}
spread = max(res[27]) - min(res[27])
print(f"baseline (27) spread max - min: {spread * 1e3:.1f} us; keep a part only above 3x = {3 * spread * 1e3:.1f} us")
for v in SETTINGS:
    gain = med[27] - med[v]
    print(f"rowgemv {v:3d}: median {med[v]:.4f} ms/frame, gain over 27 {gain * 1e3:7.1f} us ({100 * gain / med[27]:.2f} %)"
          + ("" if v == 27 else f"  -> {'clears' if gain > 3 * spread else 'does NOT clear'} 3x spread"))
m.close()
