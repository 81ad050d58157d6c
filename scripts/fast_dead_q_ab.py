"""A/B of fm_tune fast_dead_q (weight-only int8 / int4 handles: bit 0 the first fast layer's QKV table, bit 1
K / V only at codebook 0) in ONE process: S2-Pro synthetic weights as bench.py makes them, int8, then int4 group
128, batch 1, graph-replayed frames from a 64-token prompt, settings 0 / 1 / 2 / 3 interleaved (A B C D A B C D
...).  Prints ms per frame per repetition, per setting the mean and max - min, the baseline's own max - min (the
spread a gain has to clear three times over), each setting's mean gain, and the table's build time (the first
prefill call after a knob change, with the table minus without).

usage: python scripts/fast_dead_q_ab.py [repetitions >= 6] [frames >= 200]"""
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
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 200
SETTINGS = (0, 1, 2, 3)

cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
p = np.zeros((cfg.num_codebooks + 1, 64), np.int32)
p[0] = np.random.default_rng(1).integers(16, cfg.semantic_begin_id, 64)
sp = DualARModel.sampling(mask_im_end=True)
default = native.tune_get("fast_dead_q")


def run(m, v, frames):
    native.tune("fast_dead_q", v)
    m.use_graph(True)  # re-capture under the knob
    t = time.perf_counter()
    m.prefill(0, p, sp)  # (rebuilds the table when bit 0 is on: not timed below)
    build = time.perf_counter() - t
    m.decode_frames([0], 8)  # capture + warm-up
    t = time.perf_counter()
    cols = m.decode_frames([0], frames)
    return (time.perf_counter() - t) * 1e3 / frames, cols, build


for quant in ("int8", "int4"):
    t0 = time.perf_counter()
    m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=1, quant=quant,
                              groupsize=128)
    print(f"== {quant}: model ready in {time.perf_counter() - t0:.1f} s")
    ref = None
    for v in SETTINGS:  # warm-up round, and the streams must be the same stream
        ms, cols, build = run(m, v, FRAMES)
        ref = cols if ref is None else ref
        print(f"warm-up fast_dead_q {v}: {ms:.4f} ms/frame, prefill call {build * 1e3:.1f} ms, "
              f"columns equal to 0's: {bool(np.array_equal(cols, ref))}")
    res = {v: [] for v in SETTINGS}
    builds = {v: [] for v in SETTINGS}
    for r in range(REPS):
        for v in SETTINGS:
            ms, _, build = run(m, v, FRAMES)
            res[v].append(ms)
            builds[v].append(build * 1e3)
        print(f"rep {r}: " + "  ".join(f"{v}: {res[v][-1]:.4f}" for v in SETTINGS))
    mean = {v: float(np.mean(res[v])) for v in SETTINGS}
    spread = max(res[0]) - min(res[0])
    print(f"{quant} baseline (0) spread max - min: {spread * 1e3:.1f} us; a bit defaults to on only above 3x = "
          f"{3 * spread * 1e3:.1f} us")
    for v in SETTINGS:
        gain = mean[0] - mean[v]
        print(f"{quant} fast_dead_q {v}: mean {mean[v]:.4f} ms/frame, max - min {(max(res[v]) - min(res[v])) * 1e3:5.1f} us, "
              f"gain over 0 {gain * 1e3:7.1f} us ({100 * gain / mean[0]:.2f} %)"
              + ("" if v == 0 else f"  -> {'clears' if gain > 3 * spread else 'does NOT clear'} 3x spread"))
    print(f"{quant} table build: prefill call median {np.median(builds[1]):.1f} ms with the table, "
          f"{np.median(builds[0]):.1f} ms without -> {np.median(builds[1]) - np.median(builds[0]):.1f} ms "
          f"({cfg.codebook_size} launches)")
    m.close()
native.tune("fast_dead_q", default)
