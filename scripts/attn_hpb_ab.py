"""A/B of fm_tune settings of the batch-1 slow attention (fd_hpb: q heads of a kv head per attn_fd block;
fd_min16: its split length) in ONE process, as scripts/fast_pair_ab.py does it: S2-Pro synthetic weights
as bench.py makes them, batch 1, graph-replayed frames after a PROMPT-token prompt, the settings
interleaved (A B C A B C ...).  Prints ms per frame per repetition, each setting's mean and its own
max - min, and whether the gain over the first setting clears three times that setting's spread (this
project's bar for keeping a default).  Every setting must sample the first one's columns.  QUANT=int8 / int4
(GROUPSIZE, default 128) times a weight-only handle (fm_tune slow_attn_wo_q and its like).

usage: [SETTINGS="fd_hpb=4;fd_hpb=1;fd_hpb=2"] [PROMPT=64] [QUANT=int8|int4] python scripts/attn_hpb_ab.py [repetitions >= 3] [frames]"""
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
PROMPT = int(os.environ.get("PROMPT", "64"))
QUANT = os.environ.get("QUANT") or None
GROUPSIZE = int(os.environ.get("GROUPSIZE", "128"))
SETTINGS = [dict((k, int(v)) for k, v in (kv.split("=") for kv in s.split(",") if kv))
            for s in os.environ.get("SETTINGS", "fd_hpb=4;fd_hpb=1;fd_hpb=2").split(";")]
NAMES = [",".join(f"{k}={v}" for k, v in s.items()) for s in SETTINGS]
old = {k: native.tune_get(k) for s in SETTINGS for k in s}

cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
t0 = time.perf_counter()
m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=1, quant=QUANT,
                          groupsize=GROUPSIZE)
print(f"model ready in {time.perf_counter() - t0:.1f} s; quant {QUANT}; prompt {PROMPT}, {FRAMES} frames, {REPS} repetitions")
p = np.zeros((cfg.num_codebooks + 1, PROMPT), np.int32)
p[0] = np.random.default_rng(1).integers(16, cfg.semantic_begin_id, PROMPT)
sp = DualARModel.sampling(mask_im_end=True)


def run(i, frames):
    for k, v in {**old, **SETTINGS[i]}.items():
        native.tune(k, v)
    m.use_graph(True)  # re-capture under the knobs
    m.prefill(0, p, sp)
    m.decode_frames([0], 8)  # capture + warm-up
    t = time.perf_counter()
    cols = m.decode_frames([0], frames)
    return (time.perf_counter() - t) * 1e3 / frames, cols


ref = None
for i, name in enumerate(NAMES):  # warm-up round, and the streams must be the same stream
    ms, cols = run(i, FRAMES)
    ref = cols if ref is None else ref
    print(f"warm-up {name}: {ms:.4f} ms/frame, columns equal to {NAMES[0]}'s: {bool(np.array_equal(cols, ref))}")
res = [[] for _ in SETTINGS]
for r in range(REPS):
    for i in range(len(SETTINGS)):
        res[i].append(run(i, FRAMES)[0])
    print(f"rep {r}: " + "  ".join(f"{n}: {res[i][-1]:.4f}" for i, n in enumerate(NAMES)), flush=True)
for k, v in old.items():
    native.tune(k, v)
mean = [float(np.mean(v)) for v in res]
spread = [max(v) - min(v) for v in res]
print(f"baseline {NAMES[0]} spread max - min: {spread[0] * 1e3:.1f} us; keep a default only above 3x = {3 * spread[0] * 1e3:.1f} us")
for i, n in enumerate(NAMES):
    gain = mean[0] - mean[i]
    print(f"{n}: mean {mean[i]:.4f} ms/frame, max - min {spread[i] * 1e3:.1f} us, gain over {NAMES[0]} {gain * 1e3:7.1f} us "
          f"({100 * gain / mean[0]:.2f} %)" + ("" if i == 0 else f"  -> {'clears' if gain > 3 * spread[0] else 'does NOT clear'} 3x spread"))
m.close()
