"""Weight-only int8 on the batched frame (BASELINE config 3 shapes: synthetic S2-Pro widths, 32 slots,
ragged prompts uniform 16-256 seed 2, top_k 30 / top_p 0.8 / temperature 0.8, graph-replayed frames):
frame time and audio-s/s of the bf16 model, of the int8 model on the bf16 copy of its codes
(fm_tune "bstream_q8" 0) and of the int8 model streaming the codes ("bstream_q8" 1).  Every
measurement restarts from the same prefilled state (warm-up frames, then a timed window closed by the
host copy of the last frame's columns); the three are interleaved and repeated in one process.  Then,
per int8 form: the "linear" launches of one frame replayed back to back (fm_llm_kernel_bench) and the
per-shape kernel spans of one eager frame from the per-block stamps ("debug_ts").
Usage: python scripts/b32_int8_probe.py [out.md] [timed frames, default 192]"""
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

B, WARM, REPS = 32, 24, 3
FRAME_RATE = 44100.0 / 2048.0
out_path = sys.argv[1] if len(sys.argv) > 1 else None
timed = int(sys.argv[2]) if len(sys.argv) > 2 else 192
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
rng = np.random.default_rng(2)
prompts = []
for T in rng.integers(16, 257, B):
    p = np.zeros((cfg.num_codebooks + 1, int(T)), np.int32)
    p[0] = rng.integers(16, cfg.semantic_begin_id, int(T))
    prompts.append(p)
sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, mask_im_end=True)
slots = list(range(B))
models = {
    "int8": DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=B, quant="int8"),
    "bf16": DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=B),
}
legs = [("bf16", "bf16", 0), ("int8, bstream_q8 0 (baseline)", "int8", 0), ("int8, bstream_q8 1", "int8", 1)]


def start(m, q8):
    native.tune("bstream_q8", q8)
    m.use_graph(True)  # drops the captured frames: the next ones are recorded under the knob
    m.prefill_batch(slots, prompts, [sp] * B)
    m.decode_frames(slots, WARM)


ms = defaultdict(list)
for rep in range(REPS + 1):  # round 0 warms every leg up and is not reported
    for name, mk, q8 in legs:
        m = models[mk]
        start(m, q8)
        t0 = time.perf_counter()
        m.decode_frames(slots, timed)
        dt = (time.perf_counter() - t0) / timed * 1e3
        if rep:
            ms[name].append(dt)

emit("# Batched frame, weight-only int8 on the codes vs on their bf16 copy (MI355X)")
emit()
emit(f"Synthetic S2-Pro widths, {B} slots, prompts uniform 16-256 (seed 2), graph replay; each figure is one window of "
     f"{timed} frames after {WARM} warm-up frames from the same prefilled state, legs interleaved, {REPS} repeats "
     f"after one unreported round.")
emit()
emit("| leg | frame ms (repeats) | median ms | spread ms | audio-s/s |")
emit("|---|---|---|---|---|")
med = {}
for name, _, _ in legs:
    v = ms[name]
    med[name] = float(np.median(v))
    emit(f"| {name} | {', '.join(f'{x:.3f}' for x in v)} | {med[name]:.3f} | {max(v) - min(v):.3f} | "
         f"{B / (med[name] * 1e-3) / FRAME_RATE:.1f} |")
base, new = legs[1][0], legs[2][0]
spread = max(ms[base]) - min(ms[base])
gain = med[base] - med[new]
emit()
emit(f"int8 on the codes vs the baseline: {gain:+.3f} ms per frame ({med[base] / med[new]:.3f}x); the baseline's three "
     f"repeats spread {spread:.3f} ms -> the knob's default is {'on' if gain > spread else 'off'} by the rule "
     f"\"faster by more than that spread\".")

# per-launch figures, int8 model, both forms
m = models["int8"]
emit()
emit("## The frame's linear launches replayed back to back (fm_llm_kernel_bench \"linear\", 20 repetitions)")
emit()
emit("| form | launches | avg us per launch | ms per frame | counted GB per frame | GB/s |")
emit("|---|---|---|---|---|---|")
for q8 in (0, 1):
    start(m, q8)
    us, n, b = m.kernel_bench("linear", 20)
    emit(f"| bstream_q8 {q8} | {n} | {us:.2f} | {us * n / 1e3:.3f} | {b / 1e9:.3f} | {b / (us * n * 1e-6) / 1e9:.0f} |")
emit()
emit("## Kernel span per shape, one eager frame (\"debug_ts\" stamps: first block start to last block end, us)")
emit()
spans = {}
for q8 in (0, 1):
    start(m, q8)
    m.use_graph(False)
    native.tune("debug_ts", 1)
    m.decode_frames(slots, 1)
    rec = native.debug_ts_read().astype(np.int64)
    native.tune("debug_ts", 0)
    rec = rec[(rec[:, 0] >> 32) >= (1 << 16)]  # bsacc records: (K << 16 | N >> 4) << 32 | block
    rec = rec[np.argsort(rec[:, 1], kind="stable")]
    by, cur = defaultdict(list), None
    for r in rec:
        tag = int(r[0]) >> 32
        if cur is None or tag != cur[0] or r[1] > cur[2]:
            cur = [tag, int(r[1]), 0]
            by[tag].append(cur)
        cur[2] = max(cur[2], int(r[4]))
    spans[q8] = {tag: (len(v), float(np.mean([c[2] - c[1] for c in v])) / 100.0) for tag, v in by.items()}
emit("| N | K | launches | span us, bstream_q8 0 | span us, bstream_q8 1 | ratio |")
emit("|---|---|---|---|---|---|")
for tag in sorted(spans[0]):
    n0, s0 = spans[0][tag]
    _, s1 = spans[1].get(tag, (0, float("nan")))
    emit(f"| {(tag & 0xFFFF) * 16} | {tag >> 16} | {n0} | {s0:.2f} | {s1:.2f} | {s0 / s1:.2f} |")
emit()
emit("The N = 4096 row also holds the tied LM head (4097 rows of bf16 embeddings, the same stamp tag), which never "
     "takes the int8 form.")
for mm in models.values():
    mm.close()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
