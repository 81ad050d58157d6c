"""Weight-only int4 (group size 128) on the batched frame (BASELINE config 3 shapes: synthetic S2-Pro widths,
32 slots, ragged prompts uniform 16-256 seed 2, top_k 30 / top_p 0.8 / temperature 0.8, graph-replayed
frames): frame time and audio-s/s of the int4 model on its dequantised bf16 fragment copy (fm_tune
"bstream_q4" 0, the behaviour before the knob existed: the baseline) and streaming the 4-bit codes
("bstream_q4" 1).  Every measurement restarts from the same prefilled state (warm-up frames, then a timed
window closed by the host copy of the last frame's columns); the two are interleaved and repeated in one
process.  Then, per form: the "linear" launches of one frame replayed back to back (fm_llm_kernel_bench)
and the per-shape mean kernel spans of one eager frame from the per-block stamps ("debug_ts").

The driver runs each GPU step as a child process of its own under `timeout -k 10` and stops at the first
non-zero status; the steps leave JSON beside the report, the driver writes the report.
Usage: python scripts/b32_int4_probe.py [out.md] [timed frames, default 192]"""
import json
import os
import subprocess
import sys
import time
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))

B, WARM, REPS = 32, 24, 3
FRAME_RATE = 44100.0 / 2048.0
STEPS = [("frames", 420), ("spans", 240)]  # (step, its time limit in seconds)


def _model():
    import numpy as np

    from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig
    from fishmi.llm import DualARModel

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
    m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=B, quant="int4",
                              groupsize=128)
    slots = list(range(B))

    def start(q4):
        from fishmi import native

        native.tune("bstream_q4", q4)
        m.use_graph(True)  # drops the captured frames: the next ones are recorded under the knob
        m.prefill_batch(slots, prompts, [sp] * B)
        m.decode_frames(slots, WARM)

    return m, slots, start


def step_frames(timed):
    """interleaved frame-time windows, then the frame's linear launches replayed back to back"""
    m, slots, start = _model()
    ms = {0: [], 1: []}
    for rep in range(REPS + 1):  # round 0 warms both legs up and is not reported
        for q4 in (0, 1):
            start(q4)
            t0 = time.perf_counter()
            m.decode_frames(slots, timed)
            dt = (time.perf_counter() - t0) / timed * 1e3
            if rep:
                ms[q4].append(dt)
            print(f"round {rep} bstream_q4 {q4}: {dt:.3f} ms per frame", flush=True)
    bench = {}
    for q4 in (0, 1):
        start(q4)
        us, n, b = m.kernel_bench("linear", 20)
        bench[q4] = (us, n, b)
    m.close()
    return {"ms": {str(k): v for k, v in ms.items()}, "bench": {str(k): v for k, v in bench.items()}}


def step_spans(_timed):
    """per-shape kernel spans of one eager frame under each knob value"""
    import numpy as np

    from fishmi import native

    m, slots, start = _model()
    spans = {}
    for q4 in (0, 1):
        start(q4)
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
        spans[str(q4)] = {str(tag): (len(v), float(np.mean([c[2] - c[1] for c in v])) / 100.0) for tag, v in by.items()}
    m.use_graph(True)
    m.close()
    return spans


def report(res, timed):
    import numpy as np

    lines = []
    emit = lines.append
    ms = {int(k): v for k, v in res["frames"]["ms"].items()}
    emit("# Batched frame, weight-only int4 on the 4-bit codes vs on their dequantised bf16 copy (MI355X)")
    emit("")
    emit(f"Synthetic S2-Pro widths, int4 with groups of 128, {B} slots, prompts uniform 16-256 (seed 2), graph replay; each "
         f"figure is one window of {timed} frames after {WARM} warm-up frames from the same prefilled state, legs "
         f"interleaved, {REPS} repeats after one unreported round.  The baseline is bstream_q4 0 in the same run.")
    emit("")
    emit("| leg | frame ms (repeats) | median ms | spread ms | audio-s/s |")
    emit("|---|---|---|---|---|")
    names = {0: "int4, bstream_q4 0 (baseline)", 1: "int4, bstream_q4 1"}
    med = {}
    for q4 in (0, 1):
        v = ms[q4]
        med[q4] = float(np.median(v))
        emit(f"| {names[q4]} | {', '.join(f'{x:.3f}' for x in v)} | {med[q4]:.3f} | {max(v) - min(v):.3f} | "
             f"{B / (med[q4] * 1e-3) / FRAME_RATE:.1f} |")
    spread = max(max(ms[q4]) - min(ms[q4]) for q4 in (0, 1))
    gain = med[0] - med[1]
    emit("")
    emit(f"int4 on the codes vs the baseline: {gain:+.3f} ms per frame ({med[0] / med[1]:.3f}x); the larger of the two legs' "
         f"spreads over the three repeats is {spread:.3f} ms -> the knob's default is {'on' if gain > spread else 'off'} by "
         f"the rule \"faster by more than that spread\".")
    emit("")
    emit("## The frame's linear launches replayed back to back (fm_llm_kernel_bench \"linear\", 20 repetitions)")
    emit("")
    emit("| form | launches | avg us per launch | ms per frame | counted GB per frame | GB/s |")
    emit("|---|---|---|---|---|---|")
    for q4 in (0, 1):
        us, n, b = res["frames"]["bench"][str(q4)]
        emit(f"| bstream_q4 {q4} | {n} | {us:.2f} | {us * n / 1e3:.3f} | {b / 1e9:.3f} | {b / (us * n * 1e-6) / 1e9:.0f} |")
    emit("")
    emit("## Mean kernel span per shape, one eager frame (\"debug_ts\" stamps: first block start to last block end, us)")
    emit("")
    emit("| N | K | launches | span us, bstream_q4 0 | span us, bstream_q4 1 | ratio |")
    emit("|---|---|---|---|---|---|")
    s0, s1 = res["spans"]["0"], res["spans"]["1"]
    for tag in sorted(s0, key=int):
        n0, a = s0[tag]
        _, b = s1.get(tag, (0, float("nan")))
        emit(f"| {(int(tag) & 0xFFFF) * 16} | {int(tag) >> 16} | {n0} | {a:.2f} | {b:.2f} | {a / b:.2f} |")
    emit("")
    emit("6144 x 2560 is wqkv, 2560 x 4096 wo, 19456 x 2560 w1 || w3 and 2560 x 9728 w2 (slow and fast layers alike).  The "
         "N = 4096 row holds the codebook head and the tied LM head (4097 rows of bf16 embeddings, the same stamp tag), "
         "which never takes the int4 form.")
    return lines


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, out, timed = sys.argv[2], sys.argv[3], int(sys.argv[4])
        res = {"frames": step_frames, "spans": step_spans}[name](timed)
        with open(out, "w") as f:
            json.dump(res, f)
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 192
    base = os.path.splitext(out_path)[0] if out_path else os.path.join(ROOT, "bench_out", "b32_int4")
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    res = {}
    for name, limit in STEPS:
        js = f"{base}.{name}.json"
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, js, str(timed)]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping", flush=True)
            return rc
        with open(js) as f:
            res[name] = json.load(f)
    lines = report(res, timed)
    print("\n".join(lines), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
