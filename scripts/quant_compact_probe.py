"""Compact weight-only handles (fm_llm_set_quant_compact) against the same handles with the bf16 fragment copy
of their quantised linears: synthetic S2-Pro widths, int8 and int4 (groups of 128), opened with 1 and with 32
slots.  Per (quantisation, slots) one child process builds both handles from the same seed and records
fm_llm_memory_info of each, the wall time of a 64-token and of a 646-token prefill on slot 0, and the
graph-replayed decode frame time at all of the handle's slots (B = 1 or B = 32) -- the two handles interleaved,
three repeats after one unreported round.  The decode frames run the same launches in both modes; the prompt
pass reads code bytes instead of 2 bytes per weight on the compact handle.

The driver runs each GPU step as a child process of its own under `timeout -k 10` and stops at the first
non-zero status; the steps leave JSON beside the report, the driver writes the report.
Usage: python scripts/quant_compact_probe.py [out.md] [timed frames, default 96]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))

WARM, REPS = 16, 3
PROMPTS = (64, 646)
STEPS = [(q, n) for q in ("int8", "int4") for n in (1, 32)]
LIMIT = 420  # seconds per step


def step(quant, slots, timed):
    import numpy as np

    from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig
    from fishmi.llm import DualARModel

    cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
    cfg.im_end_id = S2_PRO_IM_END_ID
    cfg.max_seq_len = 1024
    rng = np.random.default_rng(2)

    def prompt(T):
        p = np.zeros((cfg.num_codebooks + 1, int(T)), np.int32)
        p[0] = rng.integers(16, cfg.semantic_begin_id, int(T))
        return p

    long_prompts = {T: prompt(T) for T in PROMPTS}
    batch = [prompt(T) for T in rng.integers(16, 257, slots)]
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, mask_im_end=True)
    ids = list(range(slots))
    legs = {}
    for compact in (False, True):
        legs[compact] = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=slots,
                                              quant=quant, groupsize=128, compact=compact)
    res = {"memory": {str(int(c)): m.memory_info() for c, m in legs.items()},
           "prefill_ms": {str(int(c)): {str(T): [] for T in PROMPTS} for c in legs},
           "frame_ms": {str(int(c)): [] for c in legs}}
    first = {}
    for rep in range(REPS + 1):  # round 0 warms both legs up and is not reported
        for compact, m in legs.items():
            key = str(int(compact))
            for T in PROMPTS:
                t0 = time.perf_counter()
                col = m.prefill(0, long_prompts[T], sp)
                dt = (time.perf_counter() - t0) * 1e3
                first.setdefault((compact, T), col)
                if rep:
                    res["prefill_ms"][key][str(T)].append(dt)
            m.prefill_batch(ids, batch, [sp] * slots) if slots > 1 else m.prefill(0, batch[0], sp)
            m.decode_frames(ids, WARM)
            t0 = time.perf_counter()
            m.decode_frames(ids, timed)
            dt = (time.perf_counter() - t0) / timed * 1e3
            if rep:
                res["frame_ms"][key].append(dt)
            print(f"{quant} slots {slots} round {rep} compact {int(compact)}: frame {dt:.3f} ms", flush=True)
    # the two modes compute the same thing: the first column of every timed prefill agrees
    res["same_first_columns"] = all(np.array_equal(first[(False, T)], first[(True, T)]) for T in PROMPTS)
    for m in legs.values():
        m.close()
    return res


def report(res, timed):
    import numpy as np

    lines = []
    emit = lines.append
    emit("# Compact weight-only handles: device bytes, prefill and decode frame times (MI355X)")
    emit("")
    emit("Synthetic S2-Pro widths (max_seq_len 1024), weight-only int8 and int4 (groups of 128), handles opened with 1 and "
         "with 32 slots; `compact` keeps only the codes of the quantised linears (fm_llm_set_quant_compact), the other "
         "handle also their bf16 fragment copy.  Both handles live in one process, from the same seed.")
    emit("")
    emit("## fm_llm_memory_info, MB (10^6 bytes)")
    emit("")
    emit("| model | slots | mode | bf16 fragments | GEMV codes + tables | step-granular codes | row-major copies | other weights | "
         "KV caches | activations | total |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|")
    fields = ("quant_fragments", "gemv_codes", "step_codes", "row_major", "other_weights", "kv_cache", "activations", "total")
    for (q, n), r in res.items():
        for c in ("0", "1"):
            d = r["memory"][c]
            emit(f"| {q} | {n} | {'compact' if c == '1' else 'with bf16 copy'} | " +
                 " | ".join(f"{d[f] / 1e6:.1f}" for f in fields) + " |")
    emit("")
    emit(f"## Times: median of {REPS} interleaved repeats (spread = max - min), ms")
    emit("")
    emit(f"Prefill: wall time of one fm_llm_prefill on slot 0 (the prompt pass, the first frame and the host copy of its "
         f"column).  Frame: one window of {timed} graph-replayed frames of all the handle's slots after {WARM} warm-up frames.")
    emit("")
    emit("| model | slots | measurement | with bf16 copy | compact | compact / with copy |")
    emit("|---|---|---|---|---|---|")

    def row(q, n, name, a, b):
        ma, mb = float(np.median(a)), float(np.median(b))
        emit(f"| {q} | {n} | {name} | {ma:.3f} ({max(a) - min(a):.3f}) | {mb:.3f} ({max(b) - min(b):.3f}) | {mb / ma:.3f} |")

    for (q, n), r in res.items():
        for T in PROMPTS:
            row(q, n, f"prefill, {T} tokens", r["prefill_ms"]["0"][str(T)], r["prefill_ms"]["1"][str(T)])
        row(q, n, f"decode frame, B = {n}", r["frame_ms"]["0"], r["frame_ms"]["1"])
    emit("")
    same = all(r["same_first_columns"] for r in res.values())
    emit(f"First sampled column of every timed prefill equal between the two modes: {'yes' if same else 'NO'}.")
    return lines


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        quant, slots, out, timed = sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
        with open(out, "w") as f:
            json.dump(step(quant, slots, timed), f)
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 96
    base = os.path.splitext(out_path)[0] if out_path else os.path.join(ROOT, "bench_out", "quant_compact")
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    res = {}
    for quant, slots in STEPS:
        js = f"{base}.{quant}.{slots}.json"
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", quant, str(slots), js,
               str(timed)]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {quant} / {slots} slots ended with status {rc}: stopping", flush=True)
            return rc
        with open(js) as f:
            res[(quant, slots)] = json.load(f)
    lines = report(res, timed)
    print("\n".join(lines), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
