"""The 64-token prefill of weight-only int8 / int4 (groups of 128) models at synthetic S2-Pro widths under the three
routings of their 33 .. 64-row linears (fm_tune prompt_skinny_q): 2 the 16-row tile kernel (the routing before the
skinny prompt GEMM had code forms), 0 the skinny GEMM on the bf16 fragment copy, 1 the skinny GEMM on the
step-granular codes.  Per quantisation one child process builds two handles from the same seed -- one opened with 12
slots (bf16 copy and step-granular codes: all three routings) and a compact one (codes only: 2 and 1) -- warms every
routing up, then times them interleaved, three repeats of PREFILLS prefills each.  A prefill call returns the first
sampled column, so it ends in a stream synchronise: the time is the host clock around the call (the handle's stream
is non-blocking, so no event of another stream brackets it); the handle's own HIP events around every launch
(fm_llm_profile) give the "linear" class's device time of one more prefill per routing.

`--trace` runs three prefills per routing of the 12-slot handles only, for one separate
`rocprofv3 --kernel-trace --stats -- python scripts/prompt_q_probe.py --trace` run (scripts/rocprof_summary.py
tabulates its kernel_trace.csv); the kernels of the three routings differ by name.

The driver runs each GPU step as a child process of its own under `timeout -k 10` and stops at the first non-zero
status.  Usage: python scripts/prompt_q_probe.py [out.md]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))

T, PREFILLS, REPS = 64, 8, 3
QUANTS = ("int8", "int4")
ROUTES = {2: "tile kernel (old routing)", 0: "skinny GEMM, bf16 copy", 1: "skinny GEMM, codes"}
LIMIT = 240  # seconds per step


def _setup(quant, handles):
    import numpy as np

    from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig
    from fishmi.llm import DualARModel

    cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
    cfg.im_end_id = S2_PRO_IM_END_ID
    cfg.max_seq_len = 1024
    p = np.zeros((cfg.num_codebooks + 1, T), np.int32)
    p[0] = np.random.default_rng(3).integers(16, cfg.semantic_begin_id, T)
    legs = {}
    for name in handles:
        compact = name == "compact"
        legs[name] = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16",
                                           max_slots=1 if compact else 12, quant=quant, groupsize=128, compact=compact)
    return cfg, p, legs, DualARModel.sampling(top_k=1)


def _routes(name):
    return (2, 1) if name == "compact" else (2, 0, 1)


def step(quant):
    import numpy as np

    from fishmi import native

    cfg, p, legs, sp = _setup(quant, ("copy", "compact"))
    res = {n: {str(r): {"ms": [], "first": None} for r in _routes(n)} for n in legs}
    try:
        for rep in range(REPS + 1):  # round 0 warms every routing of every handle up and is not reported
            for name, m in legs.items():
                for r in _routes(name):
                    native.tune("prompt_skinny_q", r)
                    t0 = time.perf_counter()
                    for _ in range(PREFILLS):
                        col = m.prefill(0, p, sp)
                    dt = (time.perf_counter() - t0) / PREFILLS * 1e3
                    if rep:
                        res[name][str(r)]["ms"].append(dt)
                    res[name][str(r)]["first"] = [int(c) for c in col]
                    print(f"{quant} {name} routing {r} round {rep}: {dt:.3f} ms", flush=True)
        for name, m in legs.items():  # device time of the linears, one profiled prefill per routing
            for r in _routes(name):
                native.tune("prompt_skinny_q", r)
                m.profile(True)
                m.prefill(0, p, sp)
                ms, n, b = m.profile_read("linear")
                res[name][str(r)].update(linear_ms=ms, linear_launches=n, linear_bytes=b,
                                         prompt_q_launches=m.profile_read("prompt_q")[1])
                m.profile(False)
    finally:
        native.tune("prompt_skinny_q", 1)
        for m in legs.values():
            m.close()
    return res


def trace():
    from fishmi import native

    for quant in QUANTS:
        cfg, p, legs, sp = _setup(quant, ("copy",))
        for r in _routes("copy"):
            native.tune("prompt_skinny_q", r)
            for _ in range(3):  # (the first one of a routing loads its code objects)
                legs["copy"].prefill(0, p, sp)
        legs["copy"].close()
    print("ok")


def report(res):
    lines = []
    emit = lines.append
    emit("# Quantised 64-token prefill: the 33 .. 64-row linears on the tile kernel, on the skinny GEMM's bf16 copy, "
         "on its codes (MI355X)")
    emit("")
    emit(f"Synthetic S2-Pro widths (max_seq_len 1024), weight-only int8 and int4 (groups of 128).  `copy`: a handle "
         f"opened with 12 slots (bf16 fragment copy and step-granular codes); `compact`: codes only.  fm_tune "
         f"prompt_skinny_q picks the routing.  Each figure: the mean over {REPS} interleaved repeats of the mean "
         f"wall time of {PREFILLS} fm_llm_prefill calls of {T} tokens (each ends in a stream synchronise); spread = "
         f"max - min of the repeats.  linear: the \"linear\" class of one profiled prefill (HIP events around every "
         f"launch; the prompt pass's and the first frame's linears): device ms, launches, booked MB.")
    emit("")
    emit("| model | handle | routing | prefill ms (spread) | vs old routing | linear ms | launches | MB | prompt_q launches |")
    emit("|---|---|---|---|---|---|---|---|---|")
    verdict = []
    for q, r in res.items():
        for name, legs in r.items():
            mean = {k: sum(v["ms"]) / len(v["ms"]) for k, v in legs.items()}
            spread = {k: max(v["ms"]) - min(v["ms"]) for k, v in legs.items()}
            for k, v in legs.items():
                emit(f"| {q} | {name} | {ROUTES[int(k)]} | {mean[k]:.3f} ({spread[k]:.3f}) | {mean[k] / mean['2']:.3f} | "
                     f"{v['linear_ms']:.3f} | {v['linear_launches']} | {v['linear_bytes'] / 1e6:.1f} | {v['prompt_q_launches']} |")
            best = min((k for k in legs if k != "2"), key=lambda k: mean[k])
            verdict.append((q, name, mean["2"] - mean[best], max(spread["2"], spread[best]), best,
                            None if "0" not in legs else (mean["0"] - mean["1"], max(spread["0"], spread["1"]))))
            firsts = {tuple(v["first"]) for v in legs.values()}
            emit(f"| {q} | {name} | first sampled column equal over the routings | {'yes' if len(firsts) == 1 else 'no (reordered sums)'} | | | | | |")
    emit("")
    emit("## Decision rule")
    emit("")
    for q, name, gain, sp, best, cc in verdict:
        emit(f"- {q} / {name}: the skinny route (routing {best}) is {gain:+.3f} ms against the old routing; the larger "
             f"spread of the two is {sp:.3f} ms -> {'faster by more than the spread' if gain > sp else 'NOT faster by more than the spread'}."
             + ("" if cc is None else f"  Codes against the bf16 copy: {cc[0]:+.3f} ms (spread {cc[1]:.3f}) -> "
                f"{'codes at least as fast' if cc[0] >= -cc[1] else 'the copy is faster by more than the spread'}."))
    return lines


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace()
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        with open(sys.argv[3], "w") as f:
            json.dump(step(sys.argv[2]), f)
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    base = os.path.splitext(out_path)[0] if out_path else os.path.join(ROOT, "bench_out", "prompt_q")
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    res = {}
    for quant in QUANTS:
        js = f"{base}.{quant}.json"
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", quant, js]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {quant} ended with status {rc}: stopping", flush=True)
            return rc
        with open(js) as f:
            res[quant] = json.load(f)
    lines = report(res)
    print("\n".join(lines), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
