"""The prefill of weight-only int8 / int4 (groups of 128) models at synthetic S2-Pro widths, prompts of 128, 256, 646
and 1024 tokens (one chunk each), under the routings of their linears of more than 64 rows (fm_tune prompt_gemm_q):
0 the 16-row tile kernel (the routing before the tiled prompt GEMMs took quantised linears), 1 the tiled GEMMs reading
what the handle's linears read before (the bf16 copy; a compact handle's codes), 2 the tiled GEMMs on the codes
wherever the handle has them.  Per quantisation one child process builds two handles from the same seed -- one opened
with 12 slots (bf16 copy and step-granular codes: 0, 1, 2) and a compact one (codes only).  A compact handle ignores
prompt_gemm_q 0, so its baseline leg is fm_tune prompt_gemm 0, which sends every prompt linear to linear(): at these
row counts that is the tile kernel's code form on all four linears, the routing before (leg "0" of that handle).
A third child times the unquantised bf16 model at the same lengths, as the context line.  Method as
scripts/prompt_q_probe.py: every leg warmed up, then timed interleaved, three repeats of PREFILLS prefills; the time
is the host clock around fm_llm_prefill, which ends in a stream synchronise.

`--trace` runs two 646-token prefills per routing of the 12-slot handles only, for one separate
`rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/prompt_gemm_q_probe.py --trace` run, and
`--spans <results.db | kernel_trace.csv>` tabulates that run's GEMM launches per linear (wqkv, wo, w1 || w3, w2 by
their order inside a layer, a split-K epilogue counted with its GEMM).

The driver runs each GPU step as a child process of its own under `timeout -k 10` and stops at the first non-zero
status.  Usage: python scripts/prompt_gemm_q_probe.py [out.md]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))

LENS, PREFILLS, REPS = (128, 256, 646, 1024), 8, 3
DECIDE_AT = 646  # the benchmark's clone prompt: the default rule is read at this length
QUANTS = ("int8", "int4")
ROUTES = {0: "tile kernel (old routing)", 1: "tiled GEMM, the handle's own form", 2: "tiled GEMM, codes"}
LIMIT = 420  # seconds per step
LINEARS = ("wqkv", "wo", "w1||w3", "w2")


def _setup(quant, handles):
    import numpy as np

    from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig
    from fishmi.llm import DualARModel

    cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
    cfg.im_end_id = S2_PRO_IM_END_ID
    cfg.max_seq_len = 2048
    rng = np.random.default_rng(3)
    prompts = {}
    for T in LENS:
        p = np.zeros((cfg.num_codebooks + 1, T), np.int32)
        p[0] = rng.integers(16, cfg.semantic_begin_id, T)
        prompts[T] = p
    legs = {}
    for name in handles:
        compact = name == "compact"
        legs[name] = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16",
                                           max_slots=1 if compact else 12, quant=quant, groupsize=128, compact=compact)
    return cfg, prompts, legs, DualARModel.sampling(top_k=1)


def _routes(name):
    return (0, 1) if name in ("compact", "bf16") else (0, 1, 2)


def _route(name, r):
    """put routing r of handle `name` in force"""
    from fishmi import native

    native.tune("prompt_gemm", 0 if (name == "compact" and r == 0) else 1)
    native.tune("prompt_gemm_q", r)


def step(quant):
    from fishmi import native

    bf16 = quant == "bf16"
    cfg, prompts, legs, sp = _setup(None if bf16 else quant, ("bf16",) if bf16 else ("copy", "compact"))
    routes = (lambda n: (1,)) if bf16 else _routes
    res = {n: {str(T): {str(r): {"ms": [], "first": None} for r in routes(n)} for T in LENS} for n in legs}
    try:
        for rep in range(REPS + 1):  # round 0 warms every leg up and is not reported
            for T in LENS:
                for name, m in legs.items():
                    for r in routes(name):
                        _route(name, r)
                        t0 = time.perf_counter()
                        for _ in range(PREFILLS):
                            col = m.prefill(0, prompts[T], sp)
                        dt = (time.perf_counter() - t0) / PREFILLS * 1e3
                        if rep:
                            res[name][str(T)][str(r)]["ms"].append(dt)
                        res[name][str(T)][str(r)]["first"] = [int(c) for c in col]
                        print(f"{quant} {name} T={T} routing {r} round {rep}: {dt:.3f} ms", flush=True)
        for name, m in legs.items():  # device time of the linears, one profiled prefill per leg at DECIDE_AT
            for r in routes(name):
                _route(name, r)
                m.profile(True)
                m.prefill(0, prompts[DECIDE_AT], sp)
                ms, n, b = m.profile_read("linear")
                res[name][str(DECIDE_AT)][str(r)].update(linear_ms=ms, linear_launches=n, linear_bytes=b,
                                                         prompt_gq_launches=m.profile_read("prompt_gq")[1])
                m.profile(False)
    finally:
        native.tune("prompt_gemm", 1)
        native.tune("prompt_gemm_q", 1)
        for m in legs.values():
            m.close()
    return res


def trace():
    for quant in QUANTS:
        cfg, prompts, legs, sp = _setup(quant, ("copy",))
        for r in _routes("copy"):
            _route("copy", r)
            for _ in range(2):  # (the first one of a routing loads its code objects)
                legs["copy"].prefill(0, prompts[DECIDE_AT], sp)
        legs["copy"].close()
    print("ok")


def spans(path):
    """per (model, routing, linear): the GEMM kernel, its grid in blocks, and the mean device time of the launch with
    its split-K epilogue -- from the second prefill of each routing of `--trace` (quantisations and routings in the
    order trace() runs them; every layer launches wqkv, wo, w1 || w3, w2 in this order)"""
    import csv
    import re
    import sqlite3

    rows = []
    if path.endswith(".db"):
        c = sqlite3.connect(path)
        try:
            q = c.execute("select name, start, end, grid_x, grid_y, grid_z, workgroup_x from kernels order by start").fetchall()
        except sqlite3.OperationalError:  # (no workgroup column: grid x stays in threads)
            q = [r + (1,) for r in c.execute("select name, start, end, grid_x, grid_y, grid_z from kernels order by start")]
        for name, s, e, gx, gy, gz, wx in q:
            rows.append((name, s, e, (gx // max(wx, 1), gy, gz)))
    else:
        with open(path) as fh:
            for r in csv.DictReader(fh):
                wx = max(int(r.get("Workgroup_Size_X", 1)), 1)
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                             (int(r["Grid_Size_X"]) // wx, int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))))
        rows.sort(key=lambda r: r[1])
    short = lambda n: re.sub(r"^void ", "", n).split("(")[0].replace("unsigned short", "bf16")  # noqa: E731
    gemm = lambda n: "conv_gemm" in n or ("linear_kernel" in n)  # noqa: E731
    launches = []  # [name, grid, ns] of every prompt-pass GEMM, its epilogue added
    for name, s, e, grid in rows:
        if gemm(name):
            launches.append([short(name), grid, e - s])
        elif "conv_splitk_epi_kernel" in name and launches:
            launches[-1][2] += e - s
            launches[-1][0] += " + split-K epilogue"
    from fishmi.config import S2_PRO_CONFIG, DualARConfig

    per = 4 * DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG).n_layer  # GEMM launches of one prefill
    legs = [(q, r) for q in QUANTS for r in _routes("copy")]
    lines = ["| model | routing | linear | kernel | grid (blocks) | mean us per launch |", "|---|---|---|---|---|---|"]
    if len(launches) != per * 2 * len(legs):
        lines = [f"(expected {per * 2 * len(legs)} prompt GEMM launches, found {len(launches)}: not attributed to linears)",
                 "", "| kernel | grid | launches | mean us |", "|---|---|---|---|"]
        agg = {}
        for n, g, ns in launches:
            agg.setdefault((n, g), []).append(ns)
        return lines + [f"| {n} | {g} | {len(v)} | {sum(v) / len(v) / 1e3:.1f} |" for (n, g), v in sorted(agg.items())]
    for i, (q, r) in enumerate(legs):
        second = launches[(2 * i + 1) * per:(2 * i + 2) * per]
        for j, lin in enumerate(LINEARS):
            mine = second[j::4]
            kinds = sorted({(m[0], m[1]) for m in mine})
            us = sum(m[2] for m in mine) / len(mine) / 1e3
            lines.append(f"| {q} | {r} | {lin} | {'; '.join(k[0] for k in kinds)} | {'; '.join(str(k[1]) for k in kinds)} | {us:.1f} |")
    return lines


def report(res, ctx):
    lines = []
    emit = lines.append
    emit("# Quantised prefill of more than 64 rows: the linears on the tile kernel and on the tiled prompt GEMMs (MI355X)")
    emit("")
    emit(f"Synthetic S2-Pro widths (max_seq_len 2048), weight-only int8 and int4 (groups of 128).  `copy`: a handle "
         f"opened with 12 slots (bf16 fragment copy and step-granular codes); `compact`: codes only.  fm_tune "
         f"prompt_gemm_q picks the routing (the compact handle's routing 0 is fm_tune prompt_gemm 0: it ignores "
         f"prompt_gemm_q 0).  Each figure: the mean over {REPS} interleaved repeats of the mean wall time of {PREFILLS} "
         f"fm_llm_prefill calls (each ends in a stream synchronise); spread = max - min of the repeats.  linear: the "
         f"\"linear\" class of one profiled {DECIDE_AT}-token prefill (HIP events around every launch; the prompt "
         f"pass's and the first frame's linears): device ms, launches, booked MB.")
    emit("")
    emit("Context, the unquantised bf16 model in the same run: " + ", ".join(
        f"{T} tokens {sum(v['1']['ms']) / len(v['1']['ms']):.3f} ms (spread {max(v['1']['ms']) - min(v['1']['ms']):.3f})"
        for T, v in ((T, ctx["bf16"][str(T)]) for T in LENS)) + ".")
    emit("")
    emit("| model | handle | tokens | routing | prefill ms (spread) | vs routing 0 | linear ms | launches | MB | prompt_gq launches |")
    emit("|---|---|---|---|---|---|---|---|---|---|")
    verdict = []
    for q, r in res.items():
        for name, by_len in r.items():
            for T in LENS:
                legs = by_len[str(T)]
                mean = {k: sum(v["ms"]) / len(v["ms"]) for k, v in legs.items()}
                spread = {k: max(v["ms"]) - min(v["ms"]) for k, v in legs.items()}
                for k, v in legs.items():
                    prof = (f"{v['linear_ms']:.3f} | {v['linear_launches']} | {v['linear_bytes'] / 1e6:.1f} | "
                            f"{v['prompt_gq_launches']}") if "linear_ms" in v else " | | | "
                    emit(f"| {q} | {name} | {T} | {k}: {ROUTES[int(k)]} | {mean[k]:.3f} ({spread[k]:.3f}) | "
                         f"{mean[k] / mean['0']:.3f} | {prof} |")
                if T == DECIDE_AT:
                    verdict.append((q, name, mean["0"] - mean["1"], max(spread["0"], spread["1"]),
                                    None if "2" not in legs else (mean["1"] - mean["2"], max(spread["1"], spread["2"]))))
                firsts = {tuple(v["first"]) for k, v in legs.items() if k != "0"}
                emit(f"| {q} | {name} | {T} | first sampled column equal over routings 1 / 2 | "
                     f"{'yes' if len(firsts) == 1 else 'NO'} | | | | | |")
    emit("")
    emit(f"## Default rule (read at {DECIDE_AT} tokens)")
    emit("")
    ok = True
    for q, name, gain, sp, cc in verdict:
        ok = ok and gain > sp
        emit(f"- {q} / {name}: routing 1 is {gain:+.3f} ms against routing 0; the larger spread of the two is {sp:.3f} ms "
             f"-> {'faster by more than the spread' if gain > sp else 'NOT faster by more than the spread'}."
             + ("" if cc is None else f"  Routing 2 (codes) against routing 1 (bf16 copy): {cc[0]:+.3f} ms "
                f"(spread {cc[1]:.3f})."))
    emit("")
    emit(f"Routing 1 {'is' if ok else 'is NOT'} faster than routing 0 by more than the repeats' spread on all four handles.")
    return lines


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace()
        return 0
    if len(sys.argv) > 2 and sys.argv[1] == "--spans":
        print("\n".join(spans(sys.argv[2])), flush=True)
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        with open(sys.argv[3], "w") as f:
            json.dump(step(sys.argv[2]), f)
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    base = os.path.splitext(out_path)[0] if out_path else os.path.join(ROOT, "bench_out", "prompt_gemm_q")
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    res = {}
    for quant in QUANTS + ("bf16",):
        js = f"{base}.{quant}.json"
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", quant, js]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {quant} ended with status {rc}: stopping", flush=True)
            return rc
        with open(js) as f:
            res[quant] = json.load(f)
    ctx = res.pop("bf16")
    lines = report(res, ctx)
    print("\n".join(lines), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
