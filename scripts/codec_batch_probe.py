"""Batched streamed vocoding against the serial path it replaces, S2-Pro codec config, bf16:
    python3 scripts/codec_batch_probe.py [--out profiles/codec_batch.md] [--reps 5]

Per cell (n streams, T frames each): the wall time of ONE fm_codec_stream_decode_batch call and of the
n fm_codec_stream_decode calls it replaces, same process, same handle, same contexts, repeats
interleaved (serial, batched, serial, ...) after one warm-up of each form.  Both forms end in the
codec's stream synchronise, so the host clock covers the device work.  The last listener's PCM is
complete when the serial loop ends (its "total") or when the batched call returns, so those two are
the queueing figure; the first listener's serial time is printed beside them, because batching makes
the first listener wait for the whole pass.  All contexts sit past the 128-frame window (npre = 127)
before the first cell, so every cell runs the steady-state attention.
A difference counts when it exceeds three times the serial baseline's spread (max - min)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))

NS, TS = (1, 4, 8, 16, 32), (1, 8, 21, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_batch.md"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert a.reps >= 3

    from fishmi.codec import FishMICodec
    from fishmi.config import CodecConfig

    ccfg = CodecConfig()
    C1 = ccfg.n_codebooks + 1
    m = FishMICodec.synthetic(ccfg, 1, 0, "bf16", max_frames=max(NS) * max(TS) + 8 * (max(NS) - 1))
    gap = m.batch_gap
    assert max(NS) * max(TS) + gap * (max(NS) - 1) <= m.max_frames
    rng = np.random.default_rng(0)

    def codes(T):
        c = rng.integers(0, ccfg.codebook_size, (C1, T)).astype(np.int32)
        c[0] = rng.integers(0, ccfg.semantic_codebook_size, T)
        return c

    # the S2-Pro shapes take other kernel variants than the test fixture: check the bits here too
    A = [m.open_stream() for _ in range(4)]
    B = [m.open_stream() for _ in range(4)]
    same = True
    for Ts in ((1, 8, 21, 128), (130, 3, 1, 40), (5, 5, 5, 5)):
        ch = [codes(T) for T in Ts]
        one = [s.decode_chunk(c) for s, c in zip(A, ch)]
        bat = m._decode_batch([s.sid for s in B], ch)
        same = same and all(np.array_equal(x, y) for x, y in zip(one, bat))
    for s in A + B:
        s.close()
    if not same:
        raise SystemExit("batched PCM differs from the serial path at the S2-Pro config")

    ctx = [m.open_stream() for _ in range(max(NS))]
    m.decode_chunks(ctx, [codes(128) for _ in ctx])  # every context past the window

    lines = ["# Batched streamed vocoding vs the serial path (S2-Pro codec config, bf16)", "",
             f"`scripts/codec_batch_probe.py`, {a.reps} interleaved repeats per cell after one warm-up of each form; "
             f"gap {gap} frames; batched PCM bit-identical to the serial path at this config: {same}.", "",
             "Times in ms, mean (max - min).  serial = the n `fm_codec_stream_decode` calls (the last listener's PCM "
             "is complete at its end), first = the first of them, batched = one `fm_codec_stream_decode_batch` call.  "
             "Verdict: the difference of the means against 3 x the serial spread.", "",
             "| n | T | serial | first | batched | serial / batched | verdict |", "|---|---|---|---|---|---|---|"]
    for n in NS:
        for T in TS:
            st = ctx[:n]
            sids = [s.sid for s in st]
            ser, first, bat = [], [], []
            for rep in range(a.reps + 1):
                ch = [codes(T) for _ in st]
                t0 = time.perf_counter()
                st[0].decode_chunk(ch[0])
                t1 = time.perf_counter()
                for s, c in zip(st[1:], ch[1:]):
                    s.decode_chunk(c)
                t2 = time.perf_counter()
                ch = [codes(T) for _ in st]
                t3 = time.perf_counter()
                m._decode_batch(sids, ch)  # (the native batched call, n = 1 included)
                t4 = time.perf_counter()
                if rep:  # rep 0 warms both forms up at this shape
                    first.append((t1 - t0) * 1e3)
                    ser.append((t2 - t0) * 1e3)
                    bat.append((t4 - t3) * 1e3)
            sm, bm, sp = np.mean(ser), np.mean(bat), max(ser) - min(ser)
            verdict = "batched wins" if sm - bm > 3 * sp else ("batched loses" if bm - sm > 3 * sp else "no difference")
            lines.append(f"| {n} | {T} | {sm:.3f} ({sp:.3f}) | {np.mean(first):.3f} ({max(first) - min(first):.3f}) | "
                         f"{bm:.3f} ({max(bat) - min(bat):.3f}) | {sm / bm:.2f} | {verdict} |")
            print(lines[-1], flush=True)
    for s in ctx:
        s.close()
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
