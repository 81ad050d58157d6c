"""Voice prefix cache at S2-Pro widths (synthetic bf16 weights, 36 layers): what a request saves when
its voice's prompt KV is copied into the slot instead of being prefilled.

A 646-position voice block (BASELINE config 5's clone prompt) followed by a 40-token text:
  1. time to the first column of one request: prefill of the whole prompt (the only path without
     the cache) against load_prefix + prefill of the text at pos0 = 646;
  2. the same for 32 requests starting together: prefill_batch of the whole prompts against one
     32-slot load_prefix + prefill_batch(pos0=...);
  3. the copy alone (save, load into 1 slot, load into 32 slots): bytes read + written over the host
     wall time of the call (slot list upload, one launch, stream synchronise), beside
     fm_stream_peak's copy figure from the same run.
Every timing is a host clock around calls that end in a stream synchronise; the two sides of a
comparison alternate inside one loop.  Run by hand on the GPU:
  python scripts/voice_cache_probe.py [reps]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech_amd"))
from fishmi import native  # noqa: E402
from fishmi.config import S2_PRO_CONFIG, S2_PRO_IM_END_ID, DualARConfig  # noqa: E402
from fishmi.llm import DualARModel  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
VOICE, TEXT, B = 646, 40, 32


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def report(name, ms):
    print(f"  {name:58s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms   (n={len(ms)})", flush=True)


cfg = DualARConfig._from_fish_qwen3_omni(S2_PRO_CONFIG)
cfg.im_end_id = S2_PRO_IM_END_ID
cfg.max_seq_len = 1024
m = DualARModel.synthetic(cfg, seed=0, log2_half=5, device=0, precision="bf16", max_slots=B)
rng = np.random.default_rng(7)
full = np.zeros((cfg.num_codebooks + 1, VOICE + TEXT), np.int32)
full[0] = rng.integers(16, cfg.semantic_begin_id, VOICE + TEXT)
full[0, 100:VOICE] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, VOICE - 100)  # the reference codes
full[1:, 100:VOICE] = rng.integers(0, cfg.codebook_size, (cfg.num_codebooks, VOICE - 100))
text = full[:, VOICE:]
sp = DualARModel.sampling(top_k=1, mask_im_end=True)
slots = list(range(B))

first_full = m.prefill(0, full, sp)
pid = m.save_prefix(0, VOICE)
npos, nbytes = m.prefix_info(pid)
m.load_prefix(pid, [0])
first_cached = m.prefill(0, text, sp, pos0=VOICE)
print(f"voice {npos} positions = {nbytes / 1e6:.1f} MB of slow-stack KV; text {TEXT} tokens; "
      f"first column equal on both paths: {bool(np.array_equal(first_full, first_cached))}", flush=True)

print("1. one request, time to the first column", flush=True)
a, b, c = [], [], []
for _ in range(REPS):
    a.append(timed(lambda: m.prefill(0, full, sp))[0])
    t_load = timed(lambda: m.load_prefix(pid, [0]))[0]
    t_pre = timed(lambda: m.prefill(0, text, sp, pos0=VOICE))[0]
    b.append(t_load + t_pre)
    c.append(t_load)
report(f"prefill of the whole prompt ({VOICE + TEXT} positions)", a)
report(f"load_prefix + prefill of the text at pos0 = {VOICE}", b)
report("  of which load_prefix", c)

print(f"2. {B} requests starting together, time to the first columns", flush=True)
m.prefill_batch(slots, [full] * B, [sp] * B)
m.load_prefix(pid, slots)
m.prefill_batch(slots, [text] * B, [sp] * B, pos0=[VOICE] * B)
a, b, c = [], [], []
for _ in range(max(3, REPS // 3)):
    a.append(timed(lambda: m.prefill_batch(slots, [full] * B, [sp] * B))[0])
    t_load = timed(lambda: m.load_prefix(pid, slots))[0]
    t_pre = timed(lambda: m.prefill_batch(slots, [text] * B, [sp] * B, pos0=[VOICE] * B))[0]
    b.append(t_load + t_pre)
    c.append(t_load)
report("prefill_batch of the whole prompts", a)
report("one load_prefix of all slots + prefill_batch(pos0)", b)
report("  of which load_prefix", c)

print("3. the copy alone (host wall of the call: slot list upload + one launch + synchronise)", flush=True)
m.prefill(0, full, sp)
for name, f, moved in (("save_prefix (slot -> store)", None, 2 * nbytes),
                       ("load_prefix into 1 slot", lambda: m.load_prefix(pid, [0]), 2 * nbytes),
                       (f"load_prefix into {B} slots", lambda: m.load_prefix(pid, slots), 2 * nbytes * B)):
    ms = []
    for _ in range(REPS):
        if f is None:
            t, p2 = timed(lambda: m.save_prefix(0, VOICE))  # includes the entry's hipMalloc
            m.drop_prefix(p2)
        else:
            t, _ = timed(f)
        ms.append(t)
    report(name, ms)
    print(f"    {moved / 1e6:.1f} MB read + written: {moved / statistics.median(ms) / 1e6:.0f} GB/s at the median, "
          f"{moved / min(ms) / 1e6:.0f} GB/s at the minimum", flush=True)
rd, cp = native.stream_peak(0, 2 << 30, 10)
print(f"fm_stream_peak in this run: read {rd:.0f} GB/s, copy {cp:.0f} GB/s (read + written)", flush=True)
m.drop_prefix(pid)
m.close()
