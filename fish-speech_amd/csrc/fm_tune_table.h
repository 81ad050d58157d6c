// fm_tune_table.h -- the one list of the fm_tune developer knobs: FM_KNOB(name, default, accepted values)
// and the knob's comment.  Everything else is generated from it: the FmTuning fields (fm_kernels.h; in
// this order, all int), and fm_tune / fm_tune_get (fm_llm_dev.cpp: look the key up, validate, store).
// Included twice: plainly for the rule vocabulary below, and with FM_KNOB defined for the list.
// ("debug_ts" is no entry: it allocates FmTuning::dbg and leaves FmTuning::epoch alone.)
#ifndef FM_TUNE_RULES
#define FM_TUNE_RULES
enum { FM_RULE_BOOL, FM_RULE_ANY, FM_RULE_SET, FM_RULE_RANGE, FM_RULE_MULT16 };
template <typename... V> constexpr int fm_knob_set(V... v) { return (0 | ... | (1 << v)); }
// accepted values of a knob, as (rule, a, b)
#define FM_BOOL FM_RULE_BOOL, 0, 0                      /* any value, stored as value != 0 */
#define FM_ANY FM_RULE_ANY, 0, 0                        /* any value, stored as given */
#define FM_SET(...) FM_RULE_SET, fm_knob_set(__VA_ARGS__), 0 /* one of the listed values (each 0..30) */
#define FM_RANGE(lo, hi) FM_RULE_RANGE, lo, hi          /* lo <= value <= hi */
#define FM_MIN(lo) FM_RULE_RANGE, lo, 0x7fffffff        /* value >= lo */
#define FM_MULT16 FM_RULE_MULT16, 0, 0                  /* a multiple of 16, >= 16 */
#define FM_ZERO_OR_MULT16 FM_RULE_MULT16, 1, 0          /* 0, or a multiple of 16 */
#endif

// A compact handle (fm_llm_set_quant_compact: no bf16 copy of its quantised linears) ignores the knobs that would
// pick a reader of that copy -- bstream 0, bstream_acc 0, bstream_chain 1, bstream_q8 0, bstream_q4 0, int4_stream 0
// -- and keeps its default routing (prompt_skinny_q 0 and prompt_gemm_q 0 it runs as 1); other handles in the process keep the knobs'
// meaning (include/fishmi.h, fm_tune).
#ifdef FM_KNOB
FM_KNOB(gemv_nt, 1, FM_BOOL)               // 1: non-temporal weight loads (each weight byte is read once a frame)
FM_KNOB(gemv_u, 8, FM_SET(2, 4, 8))        // weight fragments in flight per wave (2, 4 or 8)
FM_KNOB(gemv_wpb, 4, FM_SET(4, 8))         // waves per block (4 or 8) sharing one 16-row tile
FM_KNOB(sampler_kth, 1, FM_BOOL)           // sample_fast_kernel: the K-th lane maximum as the wave threshold when its candidates fit (else the radix search)
FM_KNOB(sampler_fast, 1, FM_BOOL)          // 1: two-stage register top-K sampler, 0: LDS radix-select sampler
FM_KNOB(attn_cap, 32, FM_ZERO_OR_MULT16)   // slow decode attention rows per block cap (0: the LDS-budget maximum)
FM_KNOB(attn_wo, 0, FM_BOOL)               // 1: fast-model attention recomputed in the Wo GEMV's prologue (PRO_FATT, R == 1; measured 0.37 ms/frame slower)
FM_KNOB(ksb_blocks, 512, FM_MIN(1))        // split K until the grid has at least this many blocks
FM_KNOB(batched_fused_attn, 1, FM_BOOL)    // batched decode (one row per slot): fused QK-norm/RoPE/KV-write attention kernels
FM_KNOB(attn_cap_batched, 128, FM_ZERO_OR_MULT16)  // rows per block of the batched decode attention (one row per slot)
FM_KNOB(linear_u32, 4, FM_SET(4, 8))       // linear_kernel weight fragments in flight per wave at 16 < R <= 32 (4 or 8)
FM_KNOB(linear_fill, 0, FM_MIN(0))         // batched linear_kernel: split K until this many blocks (0: never; measured slower)
FM_KNOB(attn3, 1, FM_BOOL)                 // 1: slow decode attention on attn_dec3_kernel, 0: attn_decode2_kernel
FM_KNOB(attn_fd, 1, FM_BOOL)               // 1: slow decode attention on attn_fd_kernel (flash-decode splits) where eligible
FM_KNOB(fd_min, 32, FM_MULT16)             // attn_fd: minimum positions per split at R <= 8
FM_KNOB(fd_min_batched, 512, FM_MULT16)    // attn_fd: minimum positions per split at R > 8 (B=32: one split below 512)
FM_KNOB(fd_nw, 8, FM_SET(4, 8, 16))        // attn_fd at R <= 8: waves per block (4, 8 or 16) ...
FM_KNOB(fin_ksb, 0, FM_RANGE(0, 8))        // batch-1 wo / w2 (EPI_SLABFIN) split-K factor (0: whole K whenever the x slice fits LDS; at most KSB_MAX)
FM_KNOB(fd_nw_batched, 4, FM_SET(4, 8, 16))  // attn_fd at R > 8: waves per block (4, 8 or 16)
FM_KNOB(fd_min16, 256, FM_MULT16)          // ... and splits of at least this many positions (8 or 16 waves; below it
                                           // one block per kv head, no cross-block combine)
FM_KNOB(fd_hpb, 1, FM_SET(1, 2, 4))        // attn_fd at R <= 8: q heads of a kv head per block (4: all of them, one block per kv head and
                                           // split); fewer spread the same arithmetic over more CUs (bit-identical)
FM_KNOB(prefill_attn, 1, FM_BOOL)          // 1: prompt-chunk attention on attn_prefill_kernel (bf16, head_dim 128, flash form)
FM_KNOB(prompt_gemm, 1, FM_BOOL)           // 1: prompt-chunk linears (R > 32) on the codec's LDS-tiled GEMM kernels
FM_KNOB(prompt_skinny, 1, FM_BOOL)         // prompt linears at 32 < R <= 64 rows (bf16) on prompt_skinny_kernel ...
FM_KNOB(prompt_skinny_blocks, 256, FM_MIN(1))  // ... with K sliced until its 64-row blocks number >= this
FM_KNOB(prompt_unroll, 1, FM_BOOL)         // skinny prompt GEMM: the fully unrolled form (5 / 10 / 20-chunk slices)
FM_KNOB(prompt_qkv_slab, 1, FM_BOOL)       // skinny QKV: slabs summed by qk_rope_cache_kernel (no epilogue launch)
FM_KNOB(prompt_fin, 1, FM_BOOL)            // skinny wo / w2: slabs finished by finalize_norm with the next RMSNorm
FM_KNOB(prompt_swiglu, 1, FM_BOOL)         // skinny w1 || w3: the SwiGLU in its split-K epilogue (no separate launch)
FM_KNOB(prompt_skinny_q, 1, FM_RANGE(0, 2))  // weight-only int8 / int4 (bf16 handles), 32 < R <= 64 rows: the skinny prompt GEMM streams 1 the step-granular
                                           // codes where the handle has them (compact, or opened with > 8 slots; int4: group size a multiple of 128), 0 the
                                           // bf16 fragment copy (int8: with the row scales in the epilogues; a compact handle has none and keeps the codes);
                                           // 2: no skinny GEMM for quantised linears -- linear_kernel, as before (bit-identical 0 / 1; profiles/prompt_q.md)
FM_KNOB(prompt_gemm_q, 1, FM_RANGE(0, 2))  // weight-only int8 / int4 (bf16 handles), linears of more than 64 prompt rows: 1 the tiled prompt GEMMs with the
                                           // bf16 model's K split, reading what linear() reads for the handle -- the bf16 fragment copy (int8: the row scales
                                           // in the epilogues), or a compact handle's step-granular codes; 2 the codes wherever the handle has them (> 8
                                           // slots; for measurement); 0 linear_kernel, as before (a compact handle runs 0 as 1; bit-identical 1 / 2)
FM_KNOB(prompt_ks_tiles, 384, FM_MIN(1))   // prompt GEMM: split K until ceil(R/128) ceil(N/128) ks reaches this ...
FM_KNOB(prompt_ks_max, 8, FM_SET(1, 2, 4, 8))  // ... or ks this (fp32 slabs + the conv split-K epilogue)
FM_KNOB(conv2, 1, FM_BOOL)                 // 1: codec GEMMs on the LDS-staged conv_gemm2_kernel, 0: conv_gemm_kernel
FM_KNOB(conv_splitk, 1, FM_BOOL)           // 1: small-grid codec GEMMs split K into fp32 slabs + a reduce/epilogue kernel
FM_KNOB(resunit_cfg, 1, FM_RANGE(0, 2))    // resunit_kernel tile at 192 / 96 channels: 0 (BM 128 / 256, 8 time tiles per wave), 1 (BM 64 / 128, 4 tiles), 2 (128 / 128)
FM_KNOB(resunit_enc, 1, FM_BOOL)           // 1: the encoder's units (64 / 128 / 256 / 512 channels) fused as well
FM_KNOB(resunit_384, 1, FM_BOOL)           // 1: the 384-channel stage's units fused too (BM 64, 8 waves)
FM_KNOB(codec_norm, 1, FM_BOOL)            // 1: the codec transformer's RMSNorms in the wo / w2 split-K epilogues (no rmsnorm launch)
FM_KNOB(codec_rope, 1, FM_BOOL)            // 1: the codec transformer's RoPE in the wqkv split-K epilogue (no rope_qk launch)
FM_KNOB(codec_swiglu, 1, FM_BOOL)          // 1: codec FeedForward W1 | W3 as one split-K GEMM with the SwiGLU epilogue
FM_KNOB(codec_fuse, 1, FM_BOOL)            // 1: decoder ResidualUnits at 96 / 192 / 384 channels as one resunit_kernel launch (k7 + k1)
FM_KNOB(bstream, 1, FM_BOOL)               // 1: batched decode linears (8 < R <= 32) on bstream_kernel (fm_bstream.hip)
FM_KNOB(bstream_kparts, 0, FM_SET(0, 1, 2, 4, 8))  // bstream EPI_SLAB K parts (0: by K)
FM_KNOB(bstream_nw, 0, FM_RANGE(0, 16))    // bstream waves per block (0: 16 whole-K, 8 split-K)
// ring slots past a wave's run (tail of the decode GEMV ring, bsacc tiles / steps a block does
// not own): 0 re-load the run's last fragment, 1 one fixed fragment, 2 a fixed fragment per
// (block, wave) over 256 of them.  B=1 frame 4.447 / 4.47 / 4.398 ms, B=32 6.51 / 6.44 / 6.42 ms
FM_KNOB(bs_dummy, 2, FM_RANGE(0, 2))
FM_KNOB(gemv_dummy, 2, FM_RANGE(0, 2))
FM_KNOB(bs_qkv_slab, 1, FM_BOOL)           // batched frames: QKV as K-part slabs summed by the attention (balanced
                                           // grid: 384 tiles x 2 K parts over 256 CUs; B=32 frame 6.48 -> 6.33 ms)
FM_KNOB(fast_tail, 1, FM_BOOL)             // 1: codebook 0's fast pass stops its last layer after the K / V cache write (its output is discarded)
FM_KNOB(fkv_prefetch, 0, FM_BOOL)          // 1: the batch-1 fast-model QKV GEMV pulls the fast attention's cached rows into L2 too
FM_KNOB(kv_prefetch, 1, FM_BOOL)           // 1: the batch-1 QKV GEMV pulls the next attention's K / V rows into L2
FM_KNOB(bstream_chain, 0, FM_ANY)          // 1: bsacc SLABFIN / PRENORM chain instead of finalize_norm launches (measured 6.31 -> 6.75 ms per B=32 frame)
FM_KNOB(bstream_acc, 1, FM_ANY)            // 1: bsacc_kernel (per-tile register accumulators, one reduction at the end, balanced K parts); 0: bstream_kernel
FM_KNOB(rmsnorm_block, 0, FM_BOOL)         // 1: block-per-row RMSNorm (the pre-vectorisation kernel), 0: wave-per-row when shapes allow
FM_KNOB(ksb_balance, 0, FM_BOOL)           // 1: prefer grids that are whole multiples of 256 blocks (one per CU)
FM_KNOB(chain_max, 4, FM_RANGE(2, 4))      // gemv_chain: GEMVs per launch at most (2..GEMV_CHAIN_MAX)
FM_KNOB(chain_sleep, 4, FM_SET(1, 4, 16))  // gemv_chain: s_sleep argument between a waiting block's polls (1, 4 or 16)
FM_KNOB(gemv_chain, 0, FM_BOOL)            // 1: batch-1 decode runs wo -> w1||w3 -> w2 -> next qkv as one launch (gemv_chain_kernel)
FM_KNOB(bs_xfirst, 1, FM_BOOL)             // bsacc: X operands before the weight ring (B=32 frame 6.48 -> 6.36 ms)
FM_KNOB(bs_vec_epi, 1, FM_BOOL)            // bsacc: 4-row epilogue items (bit-identical to the scalar epilogue; B=32 frame 6.31 -> 6.18 ms)
FM_KNOB(bsacc_kparts, 0, FM_SET(0, 1, 2, 4, 8))  // developer: force the K parts of the batched split-K (slab) linears (0: bsacc_plan's pick)
FM_KNOB(q_u, 4, FM_SET(2, 4, 8, 16))       // int8 / int4 decode GEMV: ring units in flight per wave (2, 4, 8, 16; int8 frame 3.79 -> 3.59 ms at 8 -> 4)
FM_KNOB(fin8, 1, FM_BOOL)                  // finalize_norm: all eight K parts' slab loads in one round trip (0: two batches of four)
FM_KNOB(fin_split, 0, FM_RANGE(0, 16))     // batched finalize_norm: each row over this many blocks (0 / 1: one block per row)
FM_KNOB(bstream_q8, 1, FM_BOOL)            // weight-only int8, 8 < R <= 32: 1 bsacc_kernel streams the int8 codes, 0 their bf16 fragment copy
                                           // (bit-identical; int8 B=32 frame 6.441 -> 5.761 ms, the bf16 model's 6.184; profiles/b32_int8.md)
FM_KNOB(bstream_q4, 1, FM_BOOL)            // weight-only int4 (group size a multiple of 128), 8 < R <= 32: 1 bsacc_kernel streams the 4-bit codes and their
                                           // (scale, zero) words, 0 the dequantised bf16 fragment copy (bit-identical; int4 B=32 frame 6.343 -> 5.848 ms;
                                           // profiles/b32_int4.md); int4_stream 0 switches it off too
FM_KNOB(int4_stream, 1, FM_BOOL)           // weight-only int4: 1 the batch <= 8 GEMVs stream the 4-bit codes, 0 the dequantised bf16 copy
FM_KNOB(fw_delay, 0, FM_RANGE(0, 1000))    // fattn_wo: FattnWoArgs::delay (10-ns ticks)
FM_KNOB(fw_cheap, 0, FM_BOOL)              // fattn_wo: FattnWoArgs::cheap
FM_KNOB(fw_prio, 0, FM_BOOL)               // fattn_wo: FattnWoArgs::prio
FM_KNOB(fattn_wo, 1, FM_BOOL)              // 1: batch-1 bf16 fast-model attention + wo as one launch (fm_rowgemv.hip fattn_wo_kernel)
FM_KNOB(fattn_ilp, 1, FM_BOOL)             // 1: fattn_wo_kernel's attention chain without serial blocks: q / k prep chains side by side, score /
                                           // softmax / PV over a compile-time position count, the softmax one position per lane (bit-identical
                                           // to 0, the early-exit loops)
FM_KNOB(row_qkv_rp, 8, FM_SET(4, 8, 16))   // developer: rows per block of the bf16 row-block wqkv (4, 8 or 16)
FM_KNOB(rowgemv_q4, 31, FM_RANGE(0, 31))   // rowgemv's bits for weight-only int4 models (w1 || w3 too: int4 frame 3.06 -> 3.01 ms; bf16 4.07 -> 4.10, int8 3.11 -> 3.20 with it)
FM_KNOB(rowgemv, 123, FM_RANGE(0, 127))    // batch-1 decode linears on the row-block GEMV (fm_rowgemv.hip): bit 0 wo / w2, bit 1 wqkv, bit 2 w1 || w3,
                                           // bit 3 the codebook head, bit 4 the first layers' wqkv (0: 16-row MFMA tiles; 3 -> 27: 4.066 -> 4.032 ms);
                                           // bit 5: the first fast layer's QKV at codebooks >= 1 read from a table of its codebook_size possible
                                           // rows (no launch); bit 6: at codebook 0 the fast layers compute K / V only (one position: attention = v)
FM_KNOB(row_copies, 1, FM_BOOL)            // 1: fm_llm_finalize keeps a row-major copy of every linear the row-block GEMV can take, so any
                                           // rowgemv bits work later (bf16 S2-Pro: ~3.7 GB beside the packed tiles); 0: only the copies the
                                           // rowgemv / rowgemv_q4 bits in force at finalize select (w1 || w3 bf16 / int8: ~3.6 GB saved)
FM_KNOB(prefix_vec, 1, FM_BOOL)            // voice prefix copy (fm_prefix.hip): 1 16-byte accesses where the runs allow, 0 the scalar path
FM_KNOB(fast_pair, 1, FM_BOOL)             // 1: batch-1 bf16 frames run the fast decoder's codebook positions 0 and 1 as ONE two-row pass (both input
                                           // rows are known once the slow sampler has run; every fast weight is then read once for the two, not twice):
                                           // needs fast_tail, fattn_wo, rowgemv bits 0, 1, 5, 6 and not 2, gemv_chain off; elsewhere, and at 0, the one-row
                                           // passes (bit-identical)
FM_KNOB(fast_dead_q, 1, FM_RANGE(0, 3))    // weight-only int8 / int4 handles only (rowgemv bits 5 / 6 govern unquantised bf16): bit 0 the first fast layer's
                                           // QKV at codebooks >= 1 read from the table, bit 1 K / V only at codebook 0 -- batch 1, inside the fused fast
                                           // attention + wo, models without an o-bias (bit-identical).  S2-Pro frame, int8 /
                                           // int4: bit 0 -69 / -59 us (2.3 / 2.0 %); bit 1 -1.2 / -8.0 us, inside three times the baseline's spread: off
FM_KNOB(slow_attn_wo, 2, FM_RANGE(0, 2))   // batch-1 bf16 unquantised slow layers: attention + wo as one launch (fm_rowgemv.hip slow_attn_wo_kernel) where
                                           // attn_slow_plan gives attn_fd at 8 waves and fd_hpb 1, wo runs on the row-block GEMV and gemv_chain is off.
                                           // 1: two 2-row wo blocks per 512-thread block (S2-Pro frame 58 .. 101 us slower: its last 128 blocks start
                                           // after the attention), 2: two 4-row ones (the whole grid resident; 46 us, 1.24 %, faster with the two knobs below);
                                           // 0, and anywhere else, the two launches (bit-identical)
FM_KNOB(slow_aw_delay, 40, FM_RANGE(0, 300))  // slow_attn_wo 2: a wo wave's first read of x waits this per cent of the attention's duration as estimated
                                           // from the position (SlowAttnWoArgs::delay_pct; 0: reads from the start; 40: -15 us per frame, 75 and up lose)
FM_KNOB(slow_aw_sleep, 1, FM_SET(1, 4, 16))  // slow_attn_wo: s_sleep argument between a wo wave's reads of x (1, 4 or 16; no difference measured)
FM_KNOB(slow_aw_cheap, 1, FM_BOOL)         // slow_attn_wo: 1: a wo wave polls one word per 128 elements of its range before its full reads (8 cache
                                           // lines per poll, not 32; -27 us per frame)
FM_KNOB(slow_attn_wo_q, 0, FM_RANGE(0, 2)) // slow_attn_wo's launch on weight-only int8 / int4 handles (bf16 compute, layers without an o-bias; slow_attn_wo
                                           // keeps governing unquantised bf16 and nothing else, this knob is inert there): wo's row blocks read the row-major
                                           // codes (QM 1 / 2 of rowgemv_body).  0 the two launches, 1 two rows per 4-wave group, 2 four; the three wait knobs
                                           // above are shared (bit-identical).  S2-Pro frame, int8 / int4: 2 loses 17 / 26 us
                                           // (0.6 / 0.9 %), 1 loses 84 / 96 us, at baseline spreads of 3 / 4 us: off
FM_KNOB(fast_pair_q, 0, FM_RANGE(0, 3))    // fast_pair's two-row pass on weight-only handles (fast_pair keeps governing unquantised bf16 and nothing else, this
                                           // knob is inert there): bit 0 int8 handles, bit 1 int4 handles.  Needs fast_tail, fattn_wo, fast_dead_q bit 0, gemv_chain
                                           // off, a fast stack without an o-bias and the mode's default routing (int8: wo / w2 on the row GEMV, wqkv and w1 || w3 on
                                           // the tiles; int4: rowgemv_q4 bits 0, 1, 2 and 4, int4_stream 1); elsewhere, and at 0, the one-row passes
                                           // (bit-identical; profiles/fast_pair_q.md)
#endif
