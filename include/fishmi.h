/*
 * fishmi.h -- C ABI of libfishmi.so, the MI355X-native Fish-Speech S2-Pro hot path:
 * the Dual-AR text->semantic decode loop and the modded-DAC codec decode.
 *
 * The reference has no FFI/plugin API for this path; its seams are Python
 * callables.  Each entry point below replaces one of them (file:line in the reference,
 * PoTaTo-Mika/fish-speech @ 2026-04-03):
 *
 *   fm_llm_open/set_tensor/finalize  <- DualARTransformer.from_pretrained + init_model +
 *                                       setup_caches           (llama.py:479-593, 307-324,
 *                                                               707-721; inference.py:362-392)
 *   fm_llm_prefill                   <- generate() prefill: decode_one_token_ar(prompt,
 *                                       arange(T))             (inference.py:322-335)
 *   fm_llm_decode                    <- decode_one_token_ar per frame, batched over slots
 *                                                              (inference.py:96-181, 209-234)
 *   fm_llm_decode_frames             <- decode_n_tokens        (inference.py:184-238)
 *   fm_llm_generate                  <- generate()             (inference.py:241-359)
 *   fm_llm_teacher_step              <- forward_generate + forward_generate_fast with given
 *                                       tokens (teacher forcing; parity tests)
 *                                                              (llama.py:390-466, 798-827)
 *   fm_codec_open/set_tensor/...     <- load_codec_model / dac.inference.load_model
 *                                                              (inference.py:395-417;
 *                                                               dac/inference.py:23-47)
 *   fm_codec_decode                  <- DAC.from_indices       (modded_dac.py:925-927)
 *
 * Conventions: every function returns FM_OK (0) or a negative FM_ERR_*; the message of the
 * last failure on the calling thread is fm_last_error().  Nothing throws across the ABI.
 * Buffers are caller-owned host memory.  One handle per GPU; calls on a handle must come from
 * one host thread at a time (the reference's single LLM worker thread, inference.py:748-799).
 * Token matrices are (C+1) x T row-major int32, exactly the reference's prompt layout
 * (row 0 = text/semantic token, rows 1..C = codebooks).
 */
#ifndef FISHMI_H
#define FISHMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_OK 0
#define FM_ERR_ARG -1
#define FM_ERR_HIP -2
#define FM_ERR_STATE -3
#define FM_ERR_OOM -4

/* precision of the compute path: bf16 storage + fp32 accumulation (production), or the fp32
   validation mode (same kernels, fp32 storage) used for token-exact parity. */
#define FM_PREC_BF16 0
#define FM_PREC_FP32 1

/* source dtype for fm_*_set_tensor (FM_DT_I8: int8 linear weights, fm_llm_set_quant INT8 only) */
#define FM_DT_F32 0
#define FM_DT_BF16 1
#define FM_DT_I8 2

/* weight-only quantization of the Dual-AR linears (fm_llm_set_quant) */
#define FM_QUANT_NONE 0
#define FM_QUANT_INT8 1
#define FM_QUANT_INT4 2  /* groupwise int4, group size 128 (fm_llm_set_quant_int4 for others) */

/* == DualARModelArgs after from_pretrained (llama.py:27-193); im_end_id from the tokenizer. */
typedef struct fm_model_config {
    int vocab_size, dim, n_layer, n_head, n_local_heads, head_dim, intermediate_size;
    float rope_base, norm_eps;
    int max_seq_len;
    int qkv_bias, o_bias, qk_norm, tie_word_embeddings;
    int codebook_size, num_codebooks, semantic_begin_id, semantic_end_id, im_end_id;
    int scale_codebook_embeddings, norm_fastlayer_input;
    int n_fast_layer, fast_dim, fast_n_head, fast_n_local_heads, fast_head_dim,
        fast_intermediate_size;
    int fast_qkv_bias, fast_o_bias, fast_qk_norm;
} fm_model_config;

/* sampling knobs of decode_one_token_ar; temperature/top_p are applied as tensors of the
   compute dtype like inference.py:305-306.  mask_im_end=1 forbids <|im_end|> (fixed-length
   timing runs). */
typedef struct fm_sampling {
    float temperature, top_p;
    int top_k;
    uint64_t seed;
    int mask_im_end;
} fm_sampling;

typedef struct fm_llm fm_llm;

int fm_device_count(void);
const char* fm_last_error(void);

/* Build provenance: the first 16 hex digits of sha256 over the sources and headers the library was
 * compiled from (fish-speech_amd/Makefile HASHED); fishmi.native.lib() refuses a library whose hash
 * differs from the tree's, so a stale prebuilt libfishmi.so cannot run. */
const char* fm_source_hash(void);
/* Measured HBM stream peak of `device` (no reference counterpart: SURVEY.md §8d's STREAM-like
   figure beside the vendor peak): a non-temporal float4 read stream (GB/s read) and a float4 copy
   (GB/s read + written) over `bytes`-sized buffers (>= 64 MiB; use >> 256 MiB to defeat the MALL),
   `reps` timed launches each. */
int fm_stream_peak(int device, int64_t bytes, int reps, double* read_gbps, double* copy_gbps);

int fm_llm_open(const fm_model_config* cfg, int device, int precision, int max_slots,
                fm_llm** out);
/* Weight-only int8 linears, opt-in (replaces tools/llama/quantize.py WeightOnlyInt8QuantHandler
   .convert_for_runtime + the int8 branch of from_pretrained, llama.py:528-535; quantize.py:190-232).
   Call before any set_tensor.  Every nn.Linear (attention wqkv/wo, feed_forward w1/w2/w3 of both
   stacks, output when untied, fast_project_in, fast_output) then takes either int8 data
   (FM_DT_I8) plus "<module>.scales" [out_features], as quantize.py writes them, or float weights
   that finalize quantizes per output channel with quantize.py's rule.  Outputs are
   round(round(x . q) * scale) like WeightOnlyInt8Linear.forward; the linears' biases are unused
   (that module has none).  Off the bf16 parity contract: parity is against the reference's own
   int8 model. */
int fm_llm_set_quant(fm_llm* h, int mode);
/* Weight-only int4, groupwise affine (replaces tools/llama/quantize.py WeightOnlyInt4QuantHandler
   .create_quantized_state_dict + convert_for_runtime and the int4 branch of from_pretrained,
   llama.py:537-543; quantize.py:57-160, 239-418).  bf16 only; bias-free linears (quantize.py:371);
   groupsize 32, 64, 128 or 256 dividing every in_features.  Every nn.Linear takes float weights, quantized at
   finalize with the reference's group_quantize_tensor (bit-exact, in its bf16 arithmetic); each
   then computes with the weights bf16(fma(q - 8, scale, zero)), and the batch <= 8 decode GEMVs
   stream the 4-bit codes (group size a multiple of 128).  The reference's packed checkpoint format
   (_convert_weight_to_int4pack tiles) is not read: quantize from the bf16 checkpoint instead. */
int fm_llm_set_quant_int4(fm_llm* h, int groupsize);
/* Compact weight-only handles, opt-in (bf16): keep only the codes.  Without it a quantised handle keeps, beside
   the codes, a full bf16 fragment copy of every quantised linear (int8: bf16(q); int4: bf16(fma(q - 8, scale,
   zero))) for the kernels that read bf16 tiles -- 2 bytes per weight.  With it fm_llm_finalize builds the
   step-granular code copy of every quantised linear whatever max_slots is, frees each linear's bf16 copy once its
   code copies are packed (an FM_DT_I8 tensor is never expanded to bf16 at all), and every launch reads codes: the
   16-row MFMA tile kernel -- prompt chunks of more than 8 rows, the heads, every batched shape without a code
   form of its own -- rebuilds each bf16 fragment from the codes right before its MFMAs, bit for bit, so a compact
   handle computes exactly what the same handle computes without the flag.  The decode-GEMV units, the row-major
   copies and the (scale, zero) / row-scale tables stay as they are.
   Call after fm_llm_set_quant / fm_llm_set_quant_int4 and before any set_tensor: FM_ERR_STATE out of that order
   or on an unquantised handle, FM_ERR_ARG on an fp32 handle (the code-reading forms are bf16).  fm_llm_finalize
   on a compact handle returns FM_ERR_ARG, naming the tensor and leaving the handle as it was, unless every
   quantised linear can be served from codes: int8, in_features a multiple of 64; int4, the group size and
   in_features multiples of 128 and in_features a whole number of groups.
   Peak memory during load is not lowered: set_tensor still uploads float weights whole before finalize quantises
   them, and both copies of a linear exist until its codes are packed. */
int fm_llm_set_quant_compact(fm_llm* h, int enable);
/* Steady-state device bytes of a finalized handle, booked where they are allocated: out[0] the bf16 / fp32
   fragment copies of quantised linears, [1] the decode-GEMV code units and their scale tables, [2] the
   step-granular codes, [3] the row-major copies (codes or bf16 as they are) and their tables, [4] every other
   weight (embeddings, norms, heads that are no quantised linear, an untied head's uploaded table, the QKV table),
   [5] the KV caches, [6] activations and scratch, [7] their sum.  On an unquantised handle [0] .. [2] are 0 and
   the packed weights count under [4].  Voice prefix snapshots are not included. */
int fm_llm_memory_info(fm_llm* h, int64_t out[8]);
/* name = reference state_dict key after remap (e.g. "layers.3.attention.wqkv.weight") */
int fm_llm_set_tensor(fm_llm* h, const char* name, const void* host_data, int src_dtype,
                      int64_t numel);
/* deterministic synthetic tensor (fishmi/synth.py formula), generated on the device */
int fm_llm_synth_tensor(fm_llm* h, const char* name, int64_t numel, uint64_t seed, float center,
                        int log2_half);
int fm_llm_finalize(fm_llm* h);
/* n requests prefilled together (each from position 0 of its own slot, slots distinct): tokens
   holds each request's (C+1) x T[i] prompt block back to back, sp one sampling record per request;
   one pass of the slow stack over all prompt rows, one batched first frame; writes n first columns
   (n x (C+1)), the same as n fm_llm_prefill calls (the reference prefills requests one by one:
   inference.py:620-724; this is the serving side's batched form of it). */
int fm_llm_prefill_batch(fm_llm* h, int n, const int32_t* slots, const int32_t* tokens, const int32_t* T,
                         const fm_sampling* sp, int32_t* first_cols);
/* resets slot's caches and runs the prompt; writes the first emitted column (C+1). */
int fm_llm_prefill(fm_llm* h, int slot, const int32_t* tokens, int T, const fm_sampling* sp,
                   int32_t* first_col);
/* one frame for n slots (each continues from its own position); cols: n x (C+1) */
int fm_llm_decode(fm_llm* h, const int32_t* slots, int n, int32_t* cols);
/* nframes frames for the n slots, queued back to back with no host round trip per frame
   (im_end does not stop it: callers drop columns after a slot's <|im_end|>, as the batched
   engine does); cols: nframes x n x (C+1). */
int fm_llm_decode_frames(fm_llm* h, const int32_t* slots, int n, int nframes, int32_t* cols);
/* full generate() for one slot: out (C+1) x max_new row-major; *n_out frames produced
   (stops after emitting <|im_end|> unless mask_im_end). */
int fm_llm_generate(fm_llm* h, int slot, const int32_t* prompt, int T, int max_new,
                    const fm_sampling* sp, int32_t* out, int* n_out);
/* generate() continuing a slot's cached prefix: positions [0, pos0) keep the KV of tokens the
   slot already ran (the previous generate_long batch's prompt and fed columns), the prompt suffix
   ((C+1) x T) is prefilled at pos0 .. pos0 + T - 1, then decoding as fm_llm_generate.  Replaces
   the whole-conversation re-prefill of generate_long (inference.py:620-724) for the shared
   prefix.  pos0 must not exceed fm_llm_slot_pos. */
int fm_llm_generate_at(fm_llm* h, int slot, const int32_t* suffix, int T, int pos0, int max_new,
                       const fm_sampling* sp, int32_t* out, int* n_out);
/* fm_llm_prefill continuing the slot's cached positions [0, pos0): the suffix runs at pos0 .. */
int fm_llm_prefill_at(fm_llm* h, int slot, const int32_t* suffix, int T, int pos0, const fm_sampling* sp,
                      int32_t* first_col);
/* positions of the slot whose KV is written (prompt + fed columns of its last generate) */
int fm_llm_slot_pos(fm_llm* h, int slot, int* pos);
/* Voice prefix cache (no reference counterpart: the reference prefills the whole conversation,
   system message with the reference voice included, for every request, inference.py:620-724).
   prefix_save snapshots the slow-stack K/V rows [0, npos) of `slot` into a device buffer owned by
   the handle, laid out [layer][K|V][kv head][npos][head_dim] in the handle's storage type;
   1 <= npos <= the slot's cached positions.  The slot is not modified.  FM_ERR_OOM when the buffer
   cannot be allocated: no id is issued and earlier entries stay intact. */
int fm_llm_prefix_save(fm_llm* h, int slot, int npos, int* prefix_id);
/* write a saved prefix into rows [0, npos) of n distinct slots (one launch for all of them) and
   set each slot's cached position to npos, as if it had just run those positions; the slots'
   rows >= npos and every other slot are untouched.  Follow with fm_llm_prefill_at /
   fm_llm_prefill_batch_at at pos0 <= npos. */
int fm_llm_prefix_load(fm_llm* h, int prefix_id, const int32_t* slots, int n);
int fm_llm_prefix_drop(fm_llm* h, int prefix_id);
int fm_llm_prefix_info(fm_llm* h, int prefix_id, int* npos, int64_t* bytes);
/* fm_llm_prefill_batch with a start position per request: request i keeps its slot's cached
   positions [0, pos0[i]) and prefills its T[i] suffix columns at pos0[i]..; pos0 all zero is
   exactly fm_llm_prefill_batch. */
int fm_llm_prefill_batch_at(fm_llm* h, int n, const int32_t* slots, const int32_t* tokens,
                            const int32_t* T, const int32_t* pos0, const fm_sampling* sp,
                            int32_t* first_cols);
/* teacher forcing for parity: run S positions of x ((C+1) x S) from pos0 on slot (pos0 == 0
   resets the slot), return the last position's slow logits (V, with the semantic bias NOT
   applied), the fast hidden (fast_dim), and -- when next_col != NULL -- the fast logits
   ((C-1) x codebook_size) obtained by feeding next_col's codebook tokens. */
int fm_llm_teacher_step(fm_llm* h, int slot, const int32_t* x, int S, int pos0,
                        const int32_t* next_col, float* slow_logits, float* hidden,
                        float* fast_logits);
/* decode-step accounting for the roofline: algorithmic HBM bytes of one frame at batch n
   (weights read once per frame + KV + embeddings) at cached length `pos`. */
int64_t fm_llm_frame_bytes(fm_llm* h, int n, int pos);
/* per-kernel-class timing (HIP events on the compute stream) */
int fm_llm_profile(fm_llm* h, int enable);
int fm_llm_profile_read(fm_llm* h, const char* kernel_class, double* total_ms, int64_t* launches,
                        int64_t* bytes);
/* roofline hook: runs one decode frame for the last decoded slot set (advancing them one frame)
   while recording the launches of kernel_class ("linear" = the decode GEMVs), then replays
   exactly those launches back to back `reps` times as one graph between two HIP events on the
   compute stream: average duration per launch, launches and algorithmic bytes per frame.
   The replays clobber activation scratch only (KV caches and slot state are untouched). */
int fm_llm_kernel_bench(fm_llm* h, const char* kernel_class, int reps, double* avg_us,
                        int64_t* launches, int64_t* bytes);
int fm_llm_use_graph(fm_llm* h, int enable);
/* developer hook: row 0 of an activation buffer of the decode path ("qkv", "att", "fh", "act",
   "fx", "fx2", "xl", "xnl": bf16/fp32 storage as floats) or slot 0's KV cache of slow layer `index`
   ("kc" / "vc": [n_local_heads][S][head_dim], n <= its size; the prefix-reuse identity tests) */
int fm_llm_debug_vec(fm_llm* h, const char* name, int index, float* out, int64_t n);
/* Teacher forcing on the PRODUCTION decode path (parity with the reference's own teacher-forced
   forward_generate / forward_generate_fast, llama.py:390-466, 798-827): while a slot is forced,
   every sampler of its frames (prefill and decode, graph-replayed or eager, batch-1 GEMV path or
   batched path) emits the given column instead of its draw and copies the logits it was handed
   to a per-slot tap.  col: (C+1) tokens of the next emitted column (row 0 a semantic id or
   <|im_end|>), or NULL to stop forcing; set it before fm_llm_prefill / each fm_llm_decode.
   read_logits: the last forced frame's slow logits (V floats, -inf outside the semantic rows and
   <|im_end|>, bias NOT applied) and fast logits ((C-1) x codebook_size, codebooks 1..C-1). */
int fm_llm_force(fm_llm* h, int slot, const int32_t* col);
int fm_llm_read_logits(fm_llm* h, int slot, float* slow_logits, float* fast_logits);
/* process-wide developer knobs selecting kernel variants (every variant stays under the default
   path's parity bar, tests/test_gpu_knobs.py).  The keys, their defaults and their accepted values
   are the entries of fish-speech_amd/csrc/fm_tune_table.h, plus "debug_ts" n (arms the records of
   fm_debug_ts_read); an unknown key or a value outside the accepted ones fails with FM_ERR_ARG.
   fm_tune_get reads the value in force ("debug_ts": whether it is armed).
   "bstream_q8" 0|1 (weight-only int8 bf16 models opened with more than 8 slots: 1, the default, the
   batched decode linears stream the int8 codes -- bit-identical outputs, half the weight bytes -- 0
   the bf16 copy of the codes; inert for every other model).
   "bstream_q4" 0|1 (weight-only int4 bf16 models with a group size that is a multiple of 128, opened
   with more than 8 slots: 1, the default, the batched decode linears stream the 4-bit codes and their group
   (scale, zero) words -- bit-identical outputs, 0.28x the weight bytes -- 0 the dequantised bf16
   copy; inert for every other model, under "int4_stream" 0, "bstream_acc" 0 and on the "bstream_chain"
   forms).
   "prompt_skinny_q" 0|1|2, default 1 (weight-only int8 / int4 models in bf16 compute, linears of 33 .. 64
   rows: a prompt chunk's, a batched frame's of 33 .. 64 slots): 1 the skinny prompt GEMM streams the
   step-granular codes where the handle holds them (a compact handle, or one opened with more than 8 slots;
   int4: a group size that is a multiple of 128), 0 it streams the bf16 copy of the quantised weights (int8:
   the row scales applied in its epilogues) -- the two give the same bits -- and 2 keeps quantised linears
   off the skinny GEMM, on the 16-row tile kernel every row count above 8 used before; a handle without
   the step-granular copy runs 1 as 0, and a compact handle, which has no bf16 copy, runs 0 as 1.  Inert
   for unquantised and fp32 models and at any other row count.
   "prompt_gemm_q" 0|1|2, default 1 (the same models, linears of more than 64 rows: a long prompt's chunks, a
   batched prefill of more than 64 rows in all): 1 the tiled prompt GEMMs of the bf16 model, with its K split,
   reading what the handle's linears read before -- the bf16 copy of the quantised weights (int8: the row
   scales applied in the epilogues), or a compact handle's step-granular codes, from which the kernels rebuild
   that copy's fragments; 2 the codes wherever the handle holds them (for measurement); 0 the 16-row tile
   kernel, as before.  1 and 2 give the same bits; a compact handle runs 0 as 1.  Inert elsewhere.
   "rowgemv" / "rowgemv_q4" bits, "row_copies" 0|1 (0: finalize keeps only the row-major weight
   copies those bits select).  "rowgemv" 0..127, default 123: bits 0-4 put wo / w2, wqkv, w1 || w3,
   the codebook head and the first layers' wqkv on the row-block GEMV; bit 5 (32): the first fast
   layer's QKV projection at codebooks >= 1 -- a pure function of the sampled code -- is read from a
   table of its codebook_size rows (codebook_size x fast nqkv bf16, 50 MB at S2-Pro; built by
   fm_llm_finalize with the frame's own kernel, one launch per code, and rebuilt before the next
   frame after any fm_tune call but "debug_ts") instead of being launched; bit 6 (64): at codebook
   0, where the fast attention has one position and its output is v, the fast layers project K / V
   only and the attention reads no Q.  Bits 5 and 6 change no output bit (finite scores); they act
   on bf16 unquantised models, batch 1, and are inert elsewhere.  Knobs apply to launches
   recorded after the call (graphs captured earlier keep theirs; fm_llm_use_graph drops them).
   "fattn_ilp" 0|1 (default 1: the fused fast attention + wo launch runs its q / k preparation and
   score / softmax / PV over a compile-time position count in one basic block) changes no output
   bit either.
   "fast_pair" 0|1 (default 1): a batch-1 bf16 frame runs the fast decoder's codebook positions 0
   and 1 -- whose input rows, the slow model's hidden row and the embedding of the code the slow
   sampler drew, are both known when the fast passes start -- as one causal two-row pass, so every
   fast weight is read once for the two and not twice (13 launches fewer per frame at 4 fast
   layers).  It engages on bf16 unquantised models at one row with "fast_tail" and "fattn_wo" on,
   "gemv_chain" off and "rowgemv" bits 0, 1, 5 and 6 set and bit 2 clear, at shapes whose two-row
   kernel forms exist; anywhere else, and at 0, the one-row passes run.  It changes no output bit.
   "fast_pair_q" 0..3 (default 0): the same two-row pass on weight-only handles (compact ones too), which
   "fast_pair" leaves alone -- bit 0 (1) int8 handles, bit 1 (2) int4 handles.  It engages at one row in
   bf16 compute on a fast stack without an o-bias, with "fast_tail" and "fattn_wo" on, "gemv_chain" off and
   "fast_dead_q" bit 0 set, on each mode's default routing -- int8: "rowgemv" bit 0 set and bits 1 and 2
   as they act on int8 (wqkv and w1 || w3 on the tile kernel), dim <= 4096; int4: "int4_stream" on and
   "rowgemv_q4" bits 0, 1, 2 and 4 set (bit 4: the pair's first layer projects row 0's K / V rows on the
   row form) -- at shapes whose two-row code forms exist: a wave's run of 512-k chunks at most 2 (int8;
   nq <= 4096) or 3 (int4; nq <= 6144) in the fused launch, at most 3 for the int4 wqkv and w1 || w3
   (dim <= 6144), at most 5 for wo and w2 (intermediate <= 10240).  Anywhere else, and at 0, the one-row
   passes run.  The knob is inert on unquantised handles and changes no output bit.
   "fast_dead_q" 0..3 (default 1): the two removals of "rowgemv" bits 5 and 6 for weight-only int8 /
   int4 handles, which those bits leave alone -- bit 0 (1) the first fast layer's QKV table (built the
   same way, by the quantised model's own launch), bit 1 (2) K / V only at codebook 0.  They act at batch
   1 in bf16 compute where the fused fast attention + wo launch runs, on models configured without an
   o-bias, and change no output bit; inert on unquantised models and everywhere else.
   "slow_attn_wo" 0..2 (default 2): a batch-1 bf16 unquantised frame runs each slow layer's attention and
   its wo as one launch (1: two wo rows per 4-wave group, 2: four) where the attention is attn_fd at 8 waves
   and one q head per block, wo is on the row-block GEMV, "gemv_chain" is off and head_dim is 128; anywhere
   else, and at 0, the two launches.  "slow_attn_wo_q" 0..2 (default 0): the same launch, with the same
   meaning of 1 and 2, on weight-only int8 / int4 handles (compact ones too) whose slow layers have no
   o-bias: wo's row blocks read the row-major codes.  Each of the two knobs is inert on the other's
   handles; both share "slow_aw_delay", "slow_aw_sleep" and "slow_aw_cheap" (how wo's waves wait: speed
   only) and change no output bit.
   Compact handles (fm_llm_set_quant_compact) hold no bf16 copy of their quantised linears, so the six knobs
   that would pick a reader of that copy are ignored for such a handle, which keeps its default routing:
   "bstream" 0 and "bstream_acc" 0 (its batched frames stay on the accumulating kernel's code forms),
   "bstream_chain" 1 (the chain forms read bf16 tiles), "bstream_q8" 0, "bstream_q4" 0 and "int4_stream" 0
   (the codes are streamed whatever they say).  A shape whose batched kernel has no code form runs on the tile
   kernel's code-reading form instead.  The knobs are process-wide: handles without the flag in the same
   process keep their meaning. */
int fm_tune(const char* key, int value);
int fm_tune_get(const char* key, int* value);
/* developer hook ("debug_ts" armed): per-block records of 8 words {tag = N<<32 | blockIdx.y<<16 |
   blockIdx.x, start, staged, streamed, end, 3 kernel-specific} of the decode GEMVs,
   s_memrealtime ticks (100 MHz). */
int fm_debug_ts_read(unsigned long long* out, int64_t max_records, int64_t* n_records);
int fm_llm_close(fm_llm* h);

/* ---- per-op parity hooks (tests): one production kernel on caller operands, fp32 host arrays
   in/out (converted to the precision's storage type).  Each replaces nothing in the reference; they
   pin the fused decode kernels to the reference's per-op semantics (tests/golden/ops.npz). */
/* RMSNorm (llama.py:989-1000), R rows of d: mode 0 = the decode GEMV prologue computing the
   statistic from the row (first layer, head), 1 = the prologue fed by the producing GEMV's per-tile
   sums of squares (every later norm of the batch-1 path), 2 = the standalone row kernel (batched /
   prefill path). */
int fm_op_rmsnorm(int device, int precision, int mode, const float* x, const float* w, int R, int d,
                  float eps, float* y);
/* QK-norm (llama.py:861-863) + RoPE with the bf16 table (llama.py:1003-1037) at position pos, as the
   fused decode attention computes them: kernel 0 = slow attn_decode2, 1 = fast-model attention,
   2 = slow attn_dec3, 3 = slow attn_fd (the production kernel).
   qkv: one raw projection row [(nh + 2 nkv) * hd]; q_out [nh * hd], k_out [nkv * hd] (the k row as
   written to the KV cache). */
int fm_op_qk_rope(int device, int precision, int kernel, const float* qkv, int nh, int nkv, int hd,
                  const float* qn, const float* kn, int qk_norm, float eps, float rope_base, int pos,
                  float* q_out, float* k_out);
/* The whole slow-model decode attention as the decode path runs it (llama.py:883-945: QK-norm, RoPE,
   KV-cache write, scaled dot-product attention with the GQA group sharing its kv head) on R rows;
   row r uses slot r of caller caches kcache / vcache [R][nkv][S][hd] holding rows < pos[r].
   kernel 0 = attn_decode2, 2 = attn_dec3, 3 = attn_fd (flash-decode splits of >= min_split
   positions).  out [R][nh * hd]; kc_out / vc_out receive the caches after the kernel's write. */
int fm_op_decode_attn(int device, int precision, int kernel, const float* qkv, int R, int nh, int nkv, int hd,
                      const float* qn, const float* kn, int qk_norm, float eps, float rope_base, const int* pos,
                      const float* kcache, const float* vcache, int S, int min_split, float* out, float* kc_out,
                      float* vc_out);
/* prompt-chunk causal attention (llama.py:883-946, the prefill path after QK-norm / RoPE / KV
   write): q [R][nh * hd] of rows at positions pos0 .. pos0 + R - 1 of one slot, caches
   kcache / vcache [nkv][S][hd] holding every position <= pos0 + R - 1.  kernel 0 = split +
   combine kernels, 1 = attn_prefill_kernel (flash form on MFMA; bf16, head_dim 128, <= 4 q heads
   per kv head).  out [R][nh * hd]. */
int fm_op_prompt_attn(int device, int precision, int kernel, const float* q, int R, int nh, int nkv, int hd, int pos0,
                      const float* kcache, const float* vcache, int S, float* out);
/* Attention hooks with the cache as the model lays it out (tests/test_gpu_attn_ops.py): kcache / vcache are
   [nslots][layers][nkv][S][hd], row r works on slot row_slot[r] (distinct where the kernel writes the cache) and
   layer `layer`; the caches are in/out where the kernel writes them, so the caller sees every word of them.

   fm_op_decode_attn_ex: fm_op_decode_attn with the launch forms of the frame.  Input qkv [R][ld], ld = (nh + 2 nkv) hd,
   or (attn_fd only) slab [kp][R][ld] fp32 K-part slabs + optional bias [ld], read as round(sum + bias).  attn_fd runs
   with nwb (4, 8, 16) waves per block and splits of at least cap positions; attn_decode2 with min(cap, its LDS
   budget) rows per block.  frame != 0: kernel, nwb and cap are what a decode frame of R rows launches under the
   current fm_tune knobs (kernel, cap, nwb arguments ignored).  reps launches on the same scratch.  The split
   partials are allocated at the documented size, poisoned, with a guard region behind them.
   info[8] out: {kernel run, nwb, cap, splits (grid z), ticket words left non-zero, guard intact (1 / 0), FD_NSP (most
   attn_fd splits), attn_decode2's LDS-budget cap}. */
int fm_op_decode_attn_ex(int device, int precision, int kernel, const float* qkv, const float* slab, int kp,
                         const float* bias, int R, int nh, int nkv, int hd, const float* qn, const float* kn,
                         int qk_norm, float eps, float rope_base, const int* row_slot, const int* pos, int nslots,
                         int layers, int layer, float* kcache, float* vcache, int S, int cap, int nwb, int frame,
                         int reps, float* out, int* info);
/* fm_op_prompt_attn on rows with their own (slot, position): one_slot != 0 says they are consecutive rows of one
   slot (what attn_prefill_kernel, kernel 1, needs); one_slot == 0 is the many-slot split + combine route. */
int fm_op_prompt_attn_ex(int device, int precision, int kernel, const float* q, int R, int nh, int nkv, int hd,
                         const int* row_slot, const int* row_pos, int one_slot, int nslots, int layers, int layer,
                         const float* kcache, const float* vcache, int S, float* out);
/* The prefill's QK-norm + RoPE + cache write (qk_rope_cache_kernel) on R rows at row_pos[r], or all at fixed_pos
   (>= 0; the fast decoder's form); input qkv or slabs + bias as fm_op_decode_attn_ex.  q_out [R][nh * hd]. */
int fm_op_qk_rope_cache(int device, int precision, const float* qkv, const float* slab, int kp, const float* bias, int R,
                        int nh, int nkv, int hd, const float* qn, const float* kn, int qk_norm, float eps,
                        float rope_base, const int* row_slot, const int* row_pos, int fixed_pos, int nslots, int layers,
                        int layer, float* kcache, float* vcache, int S, float* q_out);
/* The fast decoder's attention (llama.py:947-975) at codebook position cpos of S = num_codebooks on R rows:
   kernel 0 = fast_attn2, 1 = fast_attn2 with noq (cpos 0: the Q part of qkv is not read), 2 = fast_attn_fused,
   3 = qk_rope_cache(fixed_pos) + fast_attn_kernel (the unfused pair).  out [R][nh * hd]. */
int fm_op_fast_attn(int device, int precision, int kernel, const float* qkv, int R, int nh, int nkv, int hd,
                    const float* qn, const float* kn, int qk_norm, float eps, float rope_base, const int* row_slot,
                    int cpos, int nslots, int layers, int layer, float* kcache, float* vcache, int S, float* out);
/* The batch-1 fast decoder's attention + wo at codebook position cpos of slot `slot` (bf16 attention; wo in bf16,
   int8 or int4: quant FM_QUANT_*, gs the int4 group size).  fused != 0: ONE launch_fattn_wo; fused == 0: the launches
   it replaces on the same device operands (fast_attn2 + the row GEMV, FIN).  qkv [1 or (pair) 2][ld]; qtab
   [qrows][ld] or NULL: the QKV table, row idx[idx_col] clamped into it; idx also gathers the residual row of res
   [res_rows][ldr] (NULL: row 0); kv0: the K / V-only form of codebook 0 (the Q part of qkv is not read); pair 1 / 2:
   codebooks 0 and 1 in one launch (res0 [N]: row 0's residual for pair 1; y [2][N]), else y [N]; ilp: fm_tune
   fattn_ilp; gen (1..40) and pos0 make the hand-off tag; xt_init [2 nh hd] or NULL pre-fills the tagged words.
   w [N][nh hd], bias [N] or NULL.  The pair forms take int8 / int4 wo too (fm_tune "fast_pair_q").  status[2] out:
   {0 = not dispatchable, nothing was launched (fattn_wo_ok, fattn_wo_dead_ok for the table and K / V-only forms,
   the pair form's depth), else the dispatched depth in chunks per wave; the err word after the launch}. */
int fm_op_fattn_wo(int device, int quant, int gs, int fused, const float* qkv, const float* qtab, int qrows,
                   const int32_t* idx, int idx_n, int idx_col, int nh, int nkv, int hd, const float* qn, const float* kn,
                   int qk_norm, float eps, float rope_base, int slot, int cpos, int nslots, int layers, int layer,
                   float* kcache, float* vcache, int S, const float* w, const float* bias, const float* res,
                   int res_rows, int ldr, const float* res0, int N, int kv0, int pair, int ilp, int gen, int pos0,
                   const uint32_t* xt_init, float* y, int* status);
/* The batch-1 slow layers' attention + wo (bf16) at nrun (slots[i], pos[i]) pairs of one layer, run one after the
   other on the same device operands and the same tagged-word buffer.  fused != 0: ONE launch_slow_attn_wo each (rp 2
   or 4 wo rows per 4-wave group: fm_tune slow_attn_wo 1 / 2); fused == 0: the launches it replaces (attn_fd as the
   batch-1 frame runs it + the row GEMV, FIN).  qkv [nrun][ld]; gens[i] (1..40) with pos[i] makes run i's hand-off
   tag; restore != 0: every run starts from the caller's cache contents, else from what the runs before it left;
   xt_init [nh hd] or NULL pre-fills the tagged words.  w [N][nh hd], bias [N] or NULL, res [N].  Out: y [nrun][N],
   k_rows / v_rows [nrun][nkv][hd] (the cache rows at pos[i] after run i), status[2] = {dispatchable as the frame asks
   (0 with fused: nothing was launched), the err word after the last run}. */
int fm_op_slow_attn_wo(int device, int fused, int rp, const float* qkv, int nh, int nkv, int hd, const float* qn,
                       const float* kn, int qk_norm, float eps, float rope_base, const int32_t* slots, const int32_t* pos,
                       const int32_t* gens, int nrun, int restore, int nslots, int layers, int layer, const float* kcache,
                       const float* vcache, int S, const float* w, const float* bias, const float* res, int N,
                       const uint32_t* xt_init, float* y, float* k_rows, float* v_rows, int* status);
/* fm_op_slow_attn_wo on weight-only codes (fm_tune slow_attn_wo_q): the bf16-valued w [N][nh hd] is quantised on the
   device by the model's own rule -- quant FM_QUANT_INT8: row scales; FM_QUANT_INT4: groups of gs along K, (scale,
   zero) per group -- and packed row-major as the model's row GEMV reads it; then, per (slots[i], pos[i]) pair, ONE
   launch_slow_attn_wo on the codes (fused != 0) or attn_fd + the row GEMV (FIN) on the same codes (fused == 0).
   status, restore, gens and xt_init as above.  q_out [N][nh hd] (int8: the codes; int4: the codes 0..15, one per
   byte), scale_out (int8 [N]; int4 [N][nh hd / gs]) and zero_out (int4) may be NULL.  FM_ERR_ARG for a bias, for
   nh hd not in whole 512-k chunks and for a gs that is no multiple of 8 or does not divide nh hd. */
int fm_op_slow_attn_wo_q(int device, int quant, int gs, int fused, int rp, const float* qkv, int nh, int nkv, int hd,
                         const float* qn, const float* kn, int qk_norm, float eps, float rope_base, const int32_t* slots,
                         const int32_t* pos, const int32_t* gens, int nrun, int restore, int nslots, int layers, int layer,
                         const float* kcache, const float* vcache, int S, const float* w, const float* bias,
                         const float* res, int N, const uint32_t* xt_init, float* y, float* k_rows, float* v_rows,
                         int* status, int8_t* q_out, float* scale_out, float* zero_out);
/* Dual-AR input embedding (llama.py:399-420): tok R x (C+1) row-major, x R x dim. */
int fm_op_embed(int device, int precision, const int32_t* tok, int R, const float* emb, int vocab,
                const float* cbemb, int dim, int num_codebooks, int codebook_size, int semantic_begin_id,
                int semantic_end_id, int scale_codebook_embeddings, float* x);
/* Weight-only int4 (fm_llm_set_quant_int4): the device quantizer on a bf16-valued w [N][K] with group
   size gs (quantize.py:57-160 in its bf16 arithmetic): codes q [N][K] (0..15), group scale / zero
   [N][K/gs] and the dequantised weights bf16(fma(q - 8, scale, zero)) [N][K].  With x (R <= 8 rows
   of K), also the decode GEMV y = x . w_deq^T ([R][N] fp32) on the dequantised bf16 weights (y_bf16)
   and, when gs and K are multiples of 128 and y_q4 is given, on the streamed 4-bit codes (y_q4). */
int fm_op_quant4(int device, const float* w, int N, int K, int gs, uint8_t* q, float* scale, float* zero,
                 float* w_deq, const float* x, int R, float* y_q4, float* y_bf16);
/* Weight-only int8 on the batched decode linear (8 < R <= 32, bf16; fm_tune "bstream_q8"): quantises
   the bf16-valued w [N][K] on the device with the int8 rule (quantize.py:22-52), packs the codes
   both ways and runs the batched linear's plan once per form: y_q8 from the streamed int8 codes,
   y_bf16 from their bf16 fragment copy.  x [R][K] bf16-valued.  epi 0 (store) / 3 (fp32): [R][N]
   outputs round(round(acc) * scale); epi 7 (SwiGLU over w's 16-row tiles of 8 gate + 8 up rows):
   [R][N/2]; epi 4 (split-K slabs): the raw fp32 slabs [kparts][R][N], no scale.  kparts: the plan's
   K parts.  q_out [N][K] / scale_out [N] (optional): the codes and bf16 row scales it used. */
int fm_op_batched_linear_q8(int device, const float* w, int N, int K, const float* x, int R, int epi,
                            float* y_q8, float* y_bf16, int* kparts, int8_t* q_out, float* scale_out);
/* ---- the decode linears (tests/test_gpu_linear_ops.py): each hook runs ONE production launcher on
   caller operands.  Weights w are row-major [N][K] (the hook packs them as the model loader does);
   epi / pro are the kernels' own codes: epi 0 store, 1 residual, 2 SwiGLU (w, w2), 3 fp32, 4 fp32 K-slice
   slabs, 5 slabs + residual finalise, 7 SwiGLU over row-interleaved 8 gate + 8 up tiles; pro 0 plain,
   1 RMSNorm from the row, 3 RMSNorm from the producer's per-tile sums of squares.  Every output array
   is in/out: [y_rows >= rows written][ld >= columns written], uploaded before the launch and
   downloaded after it, so what the kernel leaves alone comes back as the caller filled it.  reps: the
   launch is repeated that many times on the same scratch (tickets, partials, sums of squares);
   dirty: the ticket / counter words left non-zero afterwards (a correct kernel leaves 0). */
/* launch_linear (the 16-row MFMA tile kernel), any R: y = epilogue(x . w^T + bias).  split != 0 and
   8 < R <= 64: partials and tickets are supplied as the batched frame does, so fm_tune "linear_fill"
   splits K; ksb returns the slices used. */
int fm_op_linear(int device, int precision, int epi, const float* w, const float* w2, const float* bias,
                 const float* x, int ldx, const float* res, int ldr, int R, int N, int K, int split, float* y, int ldy,
                 int y_rows, int reps, int* ksb, int* dirty);
/* Weight-only int8 / int4 on launch_linear (fm_llm_set_quant_compact's kernel forms; bf16): quantises the
   bf16-valued w [N][K] on the device with the model's rule (quant 1: quantize.py's per-channel int8; quant 2:
   group_quantize_tensor, group size gs a multiple of 128 dividing K, K a multiple of 128, no bias), packs the
   bf16 fragments of the quantised weights and the step-granular codes, and runs launch_linear once per form on
   the same operands: y_bf16 from the bf16 fragments, y_q from the codes alone (no bf16 weight is passed).  epi 0
   (store), 1 (residual) or 3 (fp32); x, bias, res, split, ldy, y_rows, reps, ksb as fm_op_linear's; both outputs
   are in/out; dirty sums both forms' leftover tickets.  q_out [N][K] (optional): the codes (int4: 0 .. 15);
   scale_out: int8 [N] row scales, int4 [N][K / gs] group scales with zero_out [N][K / gs] (optional). */
int fm_op_linear_q(int device, int quant, int gs, const float* w, int N, int K, const float* bias, const float* x,
                   int ldx, const float* res, int ldr, int R, int epi, int split, float* y_q, float* y_bf16, int ldy,
                   int y_rows, int reps, int* ksb, int* dirty, int8_t* q_out, float* scale_out, float* zero_out);
/* launch_gemv (R <= 8) on ksb K slices (> 1 only with epi 4 / 5).  idx [R][idx_ld] (optional): column
   idx_col gathers the x rows (pro 1) or the residual rows (epi 5) from a table of idx_rows rows, indices
   clamped into it.  pro 3: x is first finalised by a zero-weight epi-5 launch, which leaves the sums of
   squares the prologue reads (ss_gran 1: the statistic from the staged row instead; R == 1, or R == 2 for bf16 epi 7).  Outputs:
   y [R][N] (epi 7: [R][N / 2]; epi 4: fp32 slabs [ksb][R][ldy], bias in slice 0; epi 5: the finalised
   rows round(res + round(x . w^T + bias)), and ss_out [N / 16][R] their per-tile sums of squares). */
int fm_op_gemv(int device, int precision, int pro, int epi, int ksb, const float* w, const float* w2, const float* bias,
               const float* nw, float eps, const float* x, int ldx, const int32_t* idx, int idx_ld, int idx_col,
               int idx_rows, const float* res, int ldr, int ss_gran, int R, int N, int K, float* y, int ldy, int y_rows,
               float* ss_out, int reps, int* dirty);
/* launch_rowgemv (one row, bf16): kind 0 fin (y = round(res + round(w x + bias)), res row idx[idx_col] of
   [res_rows][ldr]), 1 norm + store, 2 norm + SwiGLU (w rows 8b .. 8b+3 gate, 8b+4 .. 8b+7 up; y [N / 2]),
   3 norm + fp32; kinds 1 / 2 gather their x row idx[idx_col] from [x_rows][ldx].  q8: w is quantised on
   the device by the int8 rule and the codes are streamed (q_out [N][K], scale_out [N] optional). */
int fm_op_rowgemv(int device, int kind, int q8, const float* w, const float* bias, const float* nw, float eps,
                  const float* x, int x_rows, int ldx, const float* res, int res_rows, int ldr, const int32_t* idx,
                  int idx_n, int idx_col, int N, int K, float* y, int y_len, int reps, int8_t* q_out, float* scale_out);
/* launch_rowgemv's two-row forms (fm_tune "fast_pair"; bf16): x [2][K] against one pass over w.  kind 0 fin:
   row 0's residual res0 [N], row 1's the row idx[idx_col] of res1 [res_rows][ldr] (its row 0 without idx);
   kind 1 norm + store: blocks whose 8 rows all lie below skip0 compute row 1 only, and row 0's outputs below
   skip0 are never stored.  y [2][y_ld] in/out. */
int fm_op_rowgemv_pair(int device, int kind, const float* w, const float* bias, const float* nw, float eps, const float* x,
                       const float* res0, const float* res1, int res_rows, int ldr, const int32_t* idx, int idx_n,
                       int idx_col, int skip0, int N, int K, float* y, int y_ld);
/* The two-row forms on weight-only codes (fm_tune "fast_pair_q"): w [N][K] is quantised on the device by the model's
   rule (quant FM_QUANT_INT8: per row; FM_QUANT_INT4: groups of gs) and packed by the model's launchers; then, on the
   same device operands, the two-row launch fills y2 [2][y_ld] and the one-row production launcher, once per row,
   y1 [2][y_ld] (both in/out; row 0 of y1 holds every output, also below skip0).  kind 0 fin (int8, int4), 1 norm +
   store, 2 norm + swiglu (int4; outputs N / 2 wide); operands as fm_op_rowgemv_pair, no bias.  Optional outputs:
   q_out [N][K] (int8 codes, or int4 codes 0..15 one per byte), scale_out [N] ([N][K / gs]), zero_out [N][K / gs]. */
int fm_op_rowgemv_pair_q(int device, int quant, int gs, int kind, const float* w, const float* nw, float eps, const float* x,
                         const float* res0, const float* res1, int res_rows, int ldr, const int32_t* idx, int idx_n,
                         int idx_col, int skip0, int N, int K, float* y2, float* y1, int y_ld, int8_t* q_out, float* scale_out,
                         float* zero_out);
/* The 16-row tile kernel's two-row form on weight-only int8 codes (fm_tune "fast_pair_q" bit 0; PRO_PRENORM with the
   statistic from the staged rows, ss_gran 1): w [N][K] is quantised on the device by the model's rule and packed by
   the model's launcher; then, on the same device operands, the R = 2 launch fills y2 [y2_rows >= 2][ldy] and the R = 1
   production launch, once per row, y1 [2][ldy] (both in/out).  epi 0 (store: wqkv) or 7 (SwiGLU8: w1 || w3 in 8 + 8
   interleaved rows, outputs N / 2 wide); quant FM_QUANT_INT8 only.  Optional outputs: q_out [N][K], scale_out [N]. */
int fm_op_gemv_pair_q(int device, int quant, int epi, const float* w, const float* nw, float eps, const float* x, int N,
                      int K, float* y2, int y2_rows, float* y1, int ldy, int8_t* q_out, float* scale_out);
/* launch_bstream (8 < R <= 32) on bstream_plan's geometry, returned in plan[7] = {acc, kparts, nw, spw,
   tpi, ntm, grid} (acc 1: bsacc_kernel; fm_tune "bstream_acc" 0 or fp32: bstream_kernel).  pro 3 (bsacc,
   epi 0 / 7): the sums of squares come from a zero-weight epi-5 launch over x.  Outputs as fm_op_gemv's,
   slabs [kparts][R][ldy] (no bias: finalize_norm adds it), ss_out [R][ceil(N / 16)]. */
int fm_op_bstream(int device, int precision, int pro, int epi, const float* w, const float* bias, const float* nw,
                  float eps, const float* x, int ldx, const float* res, int ldr, int R, int N, int K, float* y, int ldy,
                  int y_rows, float* ss_out, int reps, int* plan, int* dirty);
/* launch_finalize_norm on caller slabs [kparts][R][lds] (fp32): x_out = round(res + round(sum + bias))
   (wscale: round(round(sum) * wscale) inside), xn_out = RMSNorm(x_out) * nw when nw is given.  fm_tune
   "fin_split" > 1 arms the split form as the batched frame does; split returns whether it ran, err the
   kernel's time-out word. */
int fm_op_finalize_norm(int device, int precision, const float* slab, int kparts, int lds, const float* bias,
                        const float* res, int ldr, const float* nw, const float* wscale, float eps, int d, int R,
                        float* x_out, int ldx, int x_rows, float* xn_out, int ldxn, int xn_rows, int reps, int* split,
                        int* err, int* dirty);
/* launch_prompt_skinny (R <= 64, bf16) on ks = prompt_skinny_ks(N, K, target) K slices (returned; with
   out null nothing else happens): raw fp32 slabs out [ks][R][N] (ldo == N), or with act != 0 (ks 1) the
   SwiGLU of the row-interleaved w straight to out [R][ldo >= N / 2]. */
int fm_op_prompt_skinny(int device, const float* w, const float* x, int ldx, int R, int N, int K, int target, int act,
                        float* out, int out_rows, int ldo, int reps, int* ks);
/* Weight-only int8 / int4 on launch_prompt_skinny (fm_tune "prompt_skinny_q"): quantises the bf16-valued w [N][K]
   on the device with the model's rule (quant FM_QUANT_INT8: per row; FM_QUANT_INT4: groups of gs along K, gs and K
   multiples of 128, else FM_ERR_ARG), packs the bf16 fragments and the step-granular codes with the model's pack
   launchers, and runs the launch once per form on the same x: y_bf16 from the fragments, y_q from the codes alone.
   Shapes, target, act, out_rows, ldo, reps and ks as fm_op_prompt_skinny's; with act the int8 row scales apply in
   the SwiGLU (gate and up are round(round(acc) * scale) first).  Both outputs are in/out.  q_out [N][K] (optional):
   the codes (int4: 0 .. 15); scale_out: int8 [N] row scales, int4 [N][K / gs] group scales with zero_out
   [N][K / gs] (optional). */
int fm_op_prompt_skinny_q(int device, int quant, int gs, const float* w, const float* x, int ldx, int R, int N, int K,
                          int target, int act, float* y_q, float* y_bf16, int out_rows, int ldo, int reps, int* ks,
                          int8_t* q_out, float* scale_out, float* zero_out);
/* Weight-only int8 / int4 on the tiled prompt GEMMs (fm_tune "prompt_gemm_q": launch_conv_gemm as the prompt pass calls
   it for a linear of more than 64 rows): quantises and packs w [N][K] as fm_op_prompt_skinny_q does, and runs the call
   once per form on the same rows x [R][ldx]: y_bf16 from the bf16 fragments of the quantised weights (int8: the row
   scales applied in the epilogue), y_q from the step-granular codes alone.  y = round(acc [* scale] + bias), then
   round(res + y) with res [R][ldr] (bias, res optional); ksplit K slices (1: the GEMM kernel's own epilogue), bf16.
   Both outputs [out_rows >= R][ldo >= N] are in/out.  plan[6]: conv_plan's {kernel (0 the register-tiled kernel, 1 / 2
   the LDS-tiled one at 6 / 8 channel tiles), ksplit, segments, epilogue kernel, rows per segment, kernel of the last
   segment}.  q_out, scale_out, zero_out as fm_op_prompt_skinny_q's. */
int fm_op_prompt_gemm_q(int device, int quant, int gs, const float* w, const float* bias, const float* x, int ldx, int R,
                        int N, int K, const float* res, int ldr, int ksplit, float* y_q, float* y_bf16, int out_rows,
                        int ldo, int reps, int* plan, int8_t* q_out, float* scale_out, float* zero_out);
/* launch_sample_radix once on caller operands (tests/test_gpu_sampler_ops.py): logits [R][ldl >= Nl]
   fp32, row r sampled with the parameters of slot row_slot[r] (the per-slot arrays have `slots`
   entries; seed is 64-bit).  slow != 0: column i < Nl - 1 is token sb + i and column Nl - 1 is im_end,
   the row writes cols[r][0] (token) and [1] (code), with the RAS redraw from ras [slots][10] when
   ras_enable; slow == 0: column i is code i and the row writes cols[r][col_idx] with RNG stream
   `draw`.  A slot with force != 0 emits force_cols [slots][ldc] and copies its logits row to
   tap [slots][tap_ld >= Nl].  cols [R][ldc] and tap are in/out: what the kernel leaves alone comes
   back as the caller filled it.  kernel: 1 sample_fast_kernel, 0 sample_radix_kernel, chosen as in
   production (fm_tune "sampler_fast" and the row width; "sampler_kth" is passed through).  FM_ERR_ARG
   for a row too wide for the sampler's LDS. */
int fm_op_sample(int device, int precision, int slow, const float* logits, int R, int ldl, int Nl,
                 const int32_t* row_slot, int slots, const float* temperature, const float* top_p, const int32_t* top_k,
                 const int32_t* mask_im_end, const uint64_t* seed, const int32_t* step, const int32_t* force, int sb,
                 int se, int im_end, int cb, int draw, int col_idx, const int32_t* ras, int ras_enable,
                 const int32_t* force_cols, int32_t* cols, int ldc, float* tap, int tap_ld, int* kernel);
/* Weight-only int4 on the batched decode linear (8 < R <= 32, bf16; fm_tune "bstream_q4"): quantises
   the bf16-valued w [N][K] on the device with the int4 group rule (quantize.py:57-160, groups of gs
   along K), packs the dequantised bf16 weights, the step-granular codes and the (scale, zero) table,
   and runs the batched linear's plan once per form: y_q4 from the streamed 4-bit codes, y_bf16 from
   the bf16 fragments.  x, epi, the output shapes and kparts as fm_op_batched_linear_q8 (no scale
   epilogue).  Optional outputs: q_out [N][K] codes 0..15, scale_out / zero_out [N][K/gs] (bf16-valued),
   w_deq [N][K] the dequantised bf16 weights.  FM_ERR_ARG unless gs and K are multiples of 128, K a
   multiple of gs, and the shape has an int4-code kernel. */
int fm_op_batched_linear_q4(int device, const float* w, int N, int K, int gs, const float* x, int R, int epi,
                            float* y_q4, float* y_bf16, int* kparts, uint8_t* q_out, float* scale_out,
                            float* zero_out, float* w_deq);
/* the RoPE cos/sin table the library builds on the host (precompute_freqs_cis, llama.py:1003-1022):
   out [seq_len][head_dim/2][2], bf16-valued floats.  No device needed. */
int fm_rope_table(int seq_len, int head_dim, float base, float* out);

/* ---- codec per-op hooks (tests/test_gpu_codec_ops.py): one production launcher of the codec kernels
   on caller operands, prepared by the functions the model itself calls.  fp32 host arrays converted to
   the precision's storage type; every output array is in/out, so what the kernel leaves alone comes
   back as the caller filled it; FM_ERR_ARG for a shape a launcher refuses.  reps (1..8) launches run on the
   same scratch (an in-place kernel gets the caller's values again before each); changed = the output words
   a later launch left different from the first one's. */
/* conv_gemm epilogue flags of fm_codec_conv_desc.flags (bias and the Snake follow the operands) */
#define FM_CE_GELU 2
#define FM_CE_RES 4
#define FM_CE_GAMMA 8
#define FM_CE_STORE 16
#define FM_CE_TANH 64
#define FM_CE_F32OUT 128
#define FM_CE_SWIGLU 256 /* split-K only: out [.][Co / 2] over w = [W1 rows | W3 rows] */
#define FM_CE_ROPE 512   /* split-K only: RoPE on channels [0, rope_nqk) at position t + rope_pos0 */
#define FM_CE_NORM 1024  /* split-K only: out2 = RMSNorm(y) with weight normw */
typedef struct fm_codec_conv_desc {
    int precision;
    /* the layer: w in torch layout per kind -- 0 Conv1d [Co][Ci][k] (dilation dil), 1 ConvTranspose1d
       [Ci][Co][2 stride], 2 ConvTranspose1d [Ci][Co][stride], 3 Linear [Co][Ci].  strided != 0: a Conv1d
       with k = 2 stride run as the encoder runs it, two taps over the [L / stride][stride * Ci] view of x
       (x, Lx, Lq, npre and ldx then describe that view) */
    int kind, Ci, Co, k, stride, dil, strided;
    int npre, Lx, ldx, Lq; /* x [npre + Lx][ldx]: npre carried context rows (lo = -npre), then rows [0, Lx) */
    int flags;
    int ksplit;    /* 0: the split-K factor the model gives such a layer; >= 1: forced */
    int slab_rows; /* 0: a split-K workspace for all Lq rows; else for this many (rows run in segments) */
    int rope_pos0, rope_nqk, rope_hd;
    float rope_base, norm_eps;
    int ldo, out_rows, ldr, res_rows, ldo2, out2_rows;
    int reps; /* launches on the same scratch */
} fm_codec_conv_desc;
/* launch_conv_weight + launch_pack + launch_conv_gemm.  out [out_rows][ldo] (with FM_CE_STORE; fp32
   words with FM_CE_F32OUT), out2 [out2_rows][ldo2] (the Snake with alpha2, or the norm with
   FM_CE_NORM), res [res_rows][ldr]; output row = t * stride + phase for the transposed kinds.  The
   split-K workspace has guard words behind it: dirty = any of them changed.  plan: kernel (0
   conv_gemm, 1 conv_gemm2<6>, 2 conv_gemm2<8>), K slices, row segments, epilogue kernel (0 in the
   GEMM, 1 conv_splitk_epi, 2 conv_splitk_epi_norm), output words a repeated launch changed, the kernel of
   a shorter last row segment (it has a smaller grid; the same as kernel otherwise).  plan [6]. */
int fm_op_codec_conv(int device, const fm_codec_conv_desc* d, const float* w, const float* bias, const float* x,
                     const float* gamma, const float* res, const float* alpha2, const float* normw, float* out,
                     float* out2, int* plan, int* dirty);
/* launch_resunit (bf16): x [npre + L][C] (the Snake of the unit input), k7 / k1 weights [C][C][7] /
   [C][C][1] and biases, the alphas of the inner Snake (a2) and of the output Snake (an), res
   [res_rows][C] in/out (written when store_res), out2 [out2_rows][C].  taken = 0: shape not covered
   (nothing ran); changed = output words a repeated launch changed. */
int fm_op_codec_resunit(int device, int C, int L, int npre, int dil, const float* x, const float* w7, const float* b7,
                        const float* a2, const float* w1, const float* b1, const float* an, float* res, int res_rows,
                        int store_res, float* out2, int out2_rows, int reps, int* taken, int* changed);
/* launch_window_attn: qkv [npre + Tn][3 H hd] (post-RoPE; npre carried rows), out [out_rows][H hd] */
int fm_op_codec_window_attn(int device, int precision, const float* qkv, int Tn, int H, int hd, int window, int npre,
                            float* out, int out_rows, int reps, int* changed);
/* launch_rope_qk in place on qkv [rows >= Tn][3 H hd], row t at position pos0 + t of fm_rope_table */
int fm_op_codec_rope_qk(int device, int precision, float* qkv, int rows, int Tn, int H, int hd, float base, int pos0,
                        int reps, int* changed);
/* launch_window_attn_seg, then launch_kv_roll_seg (the batched streamed decode's attention): n segments
   laid out like a batched pass, segment i at row off[i] (off[0] = 0, off[i+1] = off[i] + T[i] + gap) of
   qkv [span][3 H hd] (post-RoPE) and out [out_rows >= span][H hd] (gap rows are stored as zeros).  state
   [n][state_rows >= window-1][3 H hd], in/out: segment i's carried rows (the last npre[i] in use), one
   device buffer per segment; afterwards its first window-1 rows are the last window-1 rows of (those
   rows, then the segment's T[i] qkv rows). */
int fm_op_codec_window_attn_seg(int device, int precision, int n, const int32_t* T, const int32_t* npre, int gap,
                                const float* qkv, int H, int hd, int window, float* state, int state_rows, float* out,
                                int out_rows);
/* launch_dwconv_ln: x [npre + L][D], depthwise weight [D][7] and bias, LayerNorm weight and bias, y [y_rows][D] */
int fm_op_codec_dwconv_ln(int device, int precision, const float* x, int L, int D, int npre, const float* dw,
                          const float* db, const float* lw, const float* lb, float* y, int y_rows, int reps, int* changed);
/* launch_rvq_decode: codes [nq1][Tn] (>= 0), semantic codebook [sem][cd], residual codebooks
   [nq1 - 1][cbs][cd], folded out_proj w [nq1][D][cd] and bias [nq1][D], z [z_rows][D] */
int fm_op_codec_rvq_decode(int device, int precision, const int32_t* codes, int Tn, int nq1, int sem, int cbs, int cd,
                           const float* cb_sem, const float* cb, const float* w, const float* bias, int D, float* z,
                           int z_rows, int reps, int* changed);
/* launch_snake_inv + launch_snake: y[i] = snake(x[i], alpha[i % C]) for i < n, y [y_len]; ialpha (may be
   null) [C]: the fp32 reciprocals 1 / (alpha + 1e-9) */
int fm_op_codec_snake(int device, int precision, const float* x, int C, int64_t n, const float* alpha, float* y,
                      int64_t y_len, float* ialpha, int reps, int* changed);
/* launch_silu_mul: y[i] = round(silu(g[i])) * y[i] for i < n, y [y_len] */
int fm_op_codec_silu_mul(int device, int precision, const float* g, float* y, int64_t n, int64_t y_len, int reps,
                         int* changed);
/* launch_wn_fold (fp32): w[r][i] = v[r][i] * g[r] / ||v[r]||, w [w_len >= rows * per] */
int fm_op_codec_wn_fold(int device, const float* g, const float* v, int rows, int per, float* w, int64_t w_len, int reps,
                        int* changed);
/* launch_vq_encode (fp32): r [Tn][D] in/out (the residual after the last stage), in_proj wi [nst][cd][D]
   and bi [nst][cd], the codebooks back to back ([cbn[q]][cd] each), out_proj wo [nst][D][cd] and bo
   [nst][D]; codes [nst][Tn] */
int fm_op_codec_vq_encode(int device, float* r, int Tn, int D, int nst, int cd, const float* wi, const float* bi,
                          const float* cb, const int32_t* cbn, const float* wo, const float* bo, int32_t* codes, int reps,
                          int* changed);

/* ---- codec (modded DAC decode side, modded_dac_vq.yaml shapes) --------------------- */
typedef struct fm_codec_config {
    int latent, decoder_dim, n_codebooks, codebook_size, semantic_codebook_size, codebook_dim;
    int t_layers, t_heads, t_head_dim, t_inter, window;
    float rope_base, norm_eps;
} fm_codec_config;

typedef struct fm_codec fm_codec;

int fm_codec_open(const fm_codec_config* cfg, int device, int precision, int max_frames,
                  fm_codec** out);
int fm_codec_set_tensor(fm_codec* h, const char* name, const void* host_data, int src_dtype,
                        int64_t numel);
int fm_codec_synth_tensor(fm_codec* h, const char* name, int64_t numel, uint64_t seed,
                          float center, int log2_half);
int fm_codec_finalize(fm_codec* h);
/* codes: (n_codebooks+1) x T row-major (clamped like rvq.py:354-359, input not mutated);
   pcm: 2048*T floats in [-1, 1]. */
int fm_codec_decode(fm_codec* h, const int32_t* codes, int T, float* pcm);
/* Streamed decode (BASELINE config 5: long-form audio vocoded chunk by chunk while the LLM is
   still generating; the reference decodes each generated segment on its own,
   inference_engine/vq_manager.py:16-21).  The codec is causal end to end, so a stream of chunks
   that carries each causal reader's previous rows (conv inputs, the transformer's window of
   keys/values, the RoPE position) reproduces the one-shot fm_codec_decode of the concatenated
   codes exactly.  The handle's own stream: stream_reset starts it, each decode_chunk appends T
   frames (T <= max_frames) and returns their 2048*T samples.  Concurrent streams (one per
   streamed request, several requests on one handle): stream_open gives a new context with its own
   carried rows and position (starting at zero, like a reset), stream_decode appends to it,
   stream_close frees it; stream_rewind zeroes a context for the next request (a context pool
   needs no allocation, and no hipFree device sync, per request).  Calls on one handle are
   serialised by the caller (one host thread at a time); a context switch rebinds pointers only. */
int fm_codec_stream_reset(fm_codec* h);
int fm_codec_decode_chunk(fm_codec* h, const int32_t* codes, int T, float* pcm);
int fm_codec_stream_open(fm_codec* h, int* stream_id);
int fm_codec_stream_decode(fm_codec* h, int stream_id, const int32_t* codes, int T, float* pcm);
int fm_codec_stream_rewind(fm_codec* h, int stream_id);
int fm_codec_stream_close(fm_codec* h, int stream_id);
/* One causal pass over n stream contexts of this handle.  Segment i is the next T[i] frames of
   stream sids[i].  codes is the segments back to back, each (n_codebooks+1, T[i]) row-major.
   pcm is the segments back to back, 2048*T[i] floats each.
   Afterwards every context is exactly where n calls of the single-stream decode would have left it
   (carried rows and position), and the PCM is theirs bit for bit: every row-independent kernel runs
   once over all segments' rows (gap frames of throw-away rows between segments hold each conv's
   carried rows), the attention reads each segment's carried keys / values from its own context.
   sids are distinct and open.  Id 0, the handle's own stream, is allowed.
   T[i] >= 1, and the positions may differ between segments.
   Fails (FM_ERR_ARG) with nothing changed -- every check runs before the first launch -- on a
   duplicate or unknown id, T[i] < 1, a negative code, a position past the RoPE table, or when the
   segments do not fit: a batch fits when sum(T[i]) + gap*(n-1) <= max_frames (see batch_gap).
   The launch count of profile_read counts a batched pass's GEMM / ResidualUnit launches once,
   like a single-stream pass's. */
int fm_codec_stream_decode_batch(fm_codec* h, int n, const int32_t* sids, const int32_t* codes,
                                 const int32_t* T, float* pcm);
/* Frames of separation a batched pass inserts between segments: the smallest frame count whose
   rows, at every causal conv's level, cover the rows that conv carries (3 for the shipped config). */
int fm_codec_stream_batch_gap(fm_codec* h, int* gap_frames);
int fm_codec_profile_read(fm_codec* h, double* total_ms, int64_t* launches, double* flops);
/* test hook: intermediate of the last decode as fp32, time-major (1 transformer out [T][latent],
   2 first upsample [2T][latent], 3 decoder input [4T][latent]); other stages' buffers are
   reused in place and are not readable. */
int fm_codec_debug_read(fm_codec* h, int stage, int T, float* out);
// Codec ENCODE (voice-clone reference audio -> codes), SURVEY.md §8f row 1.  Replaces
// DAC.encode(audio[B,1,N], audio_lengths) -> (codes[B,C,T], lens) (fish_speech/models/dac/
// modded_dac.py:874-923; caller vq_manager.py:24-52 encode_reference).  enable before
// set_tensor/finalize: adds the encode-side tensors (Encoder, quantizer.downsample,
// quantizer.pre_module, VQ in_proj) to the inventory; encoder_dim 64 and enc_layers 4 for
// modded_dac_vq.yaml.  encode: mono 44.1 kHz fp32 samples (n <= 2048 * max_frames), right-padded
// to a multiple of 2048; codes (caller-owned, (n_codebooks+1) x T row-major, T = ceil(n/2048)).
int fm_codec_enable_encoder(fm_codec* h, int encoder_dim, int enc_layers);
int fm_codec_encode(fm_codec* h, const float* audio, int64_t n, int32_t* codes, int* T_out);
int fm_codec_close(fm_codec* h);

#ifdef __cplusplus
}
#endif
#endif /* FISHMI_H */
