// fm_kernels.h -- kernel argument blocks and launchers (host <-> device seam of libfishmi).
#pragma once
#include <algorithm>
#include "fm_common.h"
#include "fm_tune_table.h"

enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_F32 = 3 };

// Packed weight layout used by every GEMM here: a [N][K] nn.Linear weight is stored as
// [ceil(N/16)][K/32] blocks of 512 elements, each block holding one MFMA 16x32 A-fragment in
// lane order (bf16: lane l's 8 elements at l*8; fp32: elements 0-3 at l*4, 4-7 at 256+l*4), so
// every wave-load instruction reads 1 KB of contiguous memory.
// act[r][j] = round(silu(t[r][16*(j/8) + j%8])) * t[r][16*(j/8) + 8 + j%8]: SwiGLU over the output of
// the row-interleaved W1||W3 (batched path)
template <typename T> void launch_swiglu_i8(hipStream_t s, const T* t, int ldt, T* act, int lda, int inter, int R);
template <typename T> void launch_pack(hipStream_t s, const T* src, int N, int K, T* dst);
// Weight-only int8 (tools/llama/quantize.py:22-52, 190-232).
// quant_rows: per row n of a row-major [N][K] weight w (values as T): m = max(-min(min w, 0),
// max(max w, 0)), s = max(m / 127.5, FLT_EPSILON) in fp32, q = clamp(rint(w / s), -128, 127);
// writes q (int8 row-major), scale[n] = bf16(s) (held in T), and rewrites w with T(q) (exact).
template <typename T> void launch_quant_rows(hipStream_t s, T* w, int N, int K, int8_t* q, T* scale);
// int8 row-major -> T row-major (exact), for the kernels that read T fragments of q
template <typename T> void launch_i8_to(hipStream_t s, const int8_t* q, int64_t n, T* dst);
// int8 row-major [N][K] -> the int8 decode-GEMV layout: [ceil(N/16)][K/64] units of 1 KiB, lane l
// (row l & 15, k-offset 8 * (l >> 4)) holding 8 bytes of k-step 2u then 8 bytes of k-step 2u + 1
void launch_pack_q8(hipStream_t s, const int8_t* src, int N, int K, int8_t* dst);
// int8 row-major [N][K] -> the batched stream's step-granular layout (fm_bstream.hip, 8 < R <= 32):
// [ceil(N/16)][K/32] fragments of 512 B, lane l (row l & 15, k-offset 8 * (l >> 4)) holding its 8
// bytes of that k-step -- the packed bf16 fragments' index order at one byte per weight
void launch_pack_q8s(hipStream_t s, const int8_t* src, int N, int K, int8_t* dst);
// Weight-only int4, groupwise affine (tools/llama/quantize.py:57-160, WeightOnlyInt4QuantHandler
// :352-418), bf16 only.  quant4: per (row, group of gs along K) of a row-major bf16 [N][K] w, the
// reference's group_quantize_tensor in its bf16 arithmetic (every op computed in fp32 and rounded to
// bf16, as torch does): scale = bf16(bf16(max - min) clamped to bf16(1e-6) / 15), zero =
// bf16(min + scale * 8), q = clamp(round_half_even(bf16(bf16(w - (zero - scale * 8)) / scale)), 0, 15);
// writes q (one code per byte, row-major), sz[n][g] = scale bits | zero bits << 16, and rewrites w
// with bf16(fma(q - 8, scale, zero)) (the dequantised weight every bf16 kernel then reads).
void launch_quant4(hipStream_t s, bf16_t* w, int N, int K, int gs, uint8_t* q, uint32_t* sz);
// codes row-major [N][K] -> the int4 decode-GEMV layout: [ceil(N/16)][K/128] units of 1 KiB, lane l
// (row l & 15, k-offset 8 * (l >> 4)) holding word j = the 8 codes of k-step j of the unit, k =
// 128 u + 32 j + 8 (l >> 4) + e: even e at bits 2e (e / 2 nibbles up), odd e at bits 16 + 2(e - 1),
// so (word >> 4p) & 0x000F000F is the pair (e = 2p, 2p + 1) in bf16 mantissa position
// sz [N][K/gs] -> [ceil(N/16)][K/128][16 rows] (gs a multiple of 128: one group per unit)
void launch_pack_q4(hipStream_t s, const uint8_t* q, int N, int K, uint8_t* dst);
// int4 codes (one per byte) [N][K] -> row-major words [N][K / 8]: word j = codes 8j .. 8j+7, the even
// ones in the low half at nibble e / 2, the odd ones in the high half (fm_rowgemv.hip QM 2)
void launch_pack_q4_rows(hipStream_t s, const uint8_t* q, int N, int K, uint32_t* dst);
void launch_pack_sz4(hipStream_t s, const uint32_t* sz, int N, int K, int gs, uint32_t* dst);
// int4 codes row-major [N][K] (one byte per code) -> the batched stream's step-granular layout
// (fm_bstream.hip, 8 < R <= 32): [ceil(N/16)][K/32] fragments of 256 B, lane l's word (row l & 15)
// holding its 8 codes of that k-step, k = 8 * (l >> 4) + e in nibble e (Frag::dq4's order) -- the
// packed bf16 fragments' index order at half a byte per weight.  Rows past N: code 8 (with the
// (scale, zero) = 0 of launch_pack_sz4 they dequantise to 0)
void launch_pack_q4s(hipStream_t s, const uint8_t* q, int N, int K, uint32_t* dst);

template <typename T> struct LinearArgs {
    const T* W;      // [N(padded to 16)][K] row-major (nn.Linear layout)
    const T* W2;     // second weight for EPI_SWIGLU (w3), same shape
    const T* bias;   // [N] or null
    const T* X;      // [R][ldx]
    int ldx, R, N, K;
    T* Y;            // [R][ldy]
    int ldy;
    const T* res;    // residual [R][ldr] (EPI_RESID)
    int ldr;
    float* Yf;       // fp32 output (EPI_F32)
    // split-K (gridDim.y > 1, R <= 16 * NCG): fp32 tile partials [ksb][NACC][R][N] and one arrival
    // counter per 16-row tile (zero between launches; the last-arriving block resets it)
    float* part = nullptr;
    int* tickets = nullptr;
    // weight-only int8 (tools/llama/quantize.py WeightOnlyInt8Linear): W holds the int8 values
    // exactly and every output is round(round(acc) * wscale[n]) (not with EPI_SWIGLU)
    const T* wscale = nullptr;
    // the code-reading forms (bf16; EPI_STORE / EPI_RESID / EPI_F32): W is null and the kernel rebuilds every
    // bf16 weight fragment, bit for bit, from the step-granular code copy right before its MFMAs --
    // Wq8s (launch_pack_q8s, Frag::dq8s), or Wq4s with wsz (launch_pack_q4s / launch_pack_sz4, Frag::dq4s)
    const unsigned char* Wq8s = nullptr;
    const uint32_t* Wq4s = nullptr;
    const uint32_t* wsz = nullptr;
};

template <typename T> struct QkArgs {
    const T* qkv;    // [R][ldqkv]
    int ldqkv;
    const int* row_slot;
    const int* row_pos;
    int fixed_pos;   // >= 0: every row at this position (fast model)
    int nh, nkv, hd, qk_norm;
    float eps;
    const T* qn;
    const T* kn;
    const float* rope;  // [S][hd/2][2] (bf16-valued cos/sin)
    T* qout;         // [R][nh*hd]
    T* kc;
    T* vc;
    size_t slot_stride, layer_off;
    int S;
    // prompt chunks on the skinny GEMM: the QKV projection left qslab_kp fp32 K-slice slabs
    // [kp][R][ldqkv] (no bias) instead of qkv; the kernel reads round(sum + qbias) itself
    const float* qslab = nullptr;
    int qslab_kp = 1;
    const T* qbias = nullptr;
};

template <typename T> struct AttnArgs {
    const T* q;      // [R][nh*hd]
    const int* row_slot;
    const int* row_pos;
    const T* kc;
    const T* vc;
    size_t slot_stride, layer_off;
    int S, nh, nkv, hd, split, maxsplit;
    float scale;
    float* part;     // [R][nh][maxsplit][hd+2]
};

template <typename T> struct FastAttnArgs {
    const T* q;
    const int* row_slot;
    const T* kc;
    const T* vc;
    size_t slot_stride, layer_off;
    int S, nh, nkv, hd, cpos;
    float scale;
    T* out;
};

struct SlotParams {
    float temperature, top_p;
    int top_k, mask_im_end;
    uint64_t seed;
    int step;
    int force;  // teacher forcing (fm_llm_force): the samplers emit force_cols[slot] and tap their logits
};

struct SampleArgs {
    const float* logits;  // [R][ldl]
    int ldl, Nl;
    const int* row_slot;
    const SlotParams* sp;
    const int32_t* ras;   // [slot][ras_stride]
    int ras_stride, ras_enable;
    int slow, sb, se, im_end, cb, draw, col_idx;
    unsigned long long* dbg;  // developer timestamps (fm_tune "debug_ts")
    int32_t* cols;        // [R][ldc]
    int ldc;
    // teacher forcing (SlotParams.force): emitted tokens come from force_cols[slot][ldc] and the
    // logits row is copied to tap + slot * tap_ld (parity hook on the production decode graph)
    const int32_t* force_cols;
    float* tap;
    int tap_ld;
    int kth_fast;  // sample_fast_kernel: try the lane-maxima threshold before the radix search (launcher: fm_tune sampler_kth)
};

template <typename T>
void launch_embed(hipStream_t s, const int32_t* tok, int R, const T* emb, const T* cbemb, int d,
                  int C, int cb, int sb, int se, int scale, T* x, const int* row_slot);
template <typename T>
void launch_gather_rows(hipStream_t s, const int32_t* codes, int ldc, int col, const T* table,
                        int d, int rows, int R, T* x);
template <typename T>
void launch_rmsnorm(hipStream_t s, const T* x, int ldx, const T* w, int d, float eps, T* y,
                    int ldy, int R);
template <typename T> void launch_linear(hipStream_t s, const LinearArgs<T>& a, int epi);
constexpr size_t LINEAR_PART_CAP = (size_t)8 << 20;     // floats of split-K partials (= fm_llm skpart)
int linear_ksb(int N, int K, int R, int nacc, bool can_split);
template <typename T> void launch_qk_rope_cache(hipStream_t s, const QkArgs<T>& a, int R);
template <typename T>
void launch_attn(hipStream_t s, const AttnArgs<T>& a, int R, int nsplit, T* out, bool one_slot);  // one_slot: rows of one prompt
template <typename T> void launch_fast_attn(hipStream_t s, const FastAttnArgs<T>& a, int R);
void launch_finish(hipStream_t s, int R, const int* row_slot, int* row_pos, const int32_t* cols,
                   int ldc, int32_t* tok_in, int32_t* ras, int ras_stride, int C1, int update_ras,
                   SlotParams* sp);
template <typename T>
void launch_synth(hipStream_t s, T* dst, int64_t n, uint64_t seed, uint32_t tid, float center,
                  int log2_half);
template <typename T>
void launch_convert(hipStream_t s, const void* src, int src_bf16, int64_t n, T* dst);

// ---- decode weight-streaming path (fm_gemv.hip), R <= 8 rows --------------------------------
enum { PRO_PLAIN = 0, PRO_NORM = 1, PRO_PRENORM = 3, PRO_FATT = 4 };
// PRO_FATT (fast model, one row, cpos < 16): X' is the fast-model attention output, recomputed by
// every block from the raw QKV row and the cached K/V rows staged in LDS (llama.py:947-975), so
// the Wo GEMV needs no separate attention launch; blockIdx.x == 0 writes the new k / v of cpos.
enum { EPI_SLAB = 4, EPI_SLABFIN = 5, EPI_SWIGLU8 = 7 };
// EPI_SWIGLU8: W is the row-interleaved W1||W3 (each 16-row tile = 8 gate rows then the same 8 up
// rows, see pack_w13 in fm_llm_weights.cpp); a tile yields 8 SwiGLU outputs, N = 2 * intermediate.

template <typename T> struct FastFusedArgs {
    const T* qkv;
    int ldqkv;
    const int* row_slot;
    int nh, nkv, hd, qk_norm;
    float eps;
    const T* qn;
    const T* kn;
    const float* rope;   // [C][hd/2][2]
    T* kc;
    T* vc;
    size_t slot_stride, layer_off;
    int S, cpos;         // S = num_codebooks (fast cache length)
    float scale;
    T* out;              // [R][nh*hd]
    unsigned long long* dbg;  // developer timestamps (fm_tune "debug_ts")
    float* qdbg = nullptr;    // per-op test hook (fm_op_qk_rope): q after qk-norm + RoPE [R][nh][hd]
    int nwb = 4;              // attn_fd: waves per block (4, 8 or 16; 16 nwb positions per pass)
    // batched frames (fm_tune bs_qkv_slab): the QKV projection left qslab_kp fp32 K-part slabs
    // [kp][R][ldqkv] (no bias) instead of qkv; the attention reads round(sum + qbias) itself
    const float* qslab = nullptr;
    int qslab_kp = 1;
    const T* qbias = nullptr;
    const int* row_pos = nullptr;  // fattn_wo_kernel: the frame's position (its hand-off tag)
    int noq = 0;  // fast_attn2_kernel, cpos == 0 (fm_tune rowgemv bit 6): one position, so the output is 0 + v: the
                  // Q rows of qkv are not read (the projection did not compute them); k / v are cached as ever
};
template <typename T> struct GemvArgs {
    const T* W;
    const T* W2;             // EPI_SWIGLU: w3
    const T* bias;
    const T* X;              // [R][ldx] (or a table gathered by xidx)
    int ldx;
    const int32_t* xidx;     // optional row gather: X row = xidx[r*xidx_ld + xidx_col]
    int xidx_ld, xidx_col;
    int xidx_rows;           // rows of the gathered table: indices are clamped into it (0: unchecked)
    const int32_t* residx;   // optional row gather for res (same layout as xidx)
    const T* res;            // EPI_SLABFIN residual [R][ldr]
    int ldr;
    const float* ss_in;      // PRO_PRENORM: per-16-column-tile sums of squares of X [K/16][R]
    int ss_gran;             // PRO_PRENORM: 0 ss_in as above; 1 the statistic from the staged row itself (R == 1, whole K)
    const T* nw;             // norm weight [K]
    float eps;
    int R, N, K;
    T* Y;                    // EPI_STORE / EPI_SWIGLU [R][ldy]
    int ldy;                 // also the slab row stride for EPI_SLAB / EPI_F32
    float* Yf;               // EPI_F32 [R][ldy] | EPI_SLAB(FIN) partials [KSB][R][ldy]
    T* res_out;              // EPI_SLABFIN: x = round(res + round(sum of partials)) [R][ldro]
    int ldro;
    float* ss_out;           // EPI_SLABFIN: per-tile sums of squares of x [N/16][R]
    int* tickets;            // EPI_SLABFIN: per-tile arrival counters (zero between launches)
    T* xn_out;               // optional (ksb == 1): block (0,0) stores X' (normalised row) here
    int ldxo;
    unsigned long long* dbg; // developer timestamps (fm_tune "debug_ts"); null in production
    FastFusedArgs<T> att;    // PRO_FATT: the fast-model attention the prologue recomputes
    int fatt_off;            // PRO_FATT: byte offset of the attention staging area in LDS (launcher)
    // weight-only int8: Wq replaces W (packed [tiles][K/64][64 lanes][16 B], fm_kernels.h) and
    // each output is round(round(acc) * wscale[packed row]) (WeightOnlyInt8Linear, quantize.py:228-229)
    const unsigned char* Wq;
    const T* wscale;
    // weight-only int4 (bf16): Wq holds 4-bit codes ([tiles][K/128][64 lanes][16 B], launch_pack_q4)
    // and wsz each (tile, 128-k unit, row)'s group (scale, zero) as bf16 pairs (launch_pack_sz4)
    const uint32_t* wsz;
    int q4_xsum_off;  // int4: LDS byte offset of the per-(128-k unit, x row) sums (launcher)
    // optional KV prefetch (batch-1 QKV GEMV, fm_tune kv_prefetch): while the weights stream, the
    // cached K / V rows the next attention launch reads (positions 0 .. pos of row 0's slot) are
    // pulled into L2: block b loads kv head b % pf_nkv, which under round-robin workgroup placement
    // is the XCD that attention block (kv head h = XCD h) runs on.  Speed only, never correctness.
    const T* pf_kc;          // null: off
    const T* pf_vc;
    const int32_t* pf_slot;  // row 0's slot / position (device, as the attention reads them)
    const int32_t* pf_pos;
    size_t pf_slot_stride, pf_layer_off;
    int pf_S, pf_nkv, pf_hd;
    int dummy_tail;  // ring slots past the wave's run load one fixed fragment (else the run's last)
};
// developer knobs (fm_tune): one int field per entry of fm_tune_table.h, in its order
struct FmTuning {
#define FM_KNOB(name, def, ...) int name = def;
#include "fm_tune_table.h"
#undef FM_KNOB
    unsigned long long* dbg = nullptr;  // device buffer of per-block phase timestamps (debug_ts)
    unsigned epoch = 0;      // bumped by every fm_tune call but debug_ts: what was derived under older knobs (the QKV table) is rebuilt
};
FmTuning& fm_tuning();
// Voice prefix cache (fm_prefix.hip): rows [0, npos) of every (layer, K | V, kv head) of the listed
// slots' slow caches <-> one compact store [layer][K|V][kv head][npos][hd]; strides in bytes.
struct KvPrefixArgs {
    char *kc, *vc;       // the slow K / V caches [slot][layer][kv head][S][hd]
    char* store;         // the prefix entry
    const int* slots;    // device: the slots of the call (blockIdx.z indexes it)
    size_t slot_stride_b, layer_stride_b, head_stride_b;
    size_t run_bytes;    // npos * hd * element size
    int64_t run_units;   // (launcher) run_bytes in access units
    int nkv;
    int to_store;        // 1: slot -> store (save), 0: store -> slots (load)
};
void launch_kv_prefix_copy(hipStream_t s, const KvPrefixArgs& a, int n_layer, int nslots);
// PRO_FATT staging: raw q|k|v row, cached K/V rows [nkv][2][S-1][hd], qk-norm weights, RoPE row
inline size_t fatt_lds_bytes(int ldqkv, int nkv, int S, int hd, size_t esz) {
    return ((size_t)ldqkv + (size_t)nkv * 2 * (S - 1) * hd + 2 * (size_t)hd) * esz + (size_t)hd * 4 + 64;
}
inline size_t gemv_lds_bytes(int R, int Kb, size_t esz) {
    return (size_t)R * (Kb + 8) * esz + 16 * sizeof(float) + (2 * 8 * 16 + 16) * (size_t)R * sizeof(float) +
           8 * 8 * sizeof(float);
}
template <typename T> void launch_gemv(hipStream_t s, const GemvArgs<T>& a, int pro, int epi, int ksb);
// batch-1 row-block GEMV (fm_rowgemv.hip): row-major bf16 W [N][K], RP rows per 256-thread block.
//   ROWGEMV_FIN        (wo / w2, RP 2): y = round(res + round(W x + bias)) into res_out (its RMSNorm
//                      consumer: GemvArgs::ss_gran = 1)
//   ROWGEMV_NORM_STORE (wqkv, RP 8): x' = RMSNorm(x) * nw in the prologue, y = round(W x' + bias) into
//                      Y, optional KV prefetch (GemvArgs::pf_kc semantics)
//   ROWGEMV_NORM_SWIGLU (w1 || w3, RP 8: rows 8b .. 8b+3 = W1 rows 4b .. 4b+3, rows 8b+4 .. 8b+7 the same
//                      rows of W3): x' = RMSNorm(x) * nw, y[4b + t] = round(silu(round(g))) * round(u) into Y
//   ROWGEMV_NORM_F32   (a head, RP 8): x' = RMSNorm(x) * nw, Yf[n] = fp32 holding round(W x')
enum { ROWGEMV_FIN = 0, ROWGEMV_NORM_STORE = 1, ROWGEMV_NORM_SWIGLU = 2, ROWGEMV_NORM_F32 = 3 };
struct RowGemvArgs {
    const bf16_t* W;
    const int8_t* Wq;         // weight-only int8 (instead of W): row-major codes, output round(round(acc) * wscale)
    const bf16_t* wscale;     // int8: per-row scales [N]
    const uint32_t* Wq4;      // weight-only int4 (instead of W): packed row-major codes [N][K / 8] (launch_pack_q4_rows)
    const uint32_t* wsz;      // int4: (scale, zero) bf16 pairs [N][K / gs]
    int gs;                   // int4: group size
    const bf16_t* X;          // [K] (or a table [.][ldx] gathered by xidx[xcol], clamped to xrows; not FIN)
    int ldx;                  // (0: K)
    const int32_t* xidx;
    int xcol, xrows;
    const bf16_t* bias;       // [N] or null
    const bf16_t* nw;         // NORM: norm weight [K]
    float eps;
    const bf16_t* res;        // FIN: residual table [.][ldr] (row 0, or residx[res_col] clamped to res_rows)
    int ldr;
    const int32_t* residx;
    int res_col, res_rows;
    bf16_t* res_out;          // FIN: [N]
    bf16_t* Y;                // STORE / SWIGLU: [N] ([N / 2])
    float* Yf;                // F32: [N]
    int N, K;
    const bf16_t* pf_kc;      // STORE: KV prefetch (null: off), as GemvArgs
    const bf16_t* pf_vc;
    const int32_t* pf_slot;
    const int32_t* pf_pos;
    size_t pf_slot_stride, pf_layer_off;
    int pf_S, pf_nkv, pf_hd;
    unsigned long long* dbg;  // developer timestamps (launcher: fm_tune debug_ts)
    // two activation rows against one pass over the weights (fm_tune fast_pair: bf16 FIN / NORM_STORE; fast_pair_q: int8 FIN,
    // int4 FIN / NORM_STORE / NORM_SWIGLU; no x gather):
    // xr = 2, row 1's x, residual row (residx gathers this row only; row 0's is res as it stands), and outputs.
    // NORM_STORE: blocks whose rows all lie in [0, skip0) compute row 1 only, and row 0's outputs below skip0
    // are never stored (the Q rows of codebook 0's pass)
    int xr;
    const bf16_t* X1;
    const bf16_t* res1;
    bf16_t* res_out1;
    bf16_t* Y1;
    int skip0;
};
int rowgemv_u(int K, int qm);  // per-wave chunk depth for K (qm 1: int8 codes; 0: not eligible)
void launch_rowgemv(hipStream_t s, const RowGemvArgs& a, int kind);
// whether the two-row form (RowGemvArgs::xr = 2) of this kind exists at depth K (kind -1: the fused attention + wo pair form)
// on bf16 weights (qm 0), int8 (1) or int4 (2) codes
bool rowgemv_pair_ok(int kind, int K, bool gathered, int qm = 0);
// batch-1 fast-model attention + wo in one launch (fm_rowgemv.hip fattn_wo_kernel; wo in bf16, int8 or int4): the
// attention blocks store their output as tagged words (bf16 << 16 | gen) into xt [nh * hd]; the wo
// row-pair blocks (RowGemvArgs FIN; its X is unused) poll them.  gen: the launch's index in the
// frame, 1..40; the tag is (row_pos[0] * 41 + gen) % 65535 + 1 (at.row_pos: the frame's position);
// err: set when a wait timed out.
struct FattnWoArgs {
    FastFusedArgs<bf16_t> at;
    RowGemvArgs wo;
    uint32_t* xt;
    int gen;
    int* err;
    int delay;                // wo blocks wait this many 10-ns ticks before their weight loads (fm_tune fw_delay)
    int cheap;                // 1: poll one word per 32-element group before the full read (fm_tune fw_cheap)
    int prio;                 // 1: attention waves at s_setprio 3 (fm_tune fw_prio)
    int ilp;                  // 1: the attention chain without serial per-position blocks (fm_tune fattn_ilp)
    unsigned long long* dbg;  // developer records (launcher: fm_tune debug_ts)
    // fm_tune rowgemv bit 5 / fast_dead_q bit 0 (the first fast layer at codebook > 0): the attention blocks take the raw q|k|v
    // row from qtab [qrows][at.ldqkv], row qidx[qcol] clamped into it, instead of at.qkv (no QKV launch ran)
    const bf16_t* qtab;
    const int32_t* qidx;
    int qcol, qrows;
    // fm_tune rowgemv bit 6 / fast_dead_q bit 1 (at.cpos == 0): Q was not computed; the attention output is 0 + v
    int kv0;
    // fm_tune fast_pair / fast_pair_q (at.cpos == 1): codebook positions 0 and 1 in one launch; at.qkv holds two rows
    // (row 0: the K / V part only), qtab set: row 1's row comes from the table instead.  1: both rows' outputs
    // go to xt (2 K words) and wo runs on two rows (RowGemvArgs::xr = 2); 2 (the last layer): row 0 ends at
    // its K / V cache write and wo runs on row 1 alone (A.wo: row 1's residual and output)
    int pair;
};
bool fattn_wo_ok(int nh, int nkv, int hd, int cpos, int N, int K, int qm);
// ... and whether its table / K-V-only forms (qtab, kv0) exist and stay resident at depth K (fm_tune fast_dead_q)
bool fattn_wo_dead_ok(int K, int qm);
void launch_fattn_wo(hipStream_t s, const FattnWoArgs& a);
// batch-1 GEMV chain (fm_gemv.hip gemv_chain_kernel): 2..GEMV_CHAIN_MAX dependent GEMVs in one launch,
// whole K per block, one row.  Stage kinds: wo / w2 (PRO_PLAIN, EPI_SLABFIN; the residual may be a
// gathered row), w1||w3 (PRO_PRENORM, EPI_SWIGLU8), qkv (PRO_PRENORM, EPI_STORE), and as the last
// stage only, a head (PRO_PRENORM, EPI_F32; its outputs are read by later launches).  cnt: GEMV_CHAIN_WORDS zeroed words (the launch
// leaves them zeroed); err: set when a wait timed out.
constexpr int GEMV_CHAIN_MAX = 4;
constexpr int GEMV_CHAIN_LINE = 32;  // counter words one 128-B line apart
constexpr int GEMV_CHAIN_SLOTS = 17;  // per stage: 8 arrival shards, 1 top word, 8 done replicas
constexpr int GEMV_CHAIN_WORDS = GEMV_CHAIN_MAX * GEMV_CHAIN_SLOTS * GEMV_CHAIN_LINE;
enum { GEMV_CHAIN_WO_W2 = 0, GEMV_CHAIN_W13 = 1, GEMV_CHAIN_QKV = 2, GEMV_CHAIN_HEAD = 3 };
template <typename T> struct GemvChainArgs {
    GemvArgs<T> st[GEMV_CHAIN_MAX];
    int kind[GEMV_CHAIN_MAX];
    int off[GEMV_CHAIN_MAX + 1];
    int n;
    unsigned* cnt;
    int* err;
    int sleep;  // s_sleep between polls (fm_tune chain_sleep)
};
template <typename T> void launch_gemv_chain(hipStream_t s, const GemvChainArgs<T>& c);

// ---- batched decode weight streaming with register-resident X, 8 < R <= 32 (fm_bstream.hip) ---
template <typename T> struct BstreamArgs {
    const T* W;      // packed MFMA-fragment layout [tiles][K/32][512]
    const T* bias;   // [N] or null (EPI_STORE / EPI_F32; EPI_SLAB leaves it to finalize_norm)
    const T* X;      // [R][ldx]
    int ldx, R, N, K;
    T* Y;            // EPI_STORE / EPI_SWIGLU8 [R][ldy]
    int ldy;         // also the row stride of Yf
    float* Yf;       // EPI_F32 [R][ldy] | EPI_SLAB partial slabs [kparts][R][ldy]
    int kparts = 1;  // set by the launcher from the plan
    const T* wscale = nullptr;  // weight-only int8 row scales (EPI_SLAB: applied by finalize_norm)
    unsigned long long* dbg = nullptr;  // developer per-block timestamps (fm_tune "debug_ts")
    // bsacc_kernel only -- PRO_PRENORM: X' = RMSNorm(X) from the producer's per-tile sums of squares
    // ss_in [R][K/16] and the norm weight nw (llama.py:989-1000); EPI_SLABFIN: the last-arriving K
    // part of each tile group finalises x = round(res + round(sum of partials)) into res_out and
    // its per-tile sums of squares ss_out [R][N/16] (tickets: zero between launches).  (The batch-1
    // GEMV's tile sums are [tiles][R]; the two chains never exchange them.)
    int pro = 0;
    const float* ss_in = nullptr;
    const T* nw = nullptr;
    float eps = 0.f;
    const T* res = nullptr;
    int ldr = 0;
    T* res_out = nullptr;
    int ldro = 0;
    float* ss_out = nullptr;
    int* tickets = nullptr;
    int dummy_tail = 0;  // bsacc: ring slots past the block's tiles / steps load one cached fragment
    int xfirst = 1;      // bsacc: X (and the PRENORM operands) issued before the weight ring (fm_tune bs_xfirst)
    int vec_epi = 1;     // bsacc: epilogue items of 4 rows (16-byte LDS reads, 8 / 16-byte stores; fm_tune bs_vec_epi)
    // weight-only int8 (fm_tune bstream_q8): the step-granular code copy of W, [tiles][K/32][64 lanes][8 B]
    // (launch_pack_q8s).  Set: bsacc_kernel streams it instead of W where bsacc_q8_ok, else W as ever.
    const unsigned char* Wq8 = nullptr;
    // weight-only int4 (fm_tune bstream_q4): the step-granular code copy of W, [tiles][K/32][64 lanes] words
    // (launch_pack_q4s), and each (tile, 128-k unit, row)'s (scale, zero) (launch_pack_sz4).  Both set:
    // bsacc_kernel streams them instead of W where bsacc_q4_ok, else W as ever.
    const uint32_t* Wq4 = nullptr;
    const uint32_t* wsz = nullptr;
};
struct BstreamPlan {
    bool ok = false;
    int kparts = 1, nw = 0, spw = 0, tpi = 1, grid = 0;
    int acc = 0, ntm = 0;  // bsacc_kernel: tiles per block at most (register accumulators)
};
// (acc_default: plan as under fm_tune bstream_acc 1 whatever the knob says -- a compact handle, fm_llm_model.h)
BstreamPlan bstream_plan(int N, int K, int R, int epi, size_t esz, bool acc_default = false);
// whether launch_bstream has an int8-code form (BstreamArgs::Wq8) for this plan, epilogue and prologue
bool bsacc_q8_ok(const BstreamPlan& p, int epi, int pro, size_t esz);
// ... and an int4-code form (BstreamArgs::Wq4 / wsz): the same forms, K in whole 128-k units
bool bsacc_q4_ok(const BstreamPlan& p, int epi, int pro, size_t esz, int K);
void bsacc_init();  // kernel attributes (> 64 KiB LDS) of every bsacc_kernel, outside any capture
template <typename T> bool launch_bstream(hipStream_t s, const BstreamArgs<T>& a, int epi, const BstreamPlan& p);
// x_out = round(res + round(sum of kparts slabs + bias)); if nw: xn_out = RMSNorm(x_out) * nw
template <typename T> struct FinalizeArgs {
    const float* slab;  // [kparts][R][lds]
    int kparts, lds;
    const T* bias;      // [d] or null
    const T* res;       // [R][ldr]
    int ldr;
    T* x_out;           // [R][ldx] (may alias res)
    int ldx;
    const T* nw;        // norm weight [d] or null (no norm)
    float eps;
    T* xn_out;          // [R][ldxn]
    int ldxn, d, R;
    const T* wscale = nullptr;  // weight-only int8: round(res + round(round(sum) * wscale[n]))
    // split form (fm_tune fin_split = ch > 1): each row over ch blocks that meet on cnt[2 r .. 2 r + 1]
    // (zero between launches) after publishing their chunk's sum of squares to ss_part[r][ch]
    int ch = 0;
    int* cnt = nullptr;
    float* ss_part = nullptr;
    int fin8 = 0;       // set by the launcher (fm_tune fin8): eight K parts' slab loads in one round trip
    int* err = nullptr; // split form: set when a row's blocks timed out waiting for each other
};
template <typename T> void launch_finalize_norm(hipStream_t s, const FinalizeArgs<T>& a);

// ---- fused decode attention / sampler (fm_attn.hip) ------------------------------------------
// prompt-chunk linear at 32 < R <= 64 rows, bf16 (fm_prompt.hip): raw fp32 K-slice partials into the
// conv split-K slab layout [ks][R][N]; the conv split-K epilogue finishes it
struct PromptSkinnyArgs {
    const bf16_t* w;   // packed weight [ceil(N/16)][K/32][512]
    const bf16_t* x;   // activation rows [R][ldx]
    int ldx, R, N, K;
    float* slab;       // [ks][R][N]
    // one slice and act set: no slab, the interleaved SwiGLU of the row-interleaved W1 || W3 stored
    // straight to act [R][lda] (swiglu_i8_kernel's roundings)
    bf16_t* act = nullptr;
    int lda = 0;
    // weight-only int8 with act: the row scales of the packed (interleaved) rows [N]; gate and up are
    // round(round(acc) * wscale[n]) before the SwiGLU (linear_epi's STORE, then swiglu_i8_kernel)
    const bf16_t* wscale = nullptr;
    // the code-reading forms: w is null and the kernel rebuilds every bf16 fragment, bit for bit, from the
    // step-granular code copy right before its MFMAs -- q8s (launch_pack_q8s, Frag::dq8s), or q4s with sz
    // (launch_pack_q4s / launch_pack_sz4, Frag::dq4s; K a multiple of 128)
    const unsigned char* q8s = nullptr;
    const uint32_t* q4s = nullptr;
    const uint32_t* sz = nullptr;
};
void launch_prompt_skinny(hipStream_t s, const PromptSkinnyArgs& a, int ks);
// K slices: the smallest divisor of K/32 with >= 8 k-steps per slice giving >= target blocks of 64
// rows (the largest such when none does; 0 when K / 32 < 8)
int prompt_skinny_ks(int N, int K, int target);

template <typename T> struct AttnDecArgs {
    const T* qkv;        // raw projections [R][ldqkv] (q heads, k heads, v heads)
    int ldqkv;
    const int* row_slot;
    const int* row_pos;
    int nh, nkv, hd, qk_norm;
    float eps;
    const T* qn;
    const T* kn;
    const float* rope;   // [S][hd/2][2]
    T* kc;
    T* vc;
    size_t slot_stride, layer_off;
    int S, maxsplit;
    float scale;
    float* part;         // [R][nh][maxsplit][hd+2]
    // attn_decode2 only
    int cap;             // rows per block
    int* cnt;            // arrival tickets [R][nkv] (attn_fd: [R][nh]), zeroed at allocation, reset by the last block
    T* out;              // [R][nh*hd]
    unsigned long long* dbg;  // developer timestamps (fm_tune "debug_ts")
    float* qdbg = nullptr;    // per-op test hook (fm_op_qk_rope): q after qk-norm + RoPE [R][nh][hd]
    int nwb = 4;              // attn_fd: waves per block (4, 8 or 16; 16 nwb positions per pass)
    int hpb = 4;              // attn_fd: q heads of a kv head per block (1, 2, or 4 = all of them; fm_tune fd_hpb)
    const float* qslab = nullptr;  // as FastFusedArgs: K-part slabs of the QKV projection (attn_fd)
    int qslab_kp = 1;
    const T* qbias = nullptr;
};
// decode attention for the small-batch path (see fm_attn.hip): a.cap rows per block, a.maxsplit =
// ceil(S / cap) blocks per (row, kv head), output straight to a.out (bf16 / T)
template <typename T> void launch_attn_decode2(hipStream_t s, const AttnDecArgs<T>& a, int R);
inline size_t attn2_lds_bytes(int hd, int g, int cap, size_t esz) {
    return (size_t)cap * (hd + 8) * esz + (size_t)cap * hd * esz + (size_t)g * hd * 4 + (size_t)g * cap * 4 +
           16 + 8 * (size_t)g * 4;
}
// rows per attn_decode2 block within ~150 KB of LDS (multiple of 16, <= 256)
inline int attn2_cap(int hd, int g, size_t esz) {
    long budget = 150L * 1024 - 16 - 8L * g * 4 - (long)g * hd * 4;
    long per = (long)(2 * hd + 8) * (long)esz + 4L * g;
    long c = budget / per;
    c = c > 256 ? 256 : c;
    return (int)(c & ~15L);
}
// decode attention v3 (fm_attn.hip attn_dec3_kernel): 64 positions per block in registers,
// maxsplit set by the launcher (ceil(S / 64)); a.part must hold [R][nh][ceil(S / 64)][hd + 2]
// flash-decode attention (fm_attn.hip attn_fd_kernel), every batch size: splits of at least a.cap
// (>= 16) positions, at most FD_NSP per (row, kv head); maxsplit set by the launcher; a.part must
// hold [R][nh][min(FD_NSP, ceil(S / cap))][hd + 2], a.cnt [R][nh] zeroed tickets (one per row, kv head
// and group of a.hpb q heads)
constexpr int FD_NSP = 16;
inline bool attn_fd_ok(int hd, int g) { return (hd == 32 || hd == 64 || hd == 128) && g >= 1 && g <= 4; }
template <typename T> void launch_attn_fd(hipStream_t s, const AttnDecArgs<T>& a, int R);
// batch-1 slow-model attention + wo in one launch (fm_rowgemv.hip slow_attn_wo_kernel; bf16 compute: unquantised
// weights under fm_tune slow_attn_wo, weight-only int8 / int4 codes under slow_attn_wo_q -- wo.Wq + wscale or wo.Wq4 +
// wsz + gs select the form, as in launch_fattn_wo, and take no bias).  The lowest at.nh * maxsplit linear block indices are attn_fd's blocks at 8 waves and one q head per
// block (at.cap = the minimum split, as launch_attn_fd takes it; the launcher sets maxsplit, nwb and hpb), storing
// their output as tagged words (bf16 << 16 | gen) into xt [nh * hd] instead of at.out; the remaining blocks hold two
// 4-wave wo row blocks of rp rows each (RowGemvArgs FIN, plain residual; X is only a valid dummy address).  gen: the
// launch's index in the frame, 1..40; the tag is (row_pos[0] * 41 + gen) % 65535 + 1; err: set when a wait timed out.
struct SlowAttnWoArgs {
    AttnDecArgs<bf16_t> at;
    RowGemvArgs wo;
    uint32_t* xt;
    int gen;
    int* err;
    int rp;  // wo rows per 4-wave group: 2 (fm_tune slow_attn_wo / slow_attn_wo_q 1) or 4 (2)
    // how the wo waves wait (speed only): delay_pct, per cent of the attention's duration as estimated from the
    // position, before a wave's first read of x (rp 4 only: its whole grid starts together; fm_tune slow_aw_delay);
    // sleep, the s_sleep argument between reads (slow_aw_sleep); cheap, one word per 128 elements polled ahead of
    // the full reads (slow_aw_cheap)
    int delay_pct, sleep, cheap;
};
// qm: 0 bf16 weights, 1 int8 codes, 2 int4 code words (512-k chunks: the depth is rowgemv_u(K, qm))
bool slow_attn_wo_ok(int nh, int nkv, int hd, int N, int K, int qm = 0);
void launch_slow_attn_wo(hipStream_t s, const SlowAttnWoArgs& a);
template <typename T> void launch_attn_decode3(hipStream_t s, const AttnDecArgs<T>& a, int R);
template <typename T> void launch_fast_attn_fused(hipStream_t s, const FastFusedArgs<T>& a, int R);
// fast-model attention, one wave per q head (cpos < 16 cached rows, hd <= 256)
template <typename T> void launch_fast_attn2(hipStream_t s, const FastFusedArgs<T>& a, int R);
template <typename T> void launch_sample_radix(hipStream_t s, const SampleArgs& a, int R);
int sample_fast_max_row();  // widest row sample_fast_kernel takes (wider rows: sample_radix_kernel)
void sample_init();  // sampler kernel attributes (dynamic LDS past 64 KiB), outside any capture
template <typename T>
void launch_attn_combine(hipStream_t s, const float* part, const int* row_pos, int R, int nh, int hd,
                         int split, int maxsplit, T* out);
