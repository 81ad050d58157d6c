// fm_rowgemv.hip -- batch-1 row-block GEMV for the decode linears whose 16-row tile grids leave
// CUs idle or unbalanced.
//
// wo and w2 of a decode layer (TransformerBlock.forward, /root/reference/fish_speech/models/
// text2semantic/llama.py:838-843: h = x + attention(...), out = h + feed_forward(...)) have
// N = dim = 2560 output rows at S2-Pro shapes, and wqkv N = 6144 (Attention.forward, :883-890).  On
// the 16-row MFMA tile kernel (fm_gemv.hip) that is 160 workgroups for 256 CUs (96 CUs idle, each
// busy CU streaming 131 KiB / 311 KiB at the ~26 GB/s per CU its loads in flight sustain) and 384
// workgroups (half the CUs doing two tiles).  Here one 256-thread block owns RP consecutive rows
// (wo / w2: RP = 2, 1280 blocks = 5 per CU; wqkv: RP = 8, 768 blocks = 3 per CU) and reads them
// straight from the row-major weight: for each 256-k chunk of its wave's K range a lane loads 4 bf16
// of each of the RP rows and the matching 4 x values (coalesced 512-B wave loads) and accumulates
// two v_dot2c_f32_bf16 per row.  The whole run of a wave is in flight at once (U chunks,
// U = ceil(K / 256 / 4) <= 12), so there is no ring refill.  No MFMA: at one activation row the
// matrix cores would do 1/16 useful work; the dot2 work is 2 VALU instructions per row per chunk.
//
// Prologue  PLAIN     x as loaded
//           PRENORM   x' = round(round(x * rs) * w_norm), rs = 1 / sqrt(mean(x^2) + eps) over the
//                     whole row (RMSNorm, llama.py:989-1000): each wave sums the squares of its
//                     chunks, one LDS exchange, every block computes the same statistic in the same
//                     order.  x and w_norm are loaded ahead of the weights (in-order vmcnt).
// Epilogue  FIN       y = round(res + round(acc + bias)) into res_out (fm_gemv.hip EPI_SLABFIN
//                     semantics, llama.py:841-842); its RMSNorm consumer takes the statistic from
//                     the row it stages (GemvArgs::ss_gran = 1), so no sums of squares are written
//           STORE     y = round(acc + bias) into Y (wqkv), plus the KV prefetch of fm_gemv.hip
//                     (GemvArgs::pf_kc): the next attention's cached K / V sectors pulled into L2.
#include "fm_common.h"
#include "fm_kernels.h"
#include "fm_runtime.h"
#include "fm_attn_fd_dev.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;

// acc += w . x over 4 bf16 (two v_dot2c_f32_bf16); whole-vector bit casts, so the compiler emits v_dot2c_f32_bf16 on the loaded registers
__device__ __forceinline__ float dot4(u32x2_t w, u32x2_t x, float acc) {
    const bf16x4_t wb = __builtin_bit_cast(bf16x4_t, w), xb = __builtin_bit_cast(bf16x4_t, x);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(wb, wb, 0, 1), __builtin_shufflevector(xb, xb, 0, 1),
                                          acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(wb, wb, 2, 3), __builtin_shufflevector(xb, xb, 2, 3),
                                          acc, false);
    return acc;
}
__device__ __forceinline__ float lo16(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi16(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// acc += w . x over 8 bf16 pairs (v_dot2c_f32_bf16); whole-vector bit casts
__device__ __forceinline__ float dot8r(u32x4_t w, u32x4_t x, float acc) {
    const bf16x8_t wb = __builtin_bit_cast(bf16x8_t, w), xb = __builtin_bit_cast(bf16x8_t, x);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(wb, wb, 0, 1), __builtin_shufflevector(xb, xb, 0, 1),
                                          acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(wb, wb, 2, 3), __builtin_shufflevector(xb, xb, 2, 3),
                                          acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(wb, wb, 4, 5), __builtin_shufflevector(xb, xb, 4, 5),
                                          acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(wb, wb, 6, 7), __builtin_shufflevector(xb, xb, 6, 7),
                                          acc, false);
    return acc;
}
__device__ __forceinline__ void ld_pair_bf(const bf16_t* p, float& x0, float& x1) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    x0 = lo16(w);
    x1 = hi16(w);
}

// G: the residual row is gathered (residx; the fast model's first layer), whose index load the
// residual load must wait for -- the compiler hoists that pair ahead of the weight loads (one round
// trip), so the plain form keeps it out of the kernel entirely.
// QM 1 (weight-only int8, WeightOnlyInt8Linear, /root/reference/tools/llama/quantize.py:212-240):
// W is the int8 row-major matrix, a chunk is 512 k (8 codes = 8 B per lane per row, x 16 B), the
// codes become floats exactly (byte ^ 0x80 -> v_cvt_f32_ubyte = q + 128, the 128 * sum(x) taken off
// once at the end) and each output is round(round(acc) * scale[row]) (quantize.py:228-229).
// QM 2 (weight-only int4, group size gs a multiple of 8; quantize.py:57-160 group quantization):
// W is the packed row-major code matrix (one 32-bit word = 8 codes, the even ones in the low half),
// a chunk is 512 k (one word per lane per row); each code pair becomes the exact bf16 pair
// (128 + q) by one mask-and-or, two v_dot2c per word pair give B = sum x (128 + q) over the lane's
// 8 k (inside one group), and the group's affine map is applied as s * B + (z - 136 s) * sum x,
// i.e. sum x ((q - 8) s + z) in fp32 (the tile kernel's QM 2 form, fm_gemv.hip).
template <int QM> struct RowT {
    static constexpr int EPL = QM ? 8 : 4;  // elements per lane per chunk
    static constexpr int CE = 64 * EPL;     // k per chunk
    using XV = typename std::conditional<QM != 0, u32x4_t, u32x2_t>::type;  // EPL bf16
    static constexpr int WPL = QM == 2 ? 1 : 2;  // 32-bit words of weights per lane per row per chunk
};

// EPI: 0 STORE (wqkv), 1 FIN (wo / w2), 2 SWIGLU (w1 || w3: rows 4b .. 4b+3 of W1 then of W3 per
// block, outputs y = round(silu(round(g))) * round(u), FeedForward.forward, llama.py:978-986),
// 3 F32 (a head's logits: fp32 holding the T-rounded value).  G: FIN gathers its residual row,
// the other forms their x row (RowGemvArgs::xidx: the fast model's first layer, codebook > 0).
// TX (tagged x, fattn_wo_kernel): x is read after the weights, from 32-bit words (bf16 << 16 | gen)
// that a producer in the same launch stores write-through; the wave re-reads its words (sc1) until
// every tag equals gen (bounded; *err set on timeout).  blk: the row block's index.
// XR 2 (fm_tune fast_pair: bf16, STORE / FIN; fast_pair_q: int8 / int4 codes, SWIGLU too): two activation rows against one
// pass over the weights.  Row 1's operands are RowGemvArgs::X1 / res1 / res_out1 / Y1 (TX: the second K words of xt); G
// gathers row 1's residual only.  One accumulator set, one RMSNorm statistic and one epilogue thread per (x row, weight
// row): every output is the one-row form's operations on the same inputs in the same order.  The code forms load the
// codes, row scales and group (scale, zero) words once for both rows; int8 keeps its 128 * sum(x) and int4 its
// s * B + (z - 136 s) * sum x per x row.
// TxPoll (NG 2 only; speed, never correctness -- every full read checks every tag): delay, 10-ns ticks from the wave's
// start to its first read of x; sleep, the s_sleep argument between reads (1, 4 or 16); cheap, one word per 128
// elements of the wave's range is polled until current before the first full read.
struct TxPoll {
    unsigned delay = 0;
    int sleep = 1, cheap = 0;
};
template <int U, int RP, bool PRENORM, int EPI, bool G, int QM, bool TX, int XR = 1, int NG = 1>
__device__ __forceinline__ void rowgemv_body(const RowGemvArgs& a, const int blk, const uint32_t* xt, const uint32_t gen,
                                             int* err, const TxPoll pw = TxPoll{}) {
    static_assert(!TX || (!PRENORM && EPI == 1), "tagged x: the residual form only");
    static_assert(XR == 1 || (XR == 2 && (EPI == 1 || (QM != 1 && EPI <= (QM ? 2 : 0))) && (!G || EPI == 1)),
                  "two x rows: FIN; bf16 and int4 STORE; int4 SWIGLU");
    constexpr bool FIN = EPI == 1;
    using R = RowT<QM>;
    using XV = typename R::XV;
    constexpr int EPL = R::EPL, NW = EPL / 2;  // NW: 32-bit words of x per lane per chunk
    constexpr int SB = XR * 4 * RP;            // red: [XR][4 waves][RP] partials, then the statistics
    // deep runs (w2): row 1's x chunk is loaded into the registers row 0's chunk leaves, after its dot products, so
    // the two-row form keeps the one-row form's register budget (no scratch under waves_per_eu 5)
    constexpr bool LATE = XR == 2 && QM == 0 && !TX && !PRENORM && U >= 10;
    static_assert(NG == 1 || (NG == 2 && TX), "two row blocks per 512-thread block: the tagged-x form only");
    // NG 2 (slow_attn_wo_kernel): a 512-thread block holds two independent 4-wave groups, each one row block with its
    // own red slice; tid is the thread's index in its group (NG 1: threadIdx.x itself)
    __shared__ float red_s[NG][XR * (4 * RP + 8)];
    const unsigned tid = NG == 1 ? threadIdx.x : threadIdx.x & 255u;
    float(&red)[XR * (4 * RP + 8)] = red_s[NG == 1 ? 0 : threadIdx.x >> 8];
    const int lane = tid & 63, wave = tid >> 6;
    const int n0 = blk * RP;
    const int nch = a.K / R::CE;
    const int wa = (wave * nch) >> 2, nmy = (((wave + 1) * nch) >> 2) - wa;
    const int last = nmy > 0 ? nmy - 1 : 0;
    const unsigned long long ts0 = a.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
    // first round trip, unconditional (a load under a branch drains vmcnt): the epilogue's residual,
    // bias and (int8) scale elements of row n0 + (thread % RP), then x (and the norm weight)
    const int er = n0 + (int)(tid % RP);
    const int ex = XR == 2 ? (int)((tid / RP) & 1) : 0;  // the x row this thread finishes
    int ri = 0, xi = 0;
    if constexpr (G && FIN) {
        const int32_t iv = a.residx[a.res_col];
        ri = iv < 0 ? 0 : (iv >= a.res_rows ? a.res_rows - 1 : iv);
    } else if constexpr (G) {
        const int32_t iv = a.xidx[a.xcol];
        xi = iv < 0 ? 0 : (iv >= a.xrows ? a.xrows - 1 : iv);
    }
    bf16_t rv = 0;
    if constexpr (FIN && XR == 2) rv = ex ? a.res1[(size_t)ri * a.ldr + er] : a.res[er];
    else if constexpr (FIN) rv = a.res[(size_t)ri * a.ldr + er];
    const bf16_t bv = *(a.bias ? a.bias + er : a.X);
    bf16_t sv = 0;
    if constexpr (QM == 1) sv = a.wscale[er];
    const XV* xp = reinterpret_cast<const XV*>(a.X + (size_t)xi * a.ldx) + (size_t)wa * 64 + lane;
    const XV* gp = reinterpret_cast<const XV*>(PRENORM ? a.nw : a.X) + (size_t)wa * 64 + lane;
    XV xv[XR][U], gv[PRENORM ? U : 1];
    if constexpr (!TX) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = (u < last ? u : last) * 64;
            xv[0][u] = xp[j];
            if constexpr (XR == 2 && !LATE) xv[1][u] = (reinterpret_cast<const XV*>(a.X1) + (size_t)wa * 64 + lane)[j];
            if constexpr (PRENORM) gv[u] = gp[j];
        }
    }
    // KV prefetch (STORE form, wqkv of the slow model): slot and position ride the first round trip
    constexpr int PF = 2;
    const bool pf_on = EPI == 0 && a.pf_kc != nullptr;
    int pf_s = 0, pf_p = 0;
    if constexpr (EPI == 0) {
        pf_s = *(pf_on ? a.pf_slot : reinterpret_cast<const int32_t*>(a.X));
        pf_p = *(pf_on ? a.pf_pos : reinterpret_cast<const int32_t*>(a.X));
    }
    asm volatile("" ::: "memory");  // keep the first round trip ahead of the weight loads
    // the block's weights: RP rows of each chunk, 8 B (int4: 4 B) per lane; int4: the lane's group
    // (scale, zero) per row too (tail slots re-load the run's last chunk)
    constexpr int WU = QM == 2 ? 1 : U, WR = QM == 2 ? 1 : RP;
    constexpr int QU = QM == 2 ? U : 1, QR = QM == 2 ? RP : 1;
    u32x2_t wv[WU][WR];
    uint32_t w4[QU][QR], szv[QU][QR];
    if constexpr (QM == 2) {
        const size_t rw = (size_t)(a.K >> 3);  // one row in words
        const int ng = a.K / a.gs;
        const uint32_t* wp = a.Wq4 + (size_t)n0 * rw + (size_t)wa * 64 + lane;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jc = u < last ? u : last;
#pragma unroll
            for (int r = 0; r < RP; ++r) {
                w4[u][r] = __builtin_nontemporal_load(wp + r * rw + jc * 64);
                szv[u][r] = a.wsz[(size_t)(n0 + r) * ng + ((wa + jc) * 512 + lane * 8) / a.gs];
            }
        }
    } else {
        const unsigned char* wb = QM ? reinterpret_cast<const unsigned char*>(a.Wq) : reinterpret_cast<const unsigned char*>(a.W);
        const size_t rowb = (size_t)a.K * (QM ? 1 : 2);  // bytes per row
        const u32x2_t* wp = reinterpret_cast<const u32x2_t*>(wb + (size_t)n0 * rowb) + (size_t)wa * 64 + lane;
        const size_t rs8 = rowb / 8;  // one row in u32x2 units
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = (u < last ? u : last) * 64;
#pragma unroll
            for (int r = 0; r < RP; ++r) wv[u][r] = __builtin_nontemporal_load(wp + r * rs8 + j);
        }
    }
    asm volatile("" ::: "memory");
    unsigned long long tsw = 0, tsx = 0;  // TX developer stamps: weights issued, x words current
    unsigned polls = 0, cpolls = 0;  // full reads of x; NG 2: one-word polls ahead of them (the record's aux: polls | cpolls << 16)
    if constexpr (TX) {
        if (a.dbg) tsw = __builtin_amdgcn_s_memrealtime();
        // EPL tagged words per lane per chunk (sc1 loads, 16 B each), re-read until all are current
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)xt, (short)0, XR * a.K * 4, 0x00020000);
        u32x4_t xw[XR][U][EPL / 4];
        auto nap = [&] {
            if constexpr (NG == 2) {
                if (pw.sleep >= 16) __builtin_amdgcn_s_sleep(16);
                else if (pw.sleep >= 4) __builtin_amdgcn_s_sleep(4);
                else __builtin_amdgcn_s_sleep(1);
            } else {
                __builtin_amdgcn_s_sleep(1);
            }
        };
        if constexpr (NG == 2) {
            // the producer runs for microseconds: no read of x before pw.delay (time-bounded), then one word per 128
            // elements until those are current (bounded; the full reads below decide and report a timeout)
            const unsigned long long tw0 = __builtin_amdgcn_s_memrealtime();
            while (pw.delay && (unsigned)(__builtin_amdgcn_s_memrealtime() - tw0) < pw.delay) __builtin_amdgcn_s_sleep(8);
            if (pw.cheap) {
                const int ng = nmy * (R::CE / 128);
                const int wi = (wa * R::CE + 128 * (lane < ng ? lane : 0) + 127) * 4;
                for (unsigned it = 0; it < (1u << 14); ++it) {
                    cpolls = it + 1;
                    const uint32_t w = __builtin_amdgcn_raw_buffer_load_b32(xr, wi, 0, 16);
                    if (__all((w & 0xffffu) == gen)) break;
                    nap();
                }
            }
        }
        for (unsigned it = 0;; ++it) {
            polls = it + 1;
#pragma unroll
            for (int x = 0; x < XR; ++x)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int jc = u < last ? u : last;
#pragma unroll
                    for (int q = 0; q < EPL / 4; ++q)
                        xw[x][u][q] = __builtin_amdgcn_raw_buffer_load_b128(
                            xr, (x * a.K + (wa + jc) * R::CE + EPL * lane + 4 * q) * 4, 0, 16);
                }
            bool ok = true;
#pragma unroll
            for (int x = 0; x < XR; ++x)
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int q = 0; q < EPL / 4; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) ok = ok && ((xw[x][u][q][e] & 0xffffu) == gen);
            if (__all(ok)) break;
            if (it >= (1u << 14)) {  // bounded: the host sees err and fails the frame
                if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            nap();
        }
        if (a.dbg) tsx = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int x = 0; x < XR; ++x)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < NW; ++h) {
                    const uint32_t w0 = xw[x][u][(2 * h) >> 2][(2 * h) & 3], w1 = xw[x][u][(2 * h + 1) >> 2][(2 * h + 1) & 3];
                    xv[x][u][h] = (w0 >> 16) | (w1 & 0xffff0000u);
                }
    }
    float pfw[PF];
    if constexpr (EPI == 0) {  // GemvArgs::pf_kc: one 4-byte load per 64-B sector, after the weights
        // byte offsets from the K cache (integer selects only: a per-lane pointer select or a
        // load under a branch makes the compiler drain vmcnt)
        const char* kcb = reinterpret_cast<const char*>(pf_on ? a.pf_kc : a.X);
        const long long dv = pf_on ? reinterpret_cast<const char*>(a.pf_vc) - kcb : 0;
        const int nkv = pf_on ? a.pf_nkv : 1;
        const int b = blockIdx.x, h = b % nkv, jb = b / nkv, nb = ((int)gridDim.x - 1 - h) / nkv + 1;
        const int spr = pf_on ? a.pf_hd * 2 / 64 : 1;
        const int np = pf_on ? pf_p + 1 : 0, total = 2 * np * spr;
        const long long base = pf_on ? (long long)pf_s * (long long)a.pf_slot_stride + (long long)a.pf_layer_off +
                                           (long long)h * a.pf_S * a.pf_hd
                                     : 0;
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const int i = (jb + nb * q) * 256 + (int)threadIdx.x;
            const bool ok = i < total;
            const int ii = ok ? i : 0, row = ii / spr, sec = ii - row * spr;
            const bool isv = row >= np;
            const long long off = (isv ? dv : 0) + 2 * (base + (long long)(isv ? row - np : row) * a.pf_hd) + sec * 64;
            pfw[q] = *reinterpret_cast<const float*>(kcb + (ok ? off : 0));
        }
    }
    // PRENORM: the row statistic (every block the same sums in the same order), then x'
    if constexpr (PRENORM && XR == 1) {  // (kept apart from the two-row form below: the one-row code stays as it compiled)
        float sl = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < nmy) {
#pragma unroll
                for (int h = 0; h < NW; ++h) {
                    const float e0 = lo16(xv[0][u][h]), e1 = hi16(xv[0][u][h]);
                    sl += e0 * e0 + e1 * e1;
                }
            }
        }
        sl = wave_sum(sl);
        if (lane == 0) red[4 * RP + wave] = sl;
        lds_barrier();
        const float tot = ((red[4 * RP] + red[4 * RP + 1]) + red[4 * RP + 2]) + red[4 * RP + 3];
        const float rs = 1.0f / sqrtf(tot / (float)a.K + a.eps);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            XV o;
#pragma unroll
            for (int h = 0; h < NW; ++h) {
                const float y0 = bfround(bfround(lo16(xv[0][u][h]) * rs) * lo16(gv[u][h]));
                const float y1 = bfround(bfround(hi16(xv[0][u][h]) * rs) * hi16(gv[u][h]));
                o[h] = (uint32_t)f2bf(y0) | ((uint32_t)f2bf(y1) << 16);
            }
            xv[0][u] = o;
        }
    }
    if constexpr (PRENORM && XR == 2) {  // one statistic per x row, each the one-row form's sums in its order
#pragma unroll
        for (int x = 0; x < XR; ++x) {
            float sl = 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < nmy) {
#pragma unroll
                    for (int h = 0; h < NW; ++h) {
                        const float e0 = lo16(xv[x][u][h]), e1 = hi16(xv[x][u][h]);
                        sl += e0 * e0 + e1 * e1;
                    }
                }
            }
            sl = wave_sum(sl);
            if (lane == 0) red[SB + 4 * x + wave] = sl;
        }
        lds_barrier();
#pragma unroll
        for (int x = 0; x < XR; ++x) {
            const float tot = ((red[SB + 4 * x] + red[SB + 4 * x + 1]) + red[SB + 4 * x + 2]) + red[SB + 4 * x + 3];
            const float rs = 1.0f / sqrtf(tot / (float)a.K + a.eps);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                XV o;
#pragma unroll
                for (int h = 0; h < NW; ++h) {
                    const float y0 = bfround(bfround(lo16(xv[x][u][h]) * rs) * lo16(gv[u][h]));
                    const float y1 = bfround(bfround(hi16(xv[x][u][h]) * rs) * hi16(gv[u][h]));
                    o[h] = (uint32_t)f2bf(y0) | ((uint32_t)f2bf(y1) << 16);
                }
                xv[x][u] = o;
            }
        }
    }
    float acc[XR][RP];
#pragma unroll
    for (int x = 0; x < XR; ++x)
#pragma unroll
        for (int r = 0; r < RP; ++r) acc[x][r] = 0.f;
    float xs[XR];  // int8: this lane's sum of each x row (the 128 offset of the codes)
#pragma unroll
    for (int x = 0; x < XR; ++x) xs[x] = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (u < nmy) {
            if constexpr (QM == 0) {
#pragma unroll
                for (int r = 0; r < RP; ++r)
#pragma unroll
                    for (int x = 0; x < (LATE ? 1 : XR); ++x) acc[x][r] = dot4(wv[u][r], xv[x][u], acc[x][r]);
            } else if constexpr (QM == 2) {
                const u32x4_t ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
                const float xl = dot8r(ones, xv[0][u], 0.f);  // sum of the lane's 8 x
                float xl1 = 0.f;
                if constexpr (XR == 2) xl1 = dot8r(ones, xv[1][u], 0.f);
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    const uint32_t w = w4[u][r];
                    u32x4_t A;
#pragma unroll
                    for (int p = 0; p < 4; ++p) A[p] = ((w >> (4 * p)) & 0x000F000Fu) | 0x43004300u;
                    const float B = dot8r(A, xv[0][u], 0.f);
                    const float sc = lo16(szv[u][r]), zr = hi16(szv[u][r]);
                    acc[0][r] = fmaf(sc, B, acc[0][r]);
                    acc[0][r] = fmaf(zr - 136.f * sc, xl, acc[0][r]);
                    if constexpr (XR == 2) {  // (the word unpacked once for both rows)
                        const float B1 = dot8r(A, xv[1][u], 0.f);
                        acc[1][r] = fmaf(sc, B1, acc[1][r]);
                        acc[1][r] = fmaf(zr - 136.f * sc, xl1, acc[1][r]);
                    }
                }
            } else {
                float xf[XR][8];
#pragma unroll
                for (int x = 0; x < XR; ++x) {
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        xf[x][2 * h] = lo16(xv[x][u][h]);
                        xf[x][2 * h + 1] = hi16(xv[x][u][h]);
                    }
                    xs[x] += ((xf[x][0] + xf[x][1]) + (xf[x][2] + xf[x][3])) + ((xf[x][4] + xf[x][5]) + (xf[x][6] + xf[x][7]));
                }
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    const uint32_t c0 = wv[u][r][0] ^ 0x80808080u, c1 = wv[u][r][1] ^ 0x80808080u;
#pragma unroll
                    for (int x = 0; x < XR; ++x) {  // (the codes converted once for both rows)
                        float t = acc[x][r];
#pragma unroll
                        for (int e = 0; e < 4; ++e) t = fmaf((float)((c0 >> (8 * e)) & 0xffu), xf[x][e], t);
#pragma unroll
                        for (int e = 0; e < 4; ++e) t = fmaf((float)((c1 >> (8 * e)) & 0xffu), xf[x][4 + e], t);
                        acc[x][r] = t;
                    }
                }
            }
        }
    }
    if constexpr (LATE) {
        // row 1's loads stay behind row 0's dot products (the accumulators pass through the statement)
#pragma unroll
        for (int r = 0; r < RP; ++r) asm volatile("" : "+v"(acc[0][r])::"memory");
        const XV* xp1 = reinterpret_cast<const XV*>(a.X1) + (size_t)wa * 64 + lane;
#pragma unroll
        for (int u = 0; u < U; ++u) xv[1][u] = xp1[(u < last ? u : last) * 64];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < nmy) {
#pragma unroll
                for (int r = 0; r < RP; ++r) acc[1][r] = dot4(wv[u][r], xv[1][u], acc[1][r]);
            }
        }
    }
    if constexpr (EPI == 0) {  // keep the prefetch loads (retired with the weights)
#pragma unroll
        for (int q = 0; q < PF; ++q) asm volatile("" ::"v"(pfw[q]));
    }
    const unsigned long long ts1 = a.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
#pragma unroll
    for (int x = 0; x < XR; ++x)
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            const float v = wave_sum(acc[x][r]);
            if (lane == 0) red[(4 * x + wave) * RP + r] = v;
        }
    // int8: the four waves' sums of x, per x row (XR 1: behind the partials and the statistic; XR 2: behind both rows' of each)
    constexpr int XSB = XR == 2 ? SB + 8 : 4 * RP + 4;
    if constexpr (QM == 1) {
#pragma unroll
        for (int x = 0; x < XR; ++x) {
            const float v = wave_sum(xs[x]);
            if (lane == 0) red[XSB + 4 * x + wave] = v;
        }
    }
    __syncthreads();
    if ((int)tid < XR * RP) {
        const int t = XR == 2 ? (int)(tid % RP) : (int)tid;
        const float* rd = red + 4 * RP * ex;
        float v = ((rd[t] + rd[RP + t]) + rd[2 * RP + t]) + rd[3 * RP + t];
        if constexpr (QM == 1) {
            const float* rx = red + XSB + 4 * ex;
            const float xt = ((rx[0] + rx[1]) + rx[2]) + rx[3];
            v = bfround(bfround(v - 128.f * xt) * bf2f(sv));
        }
        if (a.bias) v += bf2f(bv);
        if constexpr (FIN) {
            (ex ? a.res_out1 : a.res_out)[er] = f2bf(bfround(bf2f(rv) + bfround(v)));
        } else if constexpr (EPI == 3) {
            a.Yf[er] = bfround(v);
        } else if constexpr (EPI == 2) {  // gate rows t < RP / 2, up rows t >= RP / 2 (same wave)
            const float up = __shfl_down(v, RP / 2, 64);  // (XR 2: lanes ex RP + t, the partner in the same x row's group)
            if (t < RP / 2) {
                const float g = bfround(v);
                (ex ? a.Y1 : a.Y)[blockIdx.x * (RP / 2) + t] = f2bf(bfround(g / (1.0f + expf(-g))) * bfround(up));
            }
        } else if constexpr (XR == 2) {  // (row 0's outputs below skip0 are not wanted: a block straddling it)
            if (ex || er >= a.skip0) (ex ? a.Y1 : a.Y)[er] = f2bf(v);
        } else {
            a.Y[er] = f2bf(v);
        }
    }
    if (a.dbg && tid == 0) {  // one record per x row: a record stands for one block's work on one row
#pragma unroll
        for (int x = 0; x < XR; ++x) {
            if constexpr (TX) {  // (wave 0) start, weights issued, x words current, dot products done, end; aux = reads of x
                const unsigned long long t[7] = {ts0, tsw, tsx, ts1, __builtin_amdgcn_s_memrealtime(), 0, 0};
                dbg_record(a.dbg, 0xFFF8u, polls | (cpolls << 16), t);
                // NG 2, the slow wo: a row-block record (0xFFFA) per row pair as well, so that the count of row-block
                // records in a frame stays what the wo launch it replaces left (tests/test_gpu_rowgemv.py counts them).
                // They are not rowgemv_kernel blocks: their span {start, dot products done, end} holds the wait for the
                // attention, and a probe that times 0xFFFA records (scripts/ts_probe.py) reads that wait as stream time;
                // aux bit 31 marks them
                if constexpr (NG == 2) {
                    const unsigned long long tr[7] = {ts0, ts1, t[4], 0, 0, 0, 0};
#pragma unroll
                    for (int p = 0; p < RP / 2; ++p) dbg_record(a.dbg, 0xFFFAu, 0x80000000u | (unsigned)(blk * (RP / 2) + p), tr);
                }
            } else {
                const unsigned long long t[7] = {ts0, ts1, __builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0};
                dbg_record(a.dbg, 0xFFFAu, (unsigned)blk, t);
            }
        }
    }
}

template <int U, int RP, bool PRENORM, int EPI, bool G, int QM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RP == 2 ? 5 : 3)))
void rowgemv_kernel(RowGemvArgs a) {
    rowgemv_body<U, RP, PRENORM, EPI, G, QM, false>(a, blockIdx.x, nullptr, 0u, nullptr);
}

// Two activation rows (fm_tune fast_pair): the same grid, each block's weights loaded once for both rows.
// STORE (wqkv): a block whose rows all lie in [0, skip0) -- the Q rows, which row 0 never reads -- runs the
// one-row body on row 1.
template <int U, int RP, bool PRENORM, int EPI, bool G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RP == 2 ? 5 : 3)))
void rowgemv2_kernel(RowGemvArgs a) {
    if constexpr (EPI == 0) {
        if (((int)blockIdx.x + 1) * RP <= a.skip0) {
            RowGemvArgs b = a;
            b.X = a.X1;
            b.Y = a.Y1;
            rowgemv_body<U, RP, PRENORM, EPI, false, 0, false>(b, blockIdx.x, nullptr, 0u, nullptr);
            return;
        }
    }
    rowgemv_body<U, RP, PRENORM, EPI, G, 0, false, 2>(a, blockIdx.x, nullptr, 0u, nullptr);
}

// ... on int8 (QM 1) / int4 (QM 2) codes (fm_tune fast_pair_q): FIN, NORM_STORE and NORM_SWIGLU (EPI 2: no row is
// skipped, both rows want every output).  The bf16 kernel above keeps its name and its code.
template <int U, int RP, bool PRENORM, int EPI, bool G, int QM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RP == 2 ? 5 : 3)))
void rowgemv2q_kernel(RowGemvArgs a) {
    static_assert(QM == 1 || QM == 2, "the code forms");
    if constexpr (EPI == 0) {
        if (((int)blockIdx.x + 1) * RP <= a.skip0) {
            RowGemvArgs b = a;
            b.X = a.X1;
            b.Y = a.Y1;
            rowgemv_body<U, RP, PRENORM, EPI, false, QM, false>(b, blockIdx.x, nullptr, 0u, nullptr);
            return;
        }
    }
    rowgemv_body<U, RP, PRENORM, EPI, G, QM, false, 2>(a, blockIdx.x, nullptr, 0u, nullptr);
}

// smallest instantiated depth covering a wave's share of the K chunks (0: not eligible)
int rowgemv_u(int K, int qm) {
    const int ce = qm ? 512 : 256;
    if (K <= 0 || K % ce) return 0;
    const int need = (K / ce + 3) / 4;
    for (int u : {2, 3, 4, 5, 6, 8, 10, 12})
        if (need <= u) return u;
    return 0;
}

template <int RP, bool PRENORM, int EPI, int QM>
static void rowgemv_go(hipStream_t s, const RowGemvArgs& a, int U) {
    const dim3 grid(a.N / RP), block(256);
    auto go = [&](void (*plain)(RowGemvArgs), void (*gathered)(RowGemvArgs)) {
        ((EPI == 1 ? a.residx != nullptr : a.xidx != nullptr) ? gathered : plain)<<<grid, block, 0, s>>>(a);
    };
#define RG(u) go(rowgemv_kernel<u, RP, PRENORM, EPI, false, QM>, rowgemv_kernel<u, RP, PRENORM, EPI, true, QM>)
    switch (U) {
        case 2: RG(2); break;
        case 3: RG(3); break;
        case 4: RG(4); break;
        case 5: RG(5); break;
        case 6: RG(6); break;
        case 8: RG(8); break;
        case 10: RG(10); break;
        default: RG(12); break;
    }
#undef RG
}

// the two-row forms: FIN (wo / w2, RP 2, row 1's residual gathered or not) and NORM_STORE (wqkv, row_qkv_rp rows)
template <int RP, bool PRENORM, int EPI>
static void rowgemv2_go(hipStream_t s, const RowGemvArgs& a, int U) {
    const dim3 grid(a.N / RP), block(256);
    const bool g = EPI == 1 && a.residx != nullptr;
#define RG(u) \
    case u: (g ? rowgemv2_kernel<u, RP, PRENORM, EPI, EPI == 1> : rowgemv2_kernel<u, RP, PRENORM, EPI, false>)<<<grid, block, 0, s>>>(a); break;
    switch (U) {
        RG(2) RG(3) RG(4) RG(5)
        default:
            if constexpr (EPI == 1) {
                if (U == 6) rowgemv2_kernel<6, RP, PRENORM, EPI, false><<<grid, block, 0, s>>>(a);
                else if (U == 8) rowgemv2_kernel<8, RP, PRENORM, EPI, false><<<grid, block, 0, s>>>(a);
                else if (U == 10) rowgemv2_kernel<10, RP, PRENORM, EPI, false><<<grid, block, 0, s>>>(a);
                else rowgemv2_kernel<12, RP, PRENORM, EPI, false><<<grid, block, 0, s>>>(a);
            }
            break;
    }
#undef RG
}

// The two-row forms that exist: every one of them fits its launch bounds without scratch (code-object metadata,
// DESIGN section 3 round 9); a shape outside them runs the one-row passes.  NORM_STORE: 8 rows per block, runs
// of at most 5 chunks; FIN: any depth, the gathered form (the first layer's wo, K = nq) at most 5; the fused
// attention + wo pair form (kind -1): at most 5, within its 80 registers.
// qm 1 / 2 (fm_tune fast_pair_q; chunks of 512 k): FIN on int8 and int4 codes at runs of at most 5 chunks (K <= 10240:
// S2-Pro's w2 at 9728 is depth 5); NORM_STORE and NORM_SWIGLU on int4 codes (8 rows per block) at most 3 (K <= 6144;
// 4 and 5 spill under their launch bounds); the fused pair form at depths 2 and, int4 only, 3 -- the ones that hold its
// 80 registers without scratch (int8 depth 3 spills 28 B per lane).
bool rowgemv_pair_ok(int kind, int K, bool gathered, int qm) {
    const int U = rowgemv_u(K, qm);
    if (U <= 0) return false;
    if (qm) {
        if (kind == ROWGEMV_FIN) return U <= 5;
        if (kind == ROWGEMV_NORM_STORE || kind == ROWGEMV_NORM_SWIGLU) return qm == 2 && U <= 3;
        return kind == -1 && U <= (qm == 2 ? 3 : 2);
    }
    if (kind == ROWGEMV_FIN) return U <= 5 || !gathered;
    if (kind == ROWGEMV_NORM_STORE) return U <= 5 && fm_tuning().row_qkv_rp == 8;
    return kind == -1 && U <= 5;
}

// the two-row code forms (rowgemv_pair_ok's depths: FIN 2 .. 5, the norm kinds 2 .. 3)
template <int RP, bool PRENORM, int EPI, int QM>
static void rowgemv2q_go(hipStream_t s, const RowGemvArgs& a, int U) {
    const dim3 grid(a.N / RP), block(256);
    const bool g = EPI == 1 && a.residx != nullptr;
#define RG(u) (g ? rowgemv2q_kernel<u, RP, PRENORM, EPI, EPI == 1, QM> : rowgemv2q_kernel<u, RP, PRENORM, EPI, false, QM>)<<<grid, block, 0, s>>>(a)
    if (U == 2) RG(2);
    else if (U == 3) RG(3);
    else if constexpr (EPI == 1) {
        if (U == 4) RG(4);
        else if (U == 5) RG(5);
        else FMCHECK(false, "row GEMV, two rows on codes: fin has depths 2 .. 5");
    } else {
        FMCHECK(false, "row GEMV, two rows on codes: the norm kinds have depths 2 .. 3");
    }
#undef RG
}

static void launch_rowgemv2q(hipStream_t s, const RowGemvArgs& a, int kind, int U, int qm) {
    FMCHECK(!a.W && !a.xidx && !a.bias && rowgemv_pair_ok(kind, a.K, a.residx != nullptr, qm),
            "row GEMV, two rows on codes: int8 fin (depths 2 .. 5), int4 fin (2 .. 5) / norm + store / norm + swiglu (2 .. 3), no x gather, no bias");
    if (kind == ROWGEMV_FIN) {
        FMCHECK(a.N % 2 == 0 && a.X1 && a.res && a.res1 && a.res_out && a.res_out1,
                "row GEMV (fin, two rows on codes): N even, both x and residual rows set");
        if (qm == 2) rowgemv2q_go<2, false, 1, 2>(s, a, U);
        else rowgemv2q_go<2, false, 1, 1>(s, a, U);
    } else if (kind == ROWGEMV_NORM_STORE) {
        FMCHECK(a.N % 8 == 0 && a.nw && a.X1 && a.Y && a.Y1 && a.skip0 >= 0,
                "row GEMV (norm, store, two rows on int4 codes): N a whole number of 8-row blocks, norm weight, both rows set");
        rowgemv2q_go<8, true, 0, 2>(s, a, U);
    } else {
        FMCHECK(a.N % 8 == 0 && a.nw && a.X1 && a.Y && a.Y1,
                "row GEMV (norm, swiglu, two rows on int4 codes): N a whole number of 4 + 4-row blocks, norm weight, both rows set");
        rowgemv2q_go<8, true, 2, 2>(s, a, U);
    }
}

static void launch_rowgemv2(hipStream_t s, const RowGemvArgs& a, int kind, int U) {
    if (a.Wq || a.Wq4) {
        launch_rowgemv2q(s, a, kind, U, a.Wq4 ? 2 : 1);
        return;
    }
    FMCHECK(a.W && !a.Wq && !a.Wq4 && !a.xidx, "row GEMV, two rows: bf16, no x gather");
    if (kind == ROWGEMV_FIN) {
        FMCHECK(a.N % 2 == 0 && a.res && a.res1 && a.res_out && a.res_out1 && rowgemv_pair_ok(kind, a.K, a.residx != nullptr),
                "row GEMV (fin, two rows): N even, both residual rows set, an instantiated depth");
        rowgemv2_go<2, false, 1>(s, a, U);
    } else {
        FMCHECK(kind == ROWGEMV_NORM_STORE && a.N % 8 == 0 && a.nw && a.X1 && a.Y && a.Y1 && a.skip0 >= 0 &&
                    rowgemv_pair_ok(kind, a.K, false),
                "row GEMV (norm, store, two rows): N a whole number of 8-row blocks, norm weight, both rows set, an instantiated depth");
        rowgemv2_go<8, true, 0>(s, a, U);
    }
}

void launch_rowgemv(hipStream_t s, const RowGemvArgs& a0, int kind) {
    RowGemvArgs a = a0;
    a.dbg = fm_tuning().dbg;
    if (!a.ldx) a.ldx = a.K;
    const int qm = a.Wq4 ? 2 : (a.Wq ? 1 : 0);
    const int U = rowgemv_u(a.K, qm);
    FMCHECK(U > 0 && a.X &&
                (qm == 2 ? (a.wsz && a.gs > 0 && a.gs % 8 == 0 && a.K % a.gs == 0 && !a.bias)
                         : (qm == 1 ? (a.Wq && a.wscale && !a.bias) : a.W != nullptr)),
            "row GEMV: K a whole number of chunks (256 k, int8 / int4 512 k), at most 48 per wave; operands set");
    if (a.xr == 2) {
        launch_rowgemv2(s, a, kind, U);
        return;
    }
    if (kind == ROWGEMV_FIN) {
        FMCHECK(a.N % 2 == 0 && a.res && a.res_out, "row GEMV (fin): N even, residual rows set");
        if (qm == 2) rowgemv_go<2, false, 1, 2>(s, a, U);
        else if (qm == 1) rowgemv_go<2, false, 1, 1>(s, a, U);
        else rowgemv_go<2, false, 1, 0>(s, a, U);
    } else if (kind == ROWGEMV_NORM_F32) {
        FMCHECK(a.N % 8 == 0 && a.nw && a.Yf && U <= 8 && !a.xidx, "row GEMV (norm, f32): N % 8 == 0, norm weight and output set");
        if (qm == 2) rowgemv_go<8, true, 3, 2>(s, a, U);
        else if (qm == 1) rowgemv_go<8, true, 3, 1>(s, a, U);
        else rowgemv_go<8, true, 3, 0>(s, a, U);
    } else if (kind == ROWGEMV_NORM_SWIGLU) {
        FMCHECK(a.N % 8 == 0 && a.nw && a.Y && U <= 8 && !a.bias,
                "row GEMV (norm, swiglu): N % 8 == 0 (4 + 4 interleaved rows), norm weight and output set");
        if (qm == 2) rowgemv_go<8, true, 2, 2>(s, a, U);
        else if (qm == 1) rowgemv_go<8, true, 2, 1>(s, a, U);
        else rowgemv_go<8, true, 2, 0>(s, a, U);
    } else {
        FMCHECK(kind == ROWGEMV_NORM_STORE && a.N % 8 == 0 && a.nw && a.Y && U <= 8,
                "row GEMV (norm, store): N % 8 == 0, norm weight and output set");
        if (qm == 2) rowgemv_go<8, true, 0, 2>(s, a, U);
        else if (qm == 1) rowgemv_go<8, true, 0, 1>(s, a, U);
        else if (fm_tuning().row_qkv_rp == 4) rowgemv_go<4, true, 0, 0>(s, a, U);
        else if (fm_tuning().row_qkv_rp == 16) rowgemv_go<16, true, 0, 0>(s, a, U);
        else rowgemv_go<8, true, 0, 0>(s, a, U);
    }
}

// =========================================================================================
// Fast-model attention + wo in ONE launch (batch 1, bf16; fm_tune fattn_wo).
//
// The fast model's attention (llama.py:947-975, one query row at codebook position cpos < 16) is
// latency-bound: ~4 us of dependent round trips on 32 of 256 CUs, while the wo GEMV that consumes
// it is a 21 MB weight stream.  Here blocks 0 .. nkv-1 run the attention (one block per kv group,
// one wave per q head, cached K / V rows staged in LDS) and blocks nkv .. nkv + N/2 - 1 are the
// row-pair wo blocks of rowgemv_kernel, which issue their whole weight run first and only then
// wait for the attention output.  The hand-off has no counters and no fences: each attention
// output element is stored write-through (sc1) as one 32-bit word (bf16 value << 16 | gen), gen a
// tag unique among consecutive launches (host: 1 + layer + n_layer * cpos), and a wo wave re-reads
// its x words (sc1 loads) until every tag is current.  Deadlock-free by dispatch order: the
// attention blocks have the lowest indices, so they are resident before any waiting block, and the
// whole grid fits at once (<= 8 blocks of 4 waves per CU, 10 KiB LDS each).  Every wait is bounded
// (FattnWoArgs::err set on timeout; the host throws and resets).
constexpr int FW_MAXJ = 15;   // cached rows staged in LDS (cpos < 16)
constexpr int FW_MAXHD = 128;

// score -> softmax -> PV of one q head over positions 0 .. cpos, cpos < NJ <= FW_MAXJ + 1 (fm_tune
// fattn_ilp).  NJ is a compile-time count, so the whole body is one basic block: every LDS read of a
// phase is issued before its first use, and the NJ wave_sum chains are independent instructions the
// scheduler interleaves.  Per position the arithmetic is that of the early-exit loops
// in fattn_wo_kernel, in the same order (max, then den and the PV sums in ascending j); a position
// j > cpos (NJ rounded up) has score -inf, weight exactly 0 and a zeroed V row, and adding its +0
// changes neither den (> 0) nor an accumulator (never -0: it starts from +0), so the bits are the same.
// Rows j >= cpos of the staged K / V hold no data; they are read (inside the array) and selected away.
// Only the lane's first RoPE pair (x0, x1 = element [0] of the loops' pairs) takes part: hd <= FW_MAXHD
// = 128, so the second pair (lane + 64 >= hd / 2) is masked to zero in every operand, its products
// add +-0 to a partial sum that is never -0, and its output is not stored.
template <int NJ>
__device__ __forceinline__ void fw_attend(const bf16_t* Ks, const bf16_t* Vs, const int hd, const int half, const int cpos,
                                          const int lane, const float scale, const float q0, const float q1, const float k0,
                                          const float k1, const float v0, const float v1, float& o0, float& o1) {
    static_assert(NJ >= 1 && NJ <= FW_MAXJ + 1 && FW_MAXHD <= 128, "positions 0 .. FW_MAXJ, one pair per lane");
    constexpr int NC = NJ < FW_MAXJ ? NJ : FW_MAXJ;  // staged rows that can be live (j < cpos <= NJ - 1)
    const bool in = lane < half;
    const int pp = in ? lane : 0;
    uint32_t kw[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) kw[j] = *reinterpret_cast<const uint32_t*>(Ks + j * hd + 2 * pp);
    float sc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const uint32_t w = kw[j < NC ? j : 0];
        const bool cached = j < NC && j < cpos;  // (else the new k: position cpos, or a masked one)
        const float a0 = cached ? (in ? lo16(w) : 0.f) : k0;
        const float a1 = cached ? (in ? hi16(w) : 0.f) : k1;
        float d = 0.f;
        d += q0 * a0 + q1 * a1;
        sc[j] = d;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) sc[j] = wave_sum(sc[j]);
    uint32_t vw[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) vw[j] = *reinterpret_cast<const uint32_t*>(Vs + j * hd + 2 * pp);
    // The NJ sums are wave-uniform: lane j takes position j's, so the two roundings of the score, expf and the
    // division run once for all positions (one per lane, lanes 0 .. NJ - 1 of the first 16-lane row) instead of
    // once per position in every lane; den is still summed in ascending j, from the lanes' values
    float s = -INFINITY;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s = lane == j ? sc[j] : s;
    s = lane <= cpos ? bfround(bfround(s) * scale) : -INFINITY;
    const float mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row_max16(s)), 0));  // (max: any order)
    const float e = lane <= cpos ? expf(s - mx) : 0.f;
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) den += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), j));
    const float p = bfround(e / den);  // lane j: position j's probability (0 past cpos)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float pj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), j));
        const uint32_t w = vw[j < NC ? j : 0];
        const bool cached = j < NC && j < cpos;
        o0 += pj * (cached ? lo16(w) : (j == cpos ? v0 : 0.f));
        o1 += pj * (cached ? hi16(w) : (j == cpos ? v1 : 0.f));
    }
}

//
// M (the attention half is bf16 whatever QM the wo half streams; forms 1 and 2 on int8 / int4 weights: fm_tune
// fast_dead_q): 0 the attention reads the raw q|k|v row the QKV launch left in at.qkv.
// 1 (fm_tune rowgemv bit 5, the first layer at codebook > 0): that row is a pure function of the
//   sampled code -- round(Wqkv rmsnorm(fast_embeddings[code]) + b) -- so it is read from the table
//   of all codebook_size rows built at load time (A.qtab) and no QKV launch runs.  The index goes
//   out first; the table-row loads wait on it.
// In forms 0 and 1 the cached K / V rows go out ahead of the q|k|v row loads, two 16-B chunks per
// thread into registers, unconditionally (a load under a branch drains vmcnt; a copy loop with a
// runtime trip count, and a knob that selects one behind a branch, both measured slower).
// 2 (bit 6, codebook 0): one position, so softmax = {1} and the output is 0 + 1 * v: no Q loads,
//   no q prep, no score (the projection computed the K / V rows only).  The 0.f + stays: it is what
//   turns a -0 of v into the +0 the full form stores.
template <int U, bool G, int QM, int M>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
void fattn_wo_kernel(FattnWoArgs A) {
    static_assert(2 * FW_MAXJ * FW_MAXHD / 8 <= 512, "cached rows: at most two 16-B chunks per thread");
    __shared__ __attribute__((aligned(16))) bf16_t kvs[2 * FW_MAXJ * FW_MAXHD];
    __shared__ float red[8];
    const FastFusedArgs<bf16_t>& at = A.at;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the tag: the frame's position (device, constant through the frame's fast passes) times 41
    // plus the launch's index in the frame (1 .. 40): distinct for any two launches less than ~1600
    // frames apart, across requests and slots too, so a stale word never passes for a fresh one
    const uint32_t gen = ((uint32_t)A.at.row_pos[0] * 41u + (uint32_t)A.gen) % 65535u + 1u;
    const unsigned long long ts0 = A.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
    if ((int)blockIdx.x < at.nkv) {
        // ---------------- attention: kv group kvh, q head kvh * g + wave ----------------------
        // top issue priority: the wo waves sharing this CU queue their whole weight run at once
        if (A.prio) __builtin_amdgcn_s_setprio(3);
        const int kvh = blockIdx.x, hd = at.hd, g = at.nh / at.nkv, cpos = at.cpos, half = hd >> 1;
        const bf16_t* qkv = at.qkv;
        if constexpr (M == 1) {  // the table row of the sampled code (rowgemv_body's xi clamp)
            const int32_t iv = A.qidx[A.qcol];
            const int xi = iv < 0 ? 0 : (iv >= A.qrows ? A.qrows - 1 : iv);
            qkv = A.qtab + (size_t)xi * at.ldqkv;
        }
        const int slot = at.row_slot[0];
        const bool live = wave < g;
        const int h = kvh * g + (live ? wave : 0);
        const float* tab = at.rope + (size_t)cpos * hd;
        const size_t base = (size_t)slot * at.slot_stride + at.layer_off + (size_t)kvh * at.S * hd;
        const int nck = cpos * hd / 8;
        // the cached rows j < cpos of this kv head -> LDS (K rows, then V rows), 16 B per thread
        auto kv_src = [&](int i) {  // chunk i of the 2 * nck (past them: chunk 0, loaded and dropped)
            const bool ok = i < 2 * nck, isv = ok && i >= nck;
            const int c = ok ? (isv ? i - nck : i) : 0;
            return reinterpret_cast<const u32x4_t*>((isv ? at.vc : at.kc) + base + (size_t)c * 8);
        };
        auto kv_dst = [&](int i) {
            const bool isv = i >= nck;
            return reinterpret_cast<u32x4_t*>(kvs + (isv ? FW_MAXJ * FW_MAXHD : 0) + (isv ? i - nck : i) * 8);
        };
        u32x4_t kvr[2];
        if constexpr (M != 2) {  // in registers, ahead of the q|k|v row loads (no branch: nothing drains)
#pragma unroll
            for (int q = 0; q < 2; ++q) kvr[q] = *kv_src((int)threadIdx.x + 256 * q);
        }
        float q0[2], q1[2], k0[2], k1[2], v0[2], v1[2], qw0[2], qw1[2], kw0[2], kw1[2], c_[2], s_[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int p = lane + 64 * u;
            const int pp = p < half ? p : 0;
            if constexpr (M == 2) q0[u] = q1[u] = 0.f;
            else ld_pair_bf(qkv + (size_t)h * hd + 2 * pp, q0[u], q1[u]);
            ld_pair_bf(qkv + (size_t)(at.nh + kvh) * hd + 2 * pp, k0[u], k1[u]);
            ld_pair_bf(qkv + (size_t)(at.nh + at.nkv + kvh) * hd + 2 * pp, v0[u], v1[u]);
            if (at.qk_norm) {
                if constexpr (M != 2) ld_pair_bf(at.qn + 2 * pp, qw0[u], qw1[u]);
                ld_pair_bf(at.kn + 2 * pp, kw0[u], kw1[u]);
            } else {
                qw0[u] = qw1[u] = kw0[u] = kw1[u] = 1.f;
            }
            c_[u] = tab[2 * pp];
            s_[u] = tab[2 * pp + 1];
            if (p >= half) q0[u] = q1[u] = k0[u] = k1[u] = v0[u] = v1[u] = 0.f;
        }
        if constexpr (M != 2) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if ((int)threadIdx.x + 256 * q < 2 * nck) *kv_dst((int)threadIdx.x + 256 * q) = kvr[q];
        }
        // qk-norm (fp32 incl. weight, one rounding) + RoPE (bf16 table, rounded): fm_attn_dev.h
        auto prep = [&](float (&x0)[2], float (&x1)[2], const float (&w0)[2], const float (&w1)[2]) {
            if (at.qk_norm) {
                float ss = 0.f;
#pragma unroll
                for (int u = 0; u < 2; ++u) ss += x0[u] * x0[u] + x1[u] * x1[u];
                ss = wave_sum(ss);
                const float rs = 1.0f / sqrtf(ss / (float)hd + at.eps);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    x0[u] = bfround((x0[u] * rs) * w0[u]);
                    x1[u] = bfround((x1[u] * rs) * w1[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float y0 = bfround(x0[u] * c_[u] - x1[u] * s_[u]);
                const float y1 = bfround(x1[u] * c_[u] + x0[u] * s_[u]);
                x0[u] = y0;
                x1[u] = y1;
            }
        };
        if (M != 2 && A.ilp) {
            // the q and k chains are independent: both in one basic block (the same operations per chain as prep),
            // so their wave_sum, rsqrt and rounding sequences interleave
            if (at.qk_norm) {
                float sq = 0.f, sk = 0.f;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    sq += q0[u] * q0[u] + q1[u] * q1[u];
                    sk += k0[u] * k0[u] + k1[u] * k1[u];
                }
                sq = wave_sum(sq);
                sk = wave_sum(sk);
                const float rq = 1.0f / sqrtf(sq / (float)hd + at.eps), rk = 1.0f / sqrtf(sk / (float)hd + at.eps);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    q0[u] = bfround((q0[u] * rq) * qw0[u]);
                    q1[u] = bfround((q1[u] * rq) * qw1[u]);
                    k0[u] = bfround((k0[u] * rk) * kw0[u]);
                    k1[u] = bfround((k1[u] * rk) * kw1[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float a0 = bfround(q0[u] * c_[u] - q1[u] * s_[u]), a1 = bfround(q1[u] * c_[u] + q0[u] * s_[u]);
                const float b0 = bfround(k0[u] * c_[u] - k1[u] * s_[u]), b1 = bfround(k1[u] * c_[u] + k0[u] * s_[u]);
                q0[u] = a0;
                q1[u] = a1;
                k0[u] = b0;
                k1[u] = b1;
            }
        } else {
            if constexpr (M != 2) prep(q0, q1, qw0, qw1);
            prep(k0, k1, kw0, kw1);
        }
        if (wave == 0) {  // the group's new k / v of cpos into the fast cache
            bf16_t* kd = at.kc + base + (size_t)cpos * hd;
            bf16_t* vd = at.vc + base + (size_t)cpos * hd;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int p = lane + 64 * u;
                if (p < half) {
                    *reinterpret_cast<uint32_t*>(kd + 2 * p) = (uint32_t)f2bf(k0[u]) | ((uint32_t)f2bf(k1[u]) << 16);
                    *reinterpret_cast<uint32_t*>(vd + 2 * p) = (uint32_t)f2bf(v0[u]) | ((uint32_t)f2bf(v1[u]) << 16);
                }
            }
        }
        __syncthreads();  // K / V rows staged
        const unsigned long long ts1 = A.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
        if (!live) return;
        const bf16_t* Ks = kvs;
        const bf16_t* Vs = kvs + FW_MAXJ * FW_MAXHD;
        // scores round(round(q.k) * scale), softmax, probabilities rounded (fast SDPA path)
        float o0[2] = {0.f, 0.f}, o1[2] = {0.f, 0.f};
        if constexpr (M == 2) {  // the one score's softmax is 1 (finite score): o = 0 + 1 * v
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                o0[u] = 0.f + v0[u];
                o1[u] = 0.f + v1[u];
            }
        } else if (A.ilp) {  // one basic block per position count (fw_attend); counts past 10 rounded up to 12 / 16
#define FWA(n) fw_attend<n>(Ks, Vs, hd, half, cpos, lane, at.scale, q0[0], q1[0], k0[0], k1[0], v0[0], v1[0], o0[0], o1[0])
            switch (cpos) {
                case 0: FWA(1); break;
                case 1: FWA(2); break;
                case 2: FWA(3); break;
                case 3: FWA(4); break;
                case 4: FWA(5); break;
                case 5: FWA(6); break;
                case 6: FWA(7); break;
                case 7: FWA(8); break;
                case 8: FWA(9); break;
                case 9: FWA(10); break;
                case 10: case 11: FWA(12); break;
                default: FWA(16); break;
            }
#undef FWA
        } else {
        float sc[FW_MAXJ + 1];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j <= FW_MAXJ; ++j) {
            if (j > cpos) break;
            float d = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int p = lane + 64 * u;
                const int pp = p < half ? p : 0;
                float a0 = k0[u], a1 = k1[u];
                if (j < cpos) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(Ks + j * hd + 2 * pp);
                    a0 = p < half ? lo16(w) : 0.f;
                    a1 = p < half ? hi16(w) : 0.f;
                }
                d += q0[u] * a0 + q1[u] * a1;
            }
            d = wave_sum(d);
            sc[j] = bfround(bfround(d) * at.scale);
            mx = fmaxf(mx, sc[j]);
        }
        float den = 0.f;
#pragma unroll
        for (int j = 0; j <= FW_MAXJ; ++j) {
            if (j > cpos) break;
            sc[j] = expf(sc[j] - mx);
            den += sc[j];
        }
#pragma unroll
        for (int j = 0; j <= FW_MAXJ; ++j) {
            if (j > cpos) break;
            const float pj = bfround(sc[j] / den);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int p = lane + 64 * u;
                const int pp = p < half ? p : 0;
                float b0 = v0[u], b1 = v1[u];
                if (j < cpos) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(Vs + j * hd + 2 * pp);
                    b0 = lo16(w);
                    b1 = hi16(w);
                }
                o0[u] += pj * b0;
                o1[u] += pj * b1;
            }
        }
        }
        // tagged write-through store: word = bf16 << 16 | gen
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int p = lane + 64 * u;
            if (p < half) {
                const uint64_t w = (uint64_t)(((uint32_t)f2bf(o0[u]) << 16) | gen) |
                                   ((uint64_t)(((uint32_t)f2bf(o1[u]) << 16) | gen) << 32);
                __hip_atomic_store(reinterpret_cast<uint64_t*>(A.xt + (size_t)h * hd + 2 * p), w, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (A.dbg && lane == 0) {  // developer record per attention wave (tag 0xFFF9): start, staged, stored
            const unsigned long long t[7] = {ts0, ts1, __builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0};
            dbg_record(A.dbg, 0xFFF9, (unsigned)h, t);
        }
        return;
    }
    // ---------------- wo rows 2p, 2p + 1: rowgemv_body FIN with x from the tagged words --------
    rowgemv_body<U, 2, false, 1, G, QM, true>(A.wo, (int)blockIdx.x - at.nkv, A.xt, gen, A.err);
}

// The pair form (fm_tune fast_pair; bf16): codebook positions 0 and 1 of the fast decoder in ONE launch.  Row 0 is
// the slow model's hidden row at position 0, row 1 the embedding of the code the slow sampler drew, at position 1;
// both are known before the fast passes start, and row 1 needs of row 0 only its K / V at this layer.  An
// attention block does both rows of its kv group:
//   row 0  form 2's arithmetic: k normed, rotated (position 0) and cached with v, output 0 + v (no Q);
//   row 1  form 0 / 1 at cpos 1: q, k normed and rotated (position 1), k / v cached, then fw_attend<2> with
//          position 0's K / V row staged in LDS from row 0's registers -- the rounded bf16 values the cache
//          holds, so no cache load and no other block is waited for.
// TAB: row 1's raw q|k|v row comes from the table (form 1: the first layer; its residual row is gathered too),
// else it is row 1 of at.qkv.  XR 2: both rows' outputs are published (K tagged words each) and the wo blocks
// run the two-row TX body; XR 1 (the last layer): row 0 ends at its K / V write, the wo blocks take row 1 only
// (A.wo holds row 1's residual and output).  One gen per launch, the tag of position 1's launch index.
// Each operation on each row is the one-row kernel's, in its order (the second RoPE pair of a lane, masked to
// zero there because hd <= FW_MAXHD, only adds +0 to sums that are never -0 and is left out).
// QM 1 / 2 (fm_tune fast_pair_q): the attention blocks are the same; the wo blocks run the two-row TX body on int8 /
// int4 codes.  The hand-off, the tag, the poll bound and err are QM 0's.
template <int U, bool TAB, int XR, int QM>
__device__ __forceinline__ void fattn_wo_pair_body(const FattnWoArgs& A) {
    __shared__ __attribute__((aligned(16))) bf16_t kvs[4 * FW_MAXHD];  // K rows 0 .. 1, V rows 0 .. 1 (row 1: read, selected away)
    const FastFusedArgs<bf16_t>& at = A.at;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t gen = ((uint32_t)A.at.row_pos[0] * 41u + (uint32_t)A.gen) % 65535u + 1u;
    const unsigned long long ts0 = A.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
    if ((int)blockIdx.x < at.nkv) {
        if (A.prio) __builtin_amdgcn_s_setprio(3);
        const int kvh = blockIdx.x, hd = at.hd, g = at.nh / at.nkv, half = hd >> 1;
        const bf16_t* r0 = at.qkv;
        const bf16_t* r1 = at.qkv + at.ldqkv;
        if constexpr (TAB) {
            const int32_t iv = A.qidx[A.qcol];
            const int xi = iv < 0 ? 0 : (iv >= A.qrows ? A.qrows - 1 : iv);
            r1 = A.qtab + (size_t)xi * at.ldqkv;
        }
        const int slot = at.row_slot[0];
        const bool live = wave < g, in = lane < half;
        const int h = kvh * g + (live ? wave : 0), pp = in ? lane : 0;
        const float* tab0 = at.rope;
        const float* tab1 = at.rope + hd;
        const size_t base = (size_t)slot * at.slot_stride + at.layer_off + (size_t)kvh * at.S * hd;
        const size_t ko = (size_t)(at.nh + kvh) * hd + 2 * pp, vo = (size_t)(at.nh + at.nkv + kvh) * hd + 2 * pp;
        float ka0, ka1, va0, va1, q0, q1, k0, k1, v0, v1, qw0 = 1.f, qw1 = 1.f, kw0 = 1.f, kw1 = 1.f;
        ld_pair_bf(r0 + ko, ka0, ka1);
        ld_pair_bf(r0 + vo, va0, va1);
        ld_pair_bf(r1 + (size_t)h * hd + 2 * pp, q0, q1);
        ld_pair_bf(r1 + ko, k0, k1);
        ld_pair_bf(r1 + vo, v0, v1);
        if (at.qk_norm) {
            ld_pair_bf(at.qn + 2 * pp, qw0, qw1);
            ld_pair_bf(at.kn + 2 * pp, kw0, kw1);
        }
        const float ca = tab0[2 * pp], sa = tab0[2 * pp + 1], cb = tab1[2 * pp], sb = tab1[2 * pp + 1];
        if (!in) ka0 = ka1 = va0 = va1 = q0 = q1 = k0 = k1 = v0 = v1 = 0.f;
        // the three chains (row 0's k, row 1's q and k) side by side, each with prep's operations
        if (at.qk_norm) {
            float sa_ = 0.f, sq = 0.f, sk = 0.f;
            sa_ += ka0 * ka0 + ka1 * ka1;
            sq += q0 * q0 + q1 * q1;
            sk += k0 * k0 + k1 * k1;
            sa_ = wave_sum(sa_);
            sq = wave_sum(sq);
            sk = wave_sum(sk);
            const float ra = 1.0f / sqrtf(sa_ / (float)hd + at.eps), rq = 1.0f / sqrtf(sq / (float)hd + at.eps),
                        rk = 1.0f / sqrtf(sk / (float)hd + at.eps);
            ka0 = bfround((ka0 * ra) * kw0);
            ka1 = bfround((ka1 * ra) * kw1);
            q0 = bfround((q0 * rq) * qw0);
            q1 = bfround((q1 * rq) * qw1);
            k0 = bfround((k0 * rk) * kw0);
            k1 = bfround((k1 * rk) * kw1);
        }
        {
            const float a0 = bfround(ka0 * ca - ka1 * sa), a1 = bfround(ka1 * ca + ka0 * sa);
            const float b0 = bfround(q0 * cb - q1 * sb), b1 = bfround(q1 * cb + q0 * sb);
            const float c0 = bfround(k0 * cb - k1 * sb), c1 = bfround(k1 * cb + k0 * sb);
            ka0 = a0;
            ka1 = a1;
            q0 = b0;
            q1 = b1;
            k0 = c0;
            k1 = c1;
        }
        if (wave == 0 && in) {  // both positions into the fast cache; position 0's row staged for row 1's scores
            const uint32_t kw = (uint32_t)f2bf(ka0) | ((uint32_t)f2bf(ka1) << 16);
            const uint32_t vw = (uint32_t)f2bf(va0) | ((uint32_t)f2bf(va1) << 16);
            *reinterpret_cast<uint32_t*>(at.kc + base + 2 * lane) = kw;
            *reinterpret_cast<uint32_t*>(at.vc + base + 2 * lane) = vw;
            *reinterpret_cast<uint32_t*>(at.kc + base + hd + 2 * lane) = (uint32_t)f2bf(k0) | ((uint32_t)f2bf(k1) << 16);
            *reinterpret_cast<uint32_t*>(at.vc + base + hd + 2 * lane) = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
            *reinterpret_cast<uint32_t*>(kvs + 2 * lane) = kw;
            *reinterpret_cast<uint32_t*>(kvs + 2 * FW_MAXHD + 2 * lane) = vw;
        }
        __syncthreads();
        const unsigned long long ts1 = A.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
        if (!live) return;
        float o0 = 0.f, o1 = 0.f;
        fw_attend<2>(kvs, kvs + 2 * FW_MAXHD, hd, half, 1, lane, at.scale, q0, q1, k0, k1, v0, v1, o0, o1);
        const int K = at.nh * hd;
        if (in) {
            if constexpr (XR == 2) {  // row 0: one position, softmax = {1}, output 0 + v
                const float p0 = 0.f + va0, p1 = 0.f + va1;
                const uint64_t w = (uint64_t)(((uint32_t)f2bf(p0) << 16) | gen) | ((uint64_t)(((uint32_t)f2bf(p1) << 16) | gen) << 32);
                __hip_atomic_store(reinterpret_cast<uint64_t*>(A.xt + (size_t)h * hd + 2 * lane), w, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            const uint64_t w = (uint64_t)(((uint32_t)f2bf(o0) << 16) | gen) | ((uint64_t)(((uint32_t)f2bf(o1) << 16) | gen) << 32);
            __hip_atomic_store(reinterpret_cast<uint64_t*>(A.xt + K + (size_t)h * hd + 2 * lane), w, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        if (A.dbg && lane == 0) {  // one attention-wave record per row whose output this wave produced
            const unsigned long long t[7] = {ts0, ts1, __builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0};
#pragma unroll
            for (int x = 0; x < XR; ++x) dbg_record(A.dbg, 0xFFF9, (unsigned)h, t);
        }
        return;
    }
    rowgemv_body<U, 2, false, 1, TAB, QM, true, XR>(A.wo, (int)blockIdx.x - at.nkv, XR == 2 ? A.xt : A.xt + A.wo.K, gen, A.err);
}
template <int U, bool TAB, int XR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
void fattn_wo_pair_kernel(FattnWoArgs A) {
    fattn_wo_pair_body<U, TAB, XR, 0>(A);
}
template <int U, bool TAB, int XR, int QM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
void fattn_wo_pair_q_kernel(FattnWoArgs A) {
    static_assert(QM == 1 || QM == 2, "the code forms");
    fattn_wo_pair_body<U, TAB, XR, QM>(A);
}

bool fattn_wo_ok(int nh, int nkv, int hd, int cpos, int N, int K, int qm) {
    const int U = rowgemv_u(K, qm);
    return nkv > 0 && nh % nkv == 0 && nh / nkv <= 4 && hd % 2 == 0 && hd <= FW_MAXHD && cpos >= 0 &&
           cpos < FW_MAXJ + 1 && K == nh * hd && N % 2 == 0 && U > 0 && U <= 8;
}

// Whether the table (M 1) and K / V-only (M 2) forms at depth K of int8 (qm 1) / int4 (qm 2) weights may be
// dispatched: the launch is deadlock-free only while its whole grid is resident -- at most 80 VGPRs, no scratch,
// under 26 KiB LDS (code-object metadata).  Elsewhere the frame keeps its launches.
bool fattn_wo_dead_ok(int K, int qm) {
    const int U = rowgemv_u(K, qm);
    // int8 / int4: depths 2 .. 5 hold 36 .. 79 VGPRs without scratch; 6 and 8 spill (20 .. 136 B per lane at 80 VGPRs,
    // as their M 0 forms do) and are not instantiated
    return U > 0 && U <= (qm ? 5 : 8);
}

void launch_fattn_wo(hipStream_t s, const FattnWoArgs& A0) {
    FattnWoArgs A = A0;
    A.dbg = fm_tuning().dbg;
    A.wo.dbg = A.dbg;
    const FastFusedArgs<bf16_t>& at = A.at;
    const int qm = A.wo.Wq4 ? 2 : (A.wo.Wq ? 1 : 0);
    FMCHECK(fattn_wo_ok(at.nh, at.nkv, at.hd, at.cpos, A.wo.N, A.wo.K, qm) && A.xt && A.err && A.gen > 0 && A.gen <= 40 && at.row_pos &&
                A.wo.res && A.wo.res_out &&
                (qm == 2 ? (A.wo.wsz && A.wo.gs % 8 == 0 && !A.wo.bias) : (qm == 1 ? (A.wo.wscale && !A.wo.bias) : A.wo.W != nullptr)),
            "fused fast attention + wo: shapes, tag and buffers");
    const dim3 grid(at.nkv + A.wo.N / 2), block(256);
    const bool G = A.wo.residx != nullptr;
    // the table form gathers its residual row by the same index; the K / V-only form runs at codebook 0 (no gather)
    FMCHECK(!A.qtab || (G && !A.kv0 && A.qidx == A.wo.residx && A.qcol == A.wo.res_col && A.qrows > 0 &&
                        A.qrows == A.wo.res_rows),
            "fused fast attention + wo: the QKV table form is gathered by the residual's index");
    FMCHECK(!A.kv0 || (!G && at.cpos == 0), "fused fast attention + wo: the K / V-only form runs at codebook 0");
    FMCHECK(!(A.qtab || A.kv0) || fattn_wo_dead_ok(A.wo.K, qm),
            "fused fast attention + wo: no resident table / K-V-only form at this depth of int8 / int4 weights");
    if (A.pair) {
        FMCHECK(!A.kv0 && at.cpos == 1 && at.S >= 2 && rowgemv_pair_ok(-1, A.wo.K, false, qm) && (A.qtab != nullptr) == G && (A.pair == 2 || (A.wo.res1 && A.wo.res_out1)),
                "fused fast attention + wo, pair form: positions 0 and 1, both rows' residuals set, an instantiated depth (bf16 2 .. 5 "
                "chunks of 256 k per wave; int8 codes 2, int4 codes 2 .. 3 chunks of 512 k)");
        const bool two = A.pair != 2;
        // (a one-layer stack would pair the table form with the last-layer form; its row-1 words would also be
        // written by one launch index only, so two slots at one position could not tell each other's words apart)
        FMCHECK(two || !A.qtab, "fused fast attention + wo, pair form: the first layer is not the last");
        if (qm) {  // fm_tune fast_pair_q: the resident depths (rowgemv_pair_ok)
            auto pq = [&](auto q) {
                constexpr int Q = decltype(q)::value;
#define FW(u)                                                                                                    \
    (A.qtab ? fattn_wo_pair_q_kernel<u, true, 2, Q>                                                              \
            : (two ? fattn_wo_pair_q_kernel<u, false, 2, Q> : fattn_wo_pair_q_kernel<u, false, 1, Q>))<<<grid, block, 0, s>>>(A)
                const int u = rowgemv_u(A.wo.K, Q);
                if (u == 2) FW(2);
                else if (Q == 2 && u == 3) {
                    if constexpr (Q == 2) FW(3);
                } else {
                    FMCHECK(false, "fused fast attention + wo, pair form on codes: int8 has depth 2, int4 depths 2 .. 3");
                }
#undef FW
            };
            if (qm == 2) pq(std::integral_constant<int, 2>{});
            else pq(std::integral_constant<int, 1>{});
            return;
        }
        switch (rowgemv_u(A.wo.K, 0)) {
#define FW(u)                                                                                                            \
    case u:                                                                                                              \
        (A.qtab ? fattn_wo_pair_kernel<u, true, 2>                                                                       \
                : (two ? fattn_wo_pair_kernel<u, false, 2> : fattn_wo_pair_kernel<u, false, 1>))<<<grid, block, 0, s>>>(A); \
        break;
            FW(2) FW(3) FW(4)
            default: FW(5)
#undef FW
        }
        return;
    }
    if ((A.qtab || A.kv0) && qm) {  // fm_tune fast_dead_q: the depths fattn_wo_dead_ok admits
        auto dead = [&](auto q) {
            constexpr int Q = decltype(q)::value;
            switch (rowgemv_u(A.wo.K, Q)) {
#define FW(u) \
    case u: (A.qtab ? fattn_wo_kernel<u, true, Q, 1> : fattn_wo_kernel<u, false, Q, 2>)<<<grid, block, 0, s>>>(A); break;
                FW(2) FW(3) FW(4)
                default: FW(5)
#undef FW
            }
        };
        if (qm == 2) dead(std::integral_constant<int, 2>{});
        else dead(std::integral_constant<int, 1>{});
        return;
    }
    if (A.qtab || A.kv0) {
        switch (rowgemv_u(A.wo.K, 0)) {
#define FW(u) \
    case u: (A.qtab ? fattn_wo_kernel<u, true, 0, 1> : fattn_wo_kernel<u, false, 0, 2>)<<<grid, block, 0, s>>>(A); break;
            FW(2) FW(3) FW(4) FW(5) FW(6)
            default: (A.qtab ? fattn_wo_kernel<8, true, 0, 1> : fattn_wo_kernel<8, false, 0, 2>)<<<grid, block, 0, s>>>(A); break;
#undef FW
        }
        return;
    }
    auto go = [&](auto q) {
        constexpr int Q = decltype(q)::value;
        switch (rowgemv_u(A.wo.K, Q)) {
#define FW(u) \
    case u: (G ? fattn_wo_kernel<u, true, Q, 0> : fattn_wo_kernel<u, false, Q, 0>)<<<grid, block, 0, s>>>(A); break;
            FW(2) FW(3) FW(4) FW(5) FW(6)
            default: (G ? fattn_wo_kernel<8, true, Q, 0> : fattn_wo_kernel<8, false, Q, 0>)<<<grid, block, 0, s>>>(A); break;
#undef FW
        }
    };
    if (qm == 2) go(std::integral_constant<int, 2>{});
    else if (qm == 1) go(std::integral_constant<int, 1>{});
    else go(std::integral_constant<int, 0>{});
}

// =========================================================================================
// Slow-model attention + wo in ONE launch (batch 1, bf16 compute; fm_tune slow_attn_wo on unquantised handles,
// slow_attn_wo_q on weight-only int8 / int4 ones).
//
// The same arrangement as fattn_wo_kernel with the slow decode attention as the producer.  Linear block indices
// 0 .. nh * maxsplit - 1 are attn_fd's blocks at 8 waves and one q head per block -- index b is block
// (0, b % nkv, b / nkv) of attn_fd_kernel's grid, so kvh stays the fastest-varying index and a block lands on the
// XCD it lands on in the stand-alone launch (kv_prefetch's L2).  They run attn_fd_body unchanged but for the final
// store, which goes out as tagged write-through words.  They never wait for another block: a split past nsp leaves
// after its first round trip and the combine is done by the last arriver.  The remaining blocks are wo's: two
// independent 4-wave groups per 512-thread block, each the TX row block of rowgemv_body on RP rows (its own red
// slice; per output row the operations of rowgemv_kernel<U, 2, false, 1, false, QM> in their order, which do not
// depend on RP nor on the group's place in the block).  QM 1 (int8 codes): the lane's xs over its chunks in chunk
// order, the four wave sums of xs added in wave order and the epilogue round(round(v - 128 * sum x) * scale[row])
// are the stand-alone kernel's; the scale is row n0 + tid % RP's, loaded in the first round trip.  QM 2 (int4 code
// words): per word the dot8r pair (B and the lane's sum of x) and the two fmas of the word's group (scale, zero), of
// row n0 + r, in chunk order.  A wo group issues its whole weight run (int4: its (scale, zero) words too), then
// re-reads its x words until every tag is current.  It waits on attention blocks only, which have lower block
// indices and are dispatched first; every wait is bounded and sets *err.
template <int U, int HD, int RP, int QM = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4)))
void slow_attn_wo_kernel(SlowAttnWoArgs A) {
    const AttnDecArgs<bf16_t>& at = A.at;
    // the tag: fattn_wo_kernel's formula on the slow launches' own indices and their own buffer
    const uint32_t gen = ((uint32_t)at.row_pos[0] * 41u + (uint32_t)A.gen) % 65535u + 1u;
    const int natt = at.nh * at.maxsplit;
    if ((int)blockIdx.x < natt) {
        const int b = blockIdx.x;
        attn_fd_body<bf16_t, HD, 8, 1, true>(at, 0, b % at.nkv, b / at.nkv, 1, A.xt, gen);
        return;
    }
    // the first read of x waits for a share of the attention's duration as the position gives it: about 3 us of round
    // trips and fold, 12 ns per position of the block's split, 1.8 us of ticket and combine past one split (10-ns ticks;
    // profiles/slow_attn_wo_probe.txt)
    TxPoll pw;
    if (RP == 4 && A.delay_pct) {
        const int npos = at.row_pos[0] + 1;
        const int nsp = min(at.maxsplit, (npos + at.cap - 1) / at.cap);
        const int chunk = ((npos + nsp - 1) / nsp + 15) & ~15;
        pw.delay = (unsigned)(A.delay_pct * (300 + chunk * 12 / 10 + (nsp > 1 ? 180 : 0)) / 100);
    }
    pw.sleep = A.sleep;
    pw.cheap = A.cheap;
    rowgemv_body<U, RP, false, 1, false, QM, true, 1, 2>(A.wo, 2 * ((int)blockIdx.x - natt) + (int)(threadIdx.x >> 8), A.xt, gen,
                                                        A.err, pw);
}

// the instantiated forms: head_dim 128, at most 4 q heads per kv head, wo rows in whole blocks of both forms (8 rows),
// depths 2 and 4 (S2-Pro: 32 / 8 heads x 128, K 4096: depth 4 of 256-k chunks on bf16 weights, depth 2 of 512-k
// chunks on int8 / int4 codes).  Every form, qm 1 / 2 included, holds the gate: 115 VGPRs, no scratch, LDS that lets
// two 512-thread blocks share a CU (profiles/slow_attn_wo_q_regs.txt)
bool slow_attn_wo_ok(int nh, int nkv, int hd, int N, int K, int qm) {
    if (qm < 0 || qm > 2) return false;
    const int U = rowgemv_u(K, qm);
    return nkv > 0 && nh % nkv == 0 && attn_fd_ok(hd, nh / nkv) && hd == 128 && K == nh * hd && N > 0 && N % 8 == 0 &&
           (U == 2 || U == 4);
}

void launch_slow_attn_wo(hipStream_t s, const SlowAttnWoArgs& A0) {
    SlowAttnWoArgs A = A0;
    AttnDecArgs<bf16_t>& at = A.at;
    at.dbg = A.wo.dbg = fm_tuning().dbg;
    if (A.sleep < 1) A.sleep = 1;
    const int qm = A.wo.Wq4 ? 2 : (A.wo.Wq ? 1 : 0);
    FMCHECK(A.delay_pct >= 0 && A.delay_pct <= 300, "fused slow attention + wo: first-read delay of 0 .. 300 per cent");
    FMCHECK(slow_attn_wo_ok(at.nh, at.nkv, at.hd, A.wo.N, A.wo.K, qm) && A.xt && A.err && A.gen > 0 && A.gen <= 40 && at.row_pos &&
                at.row_slot && at.cap >= 16 && at.cnt && at.part && !at.qslab && (A.rp == 2 || A.rp == 4) && A.wo.X &&
                A.wo.res && A.wo.res_out && !A.wo.residx && A.wo.xr != 2,
            "fused slow attention + wo: shapes, tag and buffers");
    FMCHECK(qm == 2 ? (A.wo.wsz && A.wo.gs > 0 && A.wo.gs % 8 == 0 && A.wo.K % A.wo.gs == 0 && !A.wo.bias && !A.wo.Wq && !A.wo.W)
                    : (qm == 1 ? (A.wo.wscale && !A.wo.bias && !A.wo.W) : A.wo.W != nullptr),
            "fused slow attention + wo: bf16 weights, int8 codes + row scales or int4 code words + group (scale, zero), "
            "the code forms without bias");
    at.maxsplit = std::min(FD_NSP, FM_CEIL(at.S, at.cap));
    at.nwb = 8;
    at.hpb = 1;
    const dim3 grid(at.nh * at.maxsplit + A.wo.N / (2 * A.rp)), block(512);
    const int U = rowgemv_u(A.wo.K, qm);
    auto go = [&](auto q) {
        constexpr int Q = decltype(q)::value;
#define SW(u, hd) \
    (A.rp == 4 ? slow_attn_wo_kernel<u, hd, 4, Q><<<grid, block, 0, s>>>(A) : slow_attn_wo_kernel<u, hd, 2, Q><<<grid, block, 0, s>>>(A))
        if (U == 2) SW(2, 128);
        else SW(4, 128);
#undef SW
    };
    if (qm == 2) go(std::integral_constant<int, 2>{});
    else if (qm == 1) go(std::integral_constant<int, 1>{});
    else go(std::integral_constant<int, 0>{});
}
