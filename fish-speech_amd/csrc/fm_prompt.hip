// fm_prompt.hip -- prompt-chunk linears at 32 < R <= 64 rows (bf16): one weight pass for every row.
//
// A prompt chunk (the prefill of a short prompt: config 2's 64 tokens, a speaker turn's text) runs
// each TransformerBlock linear (llama.py:838-843, 883-890, 978-986) on R activation rows.  At
// R <= 64 that is a weight stream, not a GEMM: 2 R flops per weight byte.  The codec's LDS-tiled
// conv GEMMs (fm_codec_kernels.hip) tile M = 128 rows x 96-128 columns and stream the 7.3 GB of
// S2-Pro weights at about 1.15 TB/s there (profiles/r06_prefill64_kernels.md).
//
// Here each wave owns one 16-row weight tile and streams its fragments of the packed layout
// (fm_kernels.h: 1 KiB of contiguous HBM per 16 x 32 fragment, non-temporal) through a two-set
// register ring, 8 k-steps ahead.  The R activation rows are staged through LDS in 128-k chunks
// (double-buffered, LDS-only barriers, so the weight loads stay in flight across them) and serve as
// the MFMA B operands of all 64 rows: 4 accumulators per wave.  Block = 4 waves = 64 weight rows.
// The K range is cut into ks slices (grid y) so the grid fills the chip; each slice writes raw fp32
// partials to the conv split-K slab layout [ks][R][N], and conv_splitk_epi_kernel applies the
// epilogue: round(sum of slices + bias), the residual, the store.  The fp32 sum over slices runs in
// slice order, each slice's MFMA chain in k order.  An unsliced w1 || w3 (act set) applies the
// interleaved SwiGLU itself (no slab, no epilogue launch; swiglu_i8_kernel's roundings).
//
// Measured forms that lost (profiles/r06_prompt_skinny_v3_trace.md, 64-token prefill): loading the
// activation chunks two ahead (6.88 vs 6.57 ms), staging a whole <= 20-step slice at once with a
// 16-deep ring (7.31 ms: 82 KiB of LDS leaves one block per CU), and no LDS at all -- each wave
// loading its 4 activation fragments per k-step from L2 beside its weight fragment (10.03 vs
// 6.05 ms: 4x the weight bytes through L2; w1 || w3 92 vs 34 us, profiles/r06_prompt_skinny_l2direct_trace.md).
// Neutral or slower: 8-step chunks (6.15 vs 6.04 ms, profiles/r06_prompt_chunk8_trace.md), grid
// targets of 384-1024 blocks (6.04-6.30 ms, profiles/r06_prompt_blocks_sweep.txt), and a third weight
// set in the ring (6.25 vs 6.08 ms; w1 || w3 38.9 vs 34 us).
//
// WM, the weight mode (weight-only int8 / int4 handles; fm_tune prompt_skinny_q).  0: the packed bf16 fragments
// of a.w, as above.  1 (int8): a.w is null and the ring holds the lane's 8 code bytes of each k-step, from the
// step-granular copy a.q8s [ceil(N/16)][K/32] x 512 B (launch_pack_q8s); Frag::dq8s expands a slot right
// before that step's four MFMAs.  2 (int4, group size a multiple of 128): the ring holds the lane's 4-byte word
// of a.q4s (launch_pack_q4s), and the (scale, zero) word of (tile, 128-k unit, row lane & 15) comes from a.sz
// (launch_pack_sz4).  A slice may start inside a unit (S2-Pro w2: 8 slices of 38 k-steps), so the unit of step
// s0 + 4 c + q is (s0 + 4 c + q) >> 2, not c: a chunk's four steps touch two units at most, both words are
// loaded with the chunk's set, ahead of its code words (vmcnt retires in order: no MFMA then waits for more
// than its own slot's predecessors), and one select picks the step's.  Frag::dq4s gives bf16(fma(q - 8, scale,
// zero)), the bits the bf16 copy holds.  Slices, steps, their order and the four accumulators are mode 0's, so
// the three modes write the same bytes.  A ring slot is 2 VGPRs (int8) or 1 (int4) instead of 4, and the code
// modes use that room for a deeper ring: three sets for int8 (12 k-steps ahead, 6 of mode 0's 8 KiB in flight
// per wave), four for int4 (16 k-steps, 4 KiB).  No instantiation spills, and every one keeps the 4 waves per
// SIMD the LDS allows (VGPRs + AGPRs: mode 0 94-126, int8 108-122, int4 94-128).  Seen on the
// compiler, not timed: four int8 sets take the 10- and 20-chunk unrolled forms to 130 registers, 3 waves per
// SIMD; the (scale, zero) words of a set kept as a two-element array turn the step's select into an indexed
// scratch access (48 B a lane), so they are two scalars per set.  Not tried: two-set code rings, eight int4 sets.
#include "fm_codec.h"
#include "fm_frag.h"
#include "fm_kernels.h"
#include "fm_runtime.h"

namespace {

constexpr int SK_CK = 128;          // k per staged activation chunk (4 MFMA k-steps)
constexpr int SK_XS = SK_CK + 8;    // LDS row stride in bf16 (272 B: 16-B row reads without bank conflicts)

// one k-step's raw weight operand in the ring: the fragment itself, 8 code bytes, or one word of 8 nibbles
template <int WM> struct SkRaw { typedef u32x4_t t; };
template <> struct SkRaw<1> { typedef u32x2_t t; };
template <> struct SkRaw<2> { typedef uint32_t t; };
template <int WM> constexpr int SK_NS = WM == 2 ? 4 : (WM == 1 ? 3 : 2);  // ring depth in sets of 4 k-steps

// A wave's weight stream over its K slice (k-steps [s0, s0 + kps) of tile tl): the loads of one ring set
// and the expansion of one slot.
template <int WM> struct SkW {
    using F = Frag<bf16_t>;
    typedef typename SkRaw<WM>::t raw_t;
    const bf16_t* wb = nullptr;     // WM 0: the slice's first fragment
    const u32x2_t* q8p = nullptr;   // WM 1: the lane's 8 bytes of it
    const uint32_t* q4p = nullptr;  // WM 2: the lane's word of it ...
    const uint32_t* szp = nullptr;  //       ... and the tile's (scale, zero) words [K / 128][16] at row lane & 15
    int kps, lane, s0, ul;          // ul: the unit of the slice's last step
    __device__ __forceinline__ SkW(const PromptSkinnyArgs& a, int tl, int nks, int s0_, int kps_, int lane_)
        : kps(kps_), lane(lane_), s0(s0_), ul((s0_ + kps_ - 1) >> 2) {
        const size_t f0 = (size_t)tl * nks + s0;
        if constexpr (WM == 0) wb = a.w + f0 * 512;
        if constexpr (WM == 1) q8p = reinterpret_cast<const u32x2_t*>(a.q8s + f0 * 512) + lane;
        if constexpr (WM == 2) {
            q4p = a.q4s + f0 * 64 + lane;
            szp = a.sz + (size_t)tl * (a.K >> 7) * 16 + (lane & 15);
        }
    }
    // chunk c's 4 k-steps (steps past the slice re-read its first one; never multiplied)
    __device__ __forceinline__ void load(raw_t (&w)[4], uint32_t& z0, uint32_t& z1, int c) const {
        if constexpr (WM == 2) {  // units u0 and u0 + 1 (past the slice's last unit: that one again, never selected)
            const int u0 = (s0 + 4 * c) >> 2;
            z0 = szp[(size_t)u0 * 16];
            z1 = szp[(size_t)(u0 < ul ? u0 + 1 : ul) * 16];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int st = 4 * c + q;
            const size_t sc = st < kps ? st : 0;
            if constexpr (WM == 0) w[q] = F::load_w<true>(wb + sc * 512, lane);
            if constexpr (WM == 1) w[q] = __builtin_nontemporal_load(q8p + sc * 64);
            if constexpr (WM == 2) w[q] = __builtin_nontemporal_load(q4p + sc * 64);
        }
    }
    // slot q of a chunk as the bf16 fragment: step s0 + 4 c + q is in unit u0 + ((s0 & 3) + q >> 2)
    __device__ __forceinline__ F::f expand(raw_t v, uint32_t z0, uint32_t z1, int q) const {
        if constexpr (WM == 1) {
            return F::dq8s(v);
        } else if constexpr (WM == 2) {
            const uint32_t zz = ((s0 & 3) + q) >> 2 ? z1 : z0;
            return F::dq4s(v, __uint_as_float(zz << 16), __uint_as_float(zz & 0xffff0000u));
        } else {
            return v;
        }
    }
};

// the int8 row scales of the lane's four weight rows (16 tile + 4 (lane >> 4) + j), for the direct SwiGLU
__device__ __forceinline__ void sk_scales(const PromptSkinnyArgs& a, int tl, int lane, float (&sc)[4]) {
    if (a.wscale) {
        const bf16_t* p = a.wscale + 16 * tl + 4 * (lane >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = ld(p, j);
    }
}

// grid (ceil(N / 64), ks), 256 threads
template <int WM>
__global__ __launch_bounds__(256) void prompt_skinny_kernel(PromptSkinnyArgs a) {
    using F = Frag<bf16_t>;
    typedef typename SkRaw<WM>::t raw_t;
    constexpr int NS = SK_NS<WM>;
    __shared__ __attribute__((aligned(16))) bf16_t xs[2][64][SK_XS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntile = (a.N + 15) / 16;
    const int tile = blockIdx.x * 4 + wave;
    const bool live = tile < ntile;
    const int nks = a.K / 32;                    // k-steps of the whole row
    const int kps = nks / (int)gridDim.y;        // k-steps of this slice (host: divides)
    const int s0 = (int)blockIdx.y * kps;
    const int nch = (kps + 3) / 4;
    const int tl = live ? tile : ntile - 1;
    const SkW<WM> ws(a, tl, nks, s0, kps, lane);
    // ---- activation chunk c -> registers: 64 rows x 128 k = 1024 pieces of 16 B, 4 per thread
    u32x4_t xr[4];
    auto xload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = (int)threadIdx.x + 256 * i;
            const int row = piece >> 4, kq = piece & 15;
            const int kl = 128 * c + 8 * kq;  // k within the slice
            const bool ok = row < a.R && kl < 32 * kps;
            xr[i] = F::load_masked(a.x + (size_t)(ok ? row : 0) * a.ldx + 32 * s0 + (ok ? kl : 0), ok);
        }
    };
    auto xstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = (int)threadIdx.x + 256 * i;
            *reinterpret_cast<u32x4_t*>(&xs[buf][piece >> 4][8 * (piece & 15)]) = xr[i];
        }
    };
    // ---- weight ring: set c % NS holds chunk c's 4 k-steps (int4: and its two (scale, zero) words)
    raw_t w[NS][4];
    uint32_t wz0[NS], wz1[NS];  // (two arrays: a select between elements of one would index memory)
    f32x4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    xload(0);      // the first activation chunk goes out ahead of the ring (in-order vmcnt)
#pragma unroll
    for (int i = 0; i < NS; ++i)
        if (i == 0 || i < nch) ws.load(w[i], wz0[i], wz1[i], i);
    xstore(0);
    lds_barrier();
    auto chunk = [&](raw_t (&wc)[4], uint32_t& z0, uint32_t& z1, int c) {
        if (c + 1 < nch) xload(c + 1);  // next chunk's rows in flight under this chunk's MFMAs
        const int buf = c & 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (4 * c + q < kps) {
                const F::f wf = ws.expand(wc[q], z0, z1, q);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const F::f xb = F::load(&xs[buf][16 * t + (lane & 15)][32 * q + 8 * (lane >> 4)]);
                    acc[t] = F::mma(wf, xb, acc[t]);
                }
            }
        }
        if (c + NS < nch) ws.load(wc, z0, z1, c + NS);  // the set is free: refill it NS chunks ahead
        if (c + 1 < nch) xstore(buf ^ 1);  // that buffer's previous chunk was finished before the last barrier
        lds_barrier();
    };
    for (int c = 0; c < nch; c += NS) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i == 0 || c + i < nch) chunk(w[i], wz0[i], wz1[i], c + i);
    }
    if (a.act) {  // one slice: act[r][8 tile + 4 (lane >> 4) + j] = round(round(silu(g)) * u), g the gate
        // row 16 tile + 4 (lane >> 4) + j (lanes 0-31), u the up row 8 further (lane + 32); weight-only
        // int8: both are round(round(acc) * scale of their row) first
        float sc[4] = {1.f, 1.f, 1.f, 1.f};
        sk_scales(a, tl, lane, sc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = 16 * t + (lane & 15);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = acc[t][j];
                if (a.wscale) v = rnd<bf16_t>(rnd<bf16_t>(v) * sc[j]);
                const float g = rnd<bf16_t>(v);
                const float u = rnd<bf16_t>(__shfl_xor(v, 32));
                o[j] = rnd<bf16_t>(rnd<bf16_t>(g / (1.0f + expf(-g))) * u);
            }
            if (live && lane < 32 && r < a.R) {
                bf16_t* d = a.act + (size_t)r * a.lda + 8 * tile + 4 * (lane >> 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) st(d, j, o[j]);
            }
        }
        return;
    }
    if (!live) return;
    // lane: weight rows 16 tile + 4 (lane >> 4) + j, activation row 16 t + (lane & 15)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = 16 * t + (lane & 15);
        if (r < a.R)
            *reinterpret_cast<f32x4_t*>(a.slab + ((size_t)blockIdx.y * a.R + r) * a.N + 16 * tile + 4 * (lane >> 4)) = acc[t];
    }
}

// Fully unrolled form (fm_tune prompt_unroll): NCH chunks as straight-line code, so no load is pending
// across a loop back edge (where the compiler drains vmcnt), with each chunk's activation rows
// loaded two chunks ahead.  Same MFMA chains in the same k order: bit-identical partials.
template <int NCH, int WM>
__global__ __launch_bounds__(256) void prompt_skinny_unrolled_kernel(PromptSkinnyArgs a) {
    using F = Frag<bf16_t>;
    typedef typename SkRaw<WM>::t raw_t;
    constexpr int NS = SK_NS<WM>;
    __shared__ __attribute__((aligned(16))) bf16_t xs[2][64][SK_XS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntile = (a.N + 15) / 16;
    const int tile = blockIdx.x * 4 + wave;
    const bool live = tile < ntile;
    const int nks = a.K / 32;
    const int kps = nks / (int)gridDim.y;  // host: (kps + 3) / 4 == NCH
    const int s0 = (int)blockIdx.y * kps;
    const int tl = live ? tile : ntile - 1;
    const SkW<WM> ws(a, tl, nks, s0, kps, lane);
    u32x4_t xr[2][4];
    auto xload = [&](int set, int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = (int)threadIdx.x + 256 * i;
            const int row = piece >> 4, kq = piece & 15;
            const int kl = 128 * c + 8 * kq;
            const bool ok = row < a.R && kl < 32 * kps;
            xr[set][i] = F::load_masked(a.x + (size_t)(ok ? row : 0) * a.ldx + 32 * s0 + (ok ? kl : 0), ok);
        }
    };
    auto xstore = [&](int set, int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = (int)threadIdx.x + 256 * i;
            *reinterpret_cast<u32x4_t*>(&xs[buf][piece >> 4][8 * (piece & 15)]) = xr[set][i];
        }
    };
    raw_t w[NS][4];
    uint32_t wz0[NS], wz1[NS];  // (two arrays: a select between elements of one would index memory)
    f32x4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    xload(0, 0);
    if (NCH > 1) xload(1, 1);
#pragma unroll
    for (int i = 0; i < NS; ++i)
        if (i < NCH) ws.load(w[i], wz0[i], wz1[i], i);
    xstore(0, 0);
    lds_barrier();
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 2 < NCH) xload(c & 1, c + 2);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (4 * c + q < kps) {
                const F::f wf = ws.expand(w[c % NS][q], wz0[c % NS], wz1[c % NS], q);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const F::f xb = F::load(&xs[c & 1][16 * t + (lane & 15)][32 * q + 8 * (lane >> 4)]);
                    acc[t] = F::mma(wf, xb, acc[t]);
                }
            }
        }
        if (c + NS < NCH) ws.load(w[c % NS], wz0[c % NS], wz1[c % NS], c + NS);
        if (c + 1 < NCH) xstore((c + 1) & 1, (c + 1) & 1);
        lds_barrier();
    }
    if (a.act) {
        float sc[4] = {1.f, 1.f, 1.f, 1.f};
        sk_scales(a, tl, lane, sc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = 16 * t + (lane & 15);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = acc[t][j];
                if (a.wscale) v = rnd<bf16_t>(rnd<bf16_t>(v) * sc[j]);
                const float g = rnd<bf16_t>(v);
                const float u = rnd<bf16_t>(__shfl_xor(v, 32));
                o[j] = rnd<bf16_t>(rnd<bf16_t>(g / (1.0f + expf(-g))) * u);
            }
            if (live && lane < 32 && r < a.R) {
                bf16_t* d = a.act + (size_t)r * a.lda + 8 * tile + 4 * (lane >> 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) st(d, j, o[j]);
            }
        }
        return;
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = 16 * t + (lane & 15);
        if (r < a.R)
            *reinterpret_cast<f32x4_t*>(a.slab + ((size_t)blockIdx.y * a.R + r) * a.N + 16 * tile + 4 * (lane >> 4)) = acc[t];
    }
}

template <int WM> void skinny_dispatch(hipStream_t s, const PromptSkinnyArgs& a, int ks) {
    const dim3 grid((a.N + 63) / 64, ks);
    const int nch = (a.K / 32 / ks + 3) / 4;
    if (fm_tuning().prompt_unroll) {
        switch (nch) {
            case 4: prompt_skinny_unrolled_kernel<4, WM><<<grid, 256, 0, s>>>(a); return;
            case 5: prompt_skinny_unrolled_kernel<5, WM><<<grid, 256, 0, s>>>(a); return;
            case 10: prompt_skinny_unrolled_kernel<10, WM><<<grid, 256, 0, s>>>(a); return;
            case 20: prompt_skinny_unrolled_kernel<20, WM><<<grid, 256, 0, s>>>(a); return;
            default: break;
        }
    }
    prompt_skinny_kernel<WM><<<grid, 256, 0, s>>>(a);
}

}  // namespace

int prompt_skinny_ks(int N, int K, int target) {
    const int groups = (N + 63) / 64, nks = K / 32;
    int ks = 0;
    for (int d = 1; d <= nks; ++d) {
        if (nks % d || nks / d < 8) continue;
        ks = d;
        if ((long long)groups * d >= target) break;
    }
    return ks;  // 0: K too short for a slice of 8 k-steps
}

void launch_prompt_skinny(hipStream_t s, const PromptSkinnyArgs& a, int ks) {
    FMCHECK(a.R > 0 && a.R <= 64 && a.K % 32 == 0 && ks >= 1 && (a.K / 32) % ks == 0 && a.N % 16 == 0 && a.slab &&
                a.ldx % 8 == 0 && ((uintptr_t)a.x & 15) == 0,
            "prompt skinny GEMM: R <= 64, K a multiple of 32 split evenly, N a multiple of 16, 16-B rows, slab set");
    // exactly one weight form: the bf16 fragments, the int8 codes, or the int4 codes with their (scale, zero) table
    const int wm = a.q4s ? 2 : (a.q8s ? 1 : 0);
    FMCHECK(wm == 0 ? (a.w && !a.sz) : (wm == 1 ? (!a.w && !a.sz) : (!a.w && !a.q8s && a.sz && a.K % 128 == 0)),
            "prompt skinny GEMM: one of w, q8s, or q4s with sz (K in whole 128-k units)");
    FMCHECK(!a.wscale || a.act, "prompt skinny GEMM: the row scales go with the direct SwiGLU only");
    if (wm == 2) skinny_dispatch<2>(s, a, ks);
    else if (wm == 1) skinny_dispatch<1>(s, a, ks);
    else skinny_dispatch<0>(s, a, ks);
}
