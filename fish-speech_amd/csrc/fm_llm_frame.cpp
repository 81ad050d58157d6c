// fm_llm_frame.cpp -- the launches of the Dual-AR forward: Run<T> (instantiated here only) and the
// non-template entry points the C API reaches it through.
#include <math.h>

#include <algorithm>
#include <array>

#include "fm_codec.h"
#include "fm_llm_model.h"

// ------------------------------------------------------------------------------------------
// kernels on a stack (slow or fast), templated on storage T
// ------------------------------------------------------------------------------------------
template <typename T> struct Run {
    typedef T type_t;
    fm_llm* m;
    hipStream_t s;
    int64_t E;  // element size
    // ---- the mutable state of a pass (everything else a launch needs comes from its arguments and m) ----
    // rows_distinct_slots: the rows of slow_layers are one per slot (a batched decode frame), not one prompt's
    // bs_frame: inside a batched decode frame or first frame: 8 < R <= 32 linears may run on bsacc / bstream
    // x_ss: bstream_chain only: the stack's x rows are final and m->ssX holds their tile sums
    // pend: a w2 whose fp32 K-part slabs are not yet summed into the residual rows; the next block's
    //       attention_norm launch (bs_norm_in) or flush() finalises it
    // segs: (first row, rows) of each prompt inside the current batched-prefill chunk (attention per prompt)
    bool rows_distinct_slots = false, bs_frame = false, x_ss = false;
    struct BsPending {
        bool on = false;
        const float* slab = nullptr;
        int kparts = 0, d = 0, R = 0;
        void* res = nullptr;  // residual rows (h) ...
        void* out = nullptr;  // ... + round(sum of slabs) -> out (x)
        const void* sc = nullptr;  // weight-only int8 row scales of w2
    } pend;
    std::vector<std::array<int, 2>> segs;
    void set_pending(const float* slab, int kparts, int d, int R, void* res, void* out, const void* sc) {
        pend = BsPending{true, slab, kparts, d, R, res, out, sc};
    }
    explicit Run(fm_llm* mm) : m(mm), s(mm->stream), E(sizeof(T)) {}

    // Which weight form the skinny prompt GEMM streams for W (fm_tune prompt_skinny_q): 0 the packed bf16 fragments,
    // 1 the step-granular int8 codes, 2 the int4 codes with their (scale, zero) table; -1: none (a quantised linear
    // at R > 64, which prompt_gemm asks gemm_form about instead, in fp32, under prompt_skinny_q 2, or a compact one
    // whose codes have no step-granular copy), and the caller's fallback reaches linear().  A handle with both prefers
    // the codes under 1, its bf16 copy under 0; a compact handle has only the codes.
    int skinny_form(const Linear& W, int R, int K) const {
        if (!W.q8) return 0;
        if (sizeof(T) != 2 || R > 64 || fm_tuning().prompt_skinny_q == 2) return -1;
        const int codes = W.sz ? ((W.q4s && K % 128 == 0) ? 2 : 0) : (W.q8s ? 1 : 0);
        if (codes && (!W.frag || fm_tuning().prompt_skinny_q == 1)) return codes;
        return W.frag ? 0 : -1;
    }
    // Which weight form the tiled prompt GEMMs (launch_conv_gemm) read for a quantised W at R > 64 rows (fm_tune
    // prompt_gemm_q; bf16 handles): 0 the bf16 fragment copy (int8: with the row scales in the epilogues), 1 / 2 the
    // step-granular int8 / int4 codes, -1 none -- linear(), the routing before.  A handle with the copy reads it
    // under 1, as linear() does for it, and its codes, where it has them, under 2; a compact handle has only the
    // codes and ignores 0.
    int gemm_form(const Linear& W, int K) const {
        if (sizeof(T) != 2) return -1;
        const int codes = W.sz ? ((W.q4s && K % 128 == 0) ? 2 : 0) : (W.q8s ? 1 : 0);
        if (!W.frag) return codes ? codes : -1;
        if (fm_tuning().prompt_gemm_q == 0) return -1;
        return fm_tuning().prompt_gemm_q == 2 && codes ? codes : 0;
    }
    // the skinny GEMM's weight operand of that form
    void skinny_weight(PromptSkinnyArgs& p, const Linear& W, int form) const {
        if (form == 2) {
            FMCHECK(W.q4s && W.sz, "prompt skinny GEMM: int4 linear without its step-granular codes");
            p.q4s = W.q4s;
            p.sz = W.sz;
        } else if (form == 1) {
            FMCHECK(W.q8s, "prompt skinny GEMM: int8 linear without its step-granular codes");
            p.q8s = W.q8s;
        } else {
            FMCHECK(W.frag, "prompt skinny GEMM: linear without its bf16 fragments");
            p.w = (const bf16_t*)W.frag;
        }
    }
    // Prompt chunks (R > 32 rows): a linear is a GEMM, not a weight stream, so it runs on the codec's
    // LDS-tiled implicit-GEMM kernels as a one-tap conv (conv_gemm2_kernel: 128-row x 96-128-column
    // tiles, or the 64 x 64 register tiles with split-K when the grid would not fill the chip).
    // The packed weight layout is the same; epilogues: round(acc + bias) and round(res + round(acc)).
    bool prompt_gemm(const Linear& W, const void* bias, const void* X, int ldx, int R, int N, int K, void* Y, int ldy,
                     const void* res, int ldr, int epi, const char* cls) {
        const bool tiled_q = W.q8 && R > 64;  // a quantised linear past the skinny GEMM's rows
        const int form = tiled_q ? gemm_form(W, K) : skinny_form(W, R, K);
        if (R <= 32 || form < 0 || !fm_tuning().prompt_gemm ||
            (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU8) || N % 16 || K % 32 || N < 96 ||
            (epi == EPI_SWIGLU8 && (bias || N % 16)))
            return false;
        ConvArgs<T> c{};
        c.x = (const T*)X;
        c.ldx = ldx;
        c.Ci = K;
        c.Lq = R;
        c.Lx = R;
        c.w = (const T*)W.frag;
        c.Co = N;
        c.ntaps = 1;
        c.stride = 1;
        c.nphase = 1;
        c.bias = (const T*)bias;
        c.res = epi == EPI_RESID ? (const T*)res : nullptr;
        c.ldr = ldr;
        c.out = Y;
        c.ldo = ldy;
        c.flags = CE_STORE | (bias ? CE_BIAS : 0) | (epi == EPI_RESID ? CE_RES : 0) |
                  (epi == EPI_SWIGLU8 ? CE_SWIGLU8 : 0);  // SWIGLU8: Y = act [R][N/2], ldy = N/2
        c.rscale = W.q8 ? (const T*)W.scale : nullptr;  // weight-only int8: round(round(sum) * scale) in the split-K epilogue
        hipStream_t st = s;
        const int64_t bytes = step_wbytes(form, N, K, E) + (int64_t)R * K * E + (int64_t)R * N * E;
        const double flops = 2.0 * R * N * K;
        if constexpr (sizeof(T) == 2) {
            // R <= 64: one weight pass for all rows (fm_prompt.hip), K slices finished by the conv
            // split-K epilogue (the same roundings as below)
            auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
            const int ks = prompt_skinny_ks(N, K, fm_tuning().prompt_skinny_blocks);
            if (fm_tuning().prompt_skinny && ks > 0 && R <= 64 && ldx % 8 == 0 && al16(X) && al16(Y) && ldy % 8 == 0 &&
                (!c.res || (al16(c.res) && ldr % 8 == 0)) && (long long)ks * R * N <= m->skpart_cap) {
                c.ksplit = ks;
                c.slab = m->skpart;
                c.slab_cap = (size_t)m->skpart_cap;
                PromptSkinnyArgs p{nullptr, (const bf16_t*)X, ldx, R, N, K, m->skpart};
                skinny_weight(p, W, form);
                const bool direct = ks == 1 && epi == EPI_SWIGLU8;  // the kernel stores act itself
                if (direct) {
                    p.act = (bf16_t*)Y;
                    p.lda = ldy;
                    p.wscale = (const bf16_t*)c.rscale;
                }
                auto go = [st, c, p, ks, direct] {
                    launch_prompt_skinny(st, p, ks);
                    if (!direct) launch_conv_epi<T>(st, c);
                };
                launch(cls, bytes, flops, go);
                if (form) m->prof.note("prompt_q", bytes);  // the code-streaming launches, counted apart as well
                return true;
            }
        }
        // (a quantised linear of <= 64 rows has the skinny path alone)
        if (epi == EPI_SWIGLU8 || (W.q8 && !tiled_q)) return false;  // the conv GEMMs' own epilogues have no interleaved SwiGLU
        // A quantised linear at R > 64 (fm_tune prompt_gemm_q): the same launch with the bf16 model's K-split rule,
        // on its bf16 copy (int8: rscale above, in whichever epilogue the plan runs) or on its step-granular codes,
        // from which the kernels rebuild that copy's fragments -- the same bytes out either way.
        if (tiled_q) {
            if (form == 2) {
                FMCHECK(W.q4s && W.sz, "prompt GEMM: int4 linear without its step-granular codes");
                c.w = nullptr;
                c.q4s = W.q4s;
                c.sz = W.sz;
            } else if (form == 1) {
                FMCHECK(W.q8s && W.scale, "prompt GEMM: int8 linear without its step-granular codes");
                c.w = nullptr;
                c.q8s = W.q8s;
            } else {
                FMCHECK(W.frag, "prompt GEMM: quantised linear without its bf16 fragments");
            }
        }
        // split K (fp32 slabs + the conv split-K epilogue) until the 128 x 128 tiles number >=
        // prompt_ks_tiles (default 384)
        const long long t128 = (long long)FM_CEIL(R, 128) * FM_CEIL(N, 128);
        int ks = 1;
        while (t128 * ks < fm_tuning().prompt_ks_tiles && ks < fm_tuning().prompt_ks_max && K / 32 >= 8 * ks * 2)
            ks *= 2;
        c.ksplit = ks;
        c.slab = m->skpart;
        c.slab_cap = (size_t)m->skpart_cap;
        auto go = [st, c] { launch_conv_gemm<T>(st, c); };
        launch(cls, bytes, flops, go);
        if (tiled_q) m->prof.note("prompt_gq", bytes);  // the quantised linears on the tiled route, counted apart as well
        return true;
    }
    // A prompt chunk's wo / w2 (32 < R <= 64, bf16) as raw K-slice partials in m->skpart ([ks][R][N], the
    // finalize_norm slab layout): the residual add, the bias and the next RMSNorm then run in one
    // finalize_norm launch instead of the split-K epilogue + an RMSNorm launch.  false: not eligible.
    // A weight-only int8 linear's row scales apply where the slabs' sum is rounded: scaled says the caller's
    // finisher takes them (finalize_norm's wscale); qk_rope_cache_kernel does not, so an int8 wqkv declines.
    bool prompt_slab(const Linear& W, const void* X, int ldx, int R, int N, int K, int* ks_out, bool scaled) {
        if constexpr (sizeof(T) != 2) {
            return false;
        } else {
            const int form = skinny_form(W, R, K);
            if (!fm_tuning().prompt_fin || !fm_tuning().prompt_skinny || !fm_tuning().prompt_gemm || R <= 32 ||
                R > 64 || form < 0 || (W.scale && W.q8 && !scaled) || N % 16 || K % 32 || ldx % 8 || ((uintptr_t)X & 15))
                return false;
            const int ks = prompt_skinny_ks(N, K, fm_tuning().prompt_skinny_blocks);
            if (ks <= 0 || (long long)ks * R * N > m->skpart_cap) return false;
            PromptSkinnyArgs p{nullptr, (const bf16_t*)X, ldx, R, N, K, m->skpart};
            skinny_weight(p, W, form);
            hipStream_t st = s;
            auto go = [st, p, ks] { launch_prompt_skinny(st, p, ks); };
            const int64_t bytes = step_wbytes(form, N, K, E) + (int64_t)R * K * E + (int64_t)ks * R * N * 4;
            launch("linear", bytes, 2.0 * R * N * K, go);
            if (form) m->prof.note("prompt_q", bytes);
            *ks_out = ks;
            return true;
        }
    }
    void linear(const Linear& W, const void* bias, const void* X, int ldx, int R, int N, int K, void* Y, int ldy,
                const void* res, int ldr, float* Yf, int epi, const char* cls) {
        if (bs_use(R, false) && !res && (epi == EPI_F32 || epi == EPI_STORE) &&
            bs_linear(W, bias, X, ldx, R, N, K, Y, ldy, Yf, epi))
            return;  // heads / fast_project_in of a batched frame
        if (prompt_gemm(W, bias, X, ldx, R, N, K, Y, ldy, res, ldr, epi, cls)) return;
        LinearArgs<T> a{(const T*)W.frag, nullptr, (const T*)bias, (const T*)X, ldx, R, N, K, (T*)Y,
                        ldy, (const T*)res, ldr, Yf};
        a.wscale = (const T*)W.scale;
        if (!W.frag) {  // no bf16 copy: linear_kernel's code-reading form
            FMCHECK(sizeof(T) == 2 && (epi == EPI_STORE || epi == EPI_RESID || epi == EPI_F32),
                    "compact linear: linear_kernel has no code-reading form of this launch");
            if (W.sz) {
                FMCHECK(W.q4s && K % 128 == 0, "compact int4 linear without its step-granular codes");
                a.Wq4s = W.q4s;
                a.wsz = W.sz;
            } else {
                FMCHECK(W.q8s && K % 32 == 0, "compact int8 linear without its step-granular codes");
                a.Wq8s = W.q8s;
            }
        }
        if (R > GEMV_MAX_ROWS && R <= 64) {  // batched decode: split-K over the idle CUs
            FMCHECK(m->skpart_cap >= (long long)LINEAR_PART_CAP, "split-K partial buffer too small");
            a.part = m->skpart;
            a.tickets = m->tickets;
        }
        const int64_t bytes = step_wbytes(a.Wq4s ? 2 : (a.Wq8s ? 1 : 0), N, K, E) + (int64_t)R * K * E +
                              (int64_t)R * N * (epi == EPI_F32 ? 4 : E);
        const double flops = 2.0 * R * N * K;
        hipStream_t st = s;
        auto go = [st, a, epi] { launch_linear<T>(st, a, epi); };
        launch(cls, bytes, flops, go);
    }

    // TransformerBlock.forward (llama.py:838-843) on R rows; x is updated in place.
    // ---- batched decode (8 < R <= 32 rows, one per slot) on bstream_kernel (fm_bstream.hip) ----
    // Wo and W2 leave fp32 K-part slabs; finalize_norm_kernel sums them into the residual row and
    // applies the next RMSNorm, so W2's finalise is deferred to the next block's start (or flush()).
    // slow-model decode attention: attn_dec3 (registers, 64 positions per block) for the batched
    // frame (B=32: 35.7 vs 38.1 us per layer), attn_decode2 (LDS tiles, 32-row blocks) at B <= 8,
    // where it is the faster of the two (B=1 frame 4.28 vs 4.52 ms)
    void attn_slow(const AttnDecArgs<T>& aa, int R) { attn_slow_on(s, aa, R); }
    static void attn_slow_on(hipStream_t s, const AttnDecArgs<T>& aa, int R) {
        const AttnSlowPlan p = attn_slow_plan(R, aa.hd, aa.nh / aa.nkv, aa.cap);
        if (p.kernel == 3) {
            AttnDecArgs<T> b = aa;
            b.cap = p.cap;
            b.nwb = p.nwb;
            b.hpb = p.hpb;
            launch_attn_fd<T>(s, b, R);
        } else if (p.kernel == 2)
            launch_attn_decode3<T>(s, aa, R);
        else
            launch_attn_decode2<T>(s, aa, R);
    }
    // (a compact handle runs its default routing whatever the process-wide knobs that would pick a reader of the
    // bf16 copy say -- bstream, bstream_acc, bstream_chain, bstream_q8, bstream_q4, int4_stream: fm_tune's comment)
    bool bs_use(int R, bool) const {
        return (fm_tuning().bstream || m->compact) && bs_frame && R > GEMV_MAX_ROWS && R <= 32 && m->bsA;
    }
    // one bstream linear; returns false (nothing launched) when the shape is not eligible
    // bsacc_kernel's fused prologue / epilogue operands (the batched SLABFIN / PRENORM chain)
    struct BsExtra {
        int pro = PRO_PLAIN;
        const float* ss_in = nullptr;
        const void* nw = nullptr;
        const void* res = nullptr;
        void* res_out = nullptr;
        float* ss_out = nullptr;
    };
    bool bs_linear(const Linear& W, const void* bias, const void* X, int ldx, int R, int N, int K, void* Y, int ldy,
                   float* Yf, int epi, int* kparts_out = nullptr, const BsExtra* ex = nullptr) {
        const BstreamPlan p = bstream_plan(N, K, R, epi, E, m->compact);
        if (!p.ok || ((epi == EPI_SLABFIN || (ex && ex->pro == PRO_PRENORM)) && !p.acc)) return false;
        BstreamArgs<T> a{(const T*)W.frag, (const T*)bias, (const T*)X, ldx, R, N, K, (T*)Y, ldy, Yf};
        const bool codes = !W.frag;  // no bf16 copy: only a code-streaming form will do
        a.wscale = (const T*)W.scale;
        // weight-only int8 (fm_tune bstream_q8): the accumulating kernel streams the codes where it has the form
        if (W.q8s && (fm_tuning().bstream_q8 || codes) && bsacc_q8_ok(p, epi, ex ? ex->pro : PRO_PLAIN, E)) a.Wq8 = W.q8s;
        // weight-only int4 (fm_tune bstream_q4; int4_stream 0 keeps the whole model on its dequantised weights):
        // the 4-bit codes and their (scale, zero) table
        if (W.q4s && W.sz && ((fm_tuning().bstream_q4 && fm_tuning().int4_stream) || codes) &&
            bsacc_q4_ok(p, epi, ex ? ex->pro : PRO_PLAIN, E, K)) {
            a.Wq4 = W.q4s;
            a.wsz = W.sz;
        }
        // the plan's kernel has no code instantiation: nothing launched, the caller's else branch reaches linear()
        if (codes && !a.Wq8 && !a.Wq4) return false;
        FMCHECK(a.W || a.Wq8 || (a.Wq4 && a.wsz), "bstream: no weight for the selected form");
        a.dbg = fm_tuning().dbg;
        if (ex) {
            a.pro = ex->pro;
            a.ss_in = ex->ss_in;
            a.nw = (const T*)ex->nw;
            a.eps = m->c.norm_eps;
            a.res = (const T*)ex->res;
            a.ldr = N;
            a.res_out = (T*)ex->res_out;
            a.ldro = N;
            a.ss_out = ex->ss_out;
            a.tickets = m->tickets;
        }
        const int64_t bytes = step_wbytes(a.Wq4 ? 2 : (a.Wq8 ? 1 : 0), N, K, E) + (int64_t)R * K * E +
                              (int64_t)R * N * (epi == EPI_SLAB ? 4 * p.kparts : (epi == EPI_F32 ? 4 : E));
        const double flops = 2.0 * R * N * K;
        hipStream_t st = s;
        auto go = [st, a, epi, p] { FMCHECK(launch_bstream<T>(st, a, epi, p), "bstream: no kernel for the plan"); };
        launch("linear", bytes, flops, go);
        if (kparts_out) *kparts_out = p.kparts;
        return true;
    }
    // The batched bf16 chain on bsacc_kernel (fm_tune bstream_chain): Wo and W2 finalise the residual
    // rows and their tile sums of squares (EPI_SLABFIN), QKV and W13 normalise in their prologue
    // (PRO_PRENORM) -- no finalize_norm launches.  Measured slower (B=32 frame 6.31 -> 6.75 ms): the
    // prologue's X rows and tile sums arrive ~7 us into the launch (scripts/b32_ts.py "xready"),
    // 3-4 us later than a plain prologue's, and the last K part's finalise adds 3-5 us to Wo / W2.
    bool bs_chain(const StackDims& d, int R) const {
        if (!fm_tuning().bstream_chain || m->compact || E != 2 || R > 32) return false;  // (the chain forms read bf16 tiles)
        auto ok = [&](int N, int K, int epi) { return bstream_plan(N, K, R, epi, E).acc; };
        return ok(d.nqkv(), d.dim, EPI_STORE) && ok(d.dim, d.nq(), EPI_SLABFIN) && ok(2 * d.inter, d.dim, EPI_SWIGLU8) &&
               ok(d.dim, d.inter, EPI_SLABFIN);
    }
    void finalize_norm(const float* slab, int kparts, const void* bias, const void* res, void* out, const void* nw,
                       void* xn, int d, int R, const void* sc) {
        FinalizeArgs<T> f{slab, kparts, d, (const T*)bias, (const T*)res, d, (T*)out, d, (const T*)nw,
                          m->c.norm_eps, (T*)xn, d, d, R, (const T*)sc};
        if (fm_tuning().fin_split > 1 && m->fin_cnt) {
            f.ch = fm_tuning().fin_split;
            f.cnt = m->fin_cnt;
            f.ss_part = m->fin_ss;
            f.err = m->chain_err;
        }
        run_("norm", 0, 0, [&] { launch_finalize_norm<T>(s, f); });
    }
    // finalise a W2 left pending by the last block of a stack (no norm)
    void flush() {
        if (!pend.on) return;
        pend.on = false;
        finalize_norm(pend.slab, pend.kparts, nullptr, pend.res, pend.out, nullptr, nullptr, pend.d, pend.R, pend.sc);
    }
    // the stack's input rows x are final unless a previous block left W2 pending on them
    void bs_norm_in(const StackDims& d, const LayerW& L, int R, void* xb, void* xnb) {
        if (pend.on) {
            FMCHECK(pend.out == xb && pend.R == R && pend.d == d.dim, "bstream: pending residual mismatch");
            pend.on = false;
            finalize_norm(pend.slab, pend.kparts, nullptr, pend.res, xb, L.an, xnb, d.dim, R, pend.sc);
        } else {
            run_("norm", 0, 0, [&] {
                launch_rmsnorm<T>(s, (const T*)xb, d.dim, (const T*)L.an, d.dim, m->c.norm_eps, (T*)xnb, d.dim, R);
            });
        }
    }

    // One layer of block(): its arguments and its regime.  bs: a batched frame's rows on the bsacc / bstream
    // linears (chain: their SLABFIN / PRENORM variant, fm_tune bstream_chain); else a prompt chunk (the skinny
    // GEMM's slabs where eligible) or the plain linear() fallback -- each stage tries them in that order.
    struct Blk {
        const StackDims& d;
        const LayerW& L;
        int R;
        const int *rslot, *rpos;
        int fixed_pos;
        bool is_fast;
        void *kc, *vc;
        size_t sstride, loff;
        int Sc;
        const float* rope;
        void *xb, *hb, *xnb;
        bool bs, chain;
        const float* qslab = nullptr;  // the QKV projection's K-part slabs (bs_qkv_slab, prompt_qkv_slab) instead of m->qkv
        int qslab_kp = 1;
    };
    // QKV (+ attention_norm, + the finalise of a w2 the previous block left pending)
    void blk_qkv(Blk& b) {
        const StackDims& d = b.d;
        const LayerW& L = b.L;
        const int R = b.R;
        if (b.chain && x_ss) {  // QKV normalises x itself (attention_norm from the tile sums)
            BsExtra e;
            e.pro = PRO_PRENORM;
            e.ss_in = m->ssX;
            e.nw = L.an;
            FMCHECK(bs_linear(L.wqkv, L.bqkv, b.xb, d.dim, R, d.nqkv(), d.dim, m->qkv, d.nqkv(), nullptr, EPI_STORE,
                              nullptr, &e),
                    "bsacc: no PRENORM QKV plan");
            return;
        }
        bs_norm_in(d, L, R, b.xb, b.xnb);  // (a prompt chunk's pending w2 (prompt_slab) is finalised with this norm too)
        int kp = 0;
        if (b.bs) {
            // fm_tune bs_qkv_slab: K-part slabs (a grid of whole rounds: 384 QKV tiles x 2 parts over
            // 256 CUs) summed + biased + rounded by the fused attention that reads them
            // (bsQ holds BS_KPARTS x 32 rows of either stack's width; the plan never exceeds those)
            // (only where the attention below is one of the fused kernels that read the slabs)
            const bool fused_fast = b.is_fast && b.fixed_pos >= 0 && b.fixed_pos < 16 && d.hd <= 256;
            const bool fused_slow = !b.is_fast && rows_distinct_slots && fm_tuning().attn_fd &&
                                    attn_fd_ok(d.hd, d.nh / d.nkv);
            // (weight-only int8 keeps the STORE epilogue: its row scales apply before the rounding)
            const bool slab_ok = fm_tuning().bs_qkv_slab && fm_tuning().batched_fused_attn && m->bsQ && R <= 32 &&
                                 (fused_fast || fused_slow) && !L.wqkv.q8;
            if (slab_ok && bs_linear(L.wqkv, nullptr, b.xnb, d.dim, R, d.nqkv(), d.dim, nullptr, d.nqkv(), m->bsQ,
                                     EPI_SLAB, &kp)) {
                b.qslab = m->bsQ;
                b.qslab_kp = kp;
                return;
            }
            if (bs_linear(L.wqkv, L.bqkv, b.xnb, d.dim, R, d.nqkv(), d.dim, m->qkv, d.nqkv(), nullptr, EPI_STORE)) return;
        } else if (!b.is_fast && !rows_distinct_slots && fm_tuning().prompt_qkv_slab &&
                   prompt_slab(L.wqkv, b.xnb, d.dim, R, d.nqkv(), d.dim, &kp, false)) {
            // a prompt chunk's QKV as K-slice slabs, summed by qk_rope_cache_kernel itself (no epilogue launch)
            b.qslab = m->skpart;
            b.qslab_kp = kp;
            return;
        }
        linear(L.wqkv, L.bqkv, b.xnb, d.dim, R, d.nqkv(), d.dim, m->qkv, d.nqkv(), nullptr, 0, nullptr,
               EPI_STORE, "linear");
    }
    // One row per slot (batched decode frames, every fast pass): the fused decode attention
    // kernels of the small-batch path do QK-norm, RoPE and the KV write themselves.  Prompt
    // chunks (rows of one slot, causal among themselves) keep the separate write + attention.
    void blk_attn(const Blk& b) {
        const StackDims& d = b.d;
        const LayerW& L = b.L;
        const int R = b.R;
        const float eps = m->c.norm_eps, scale = 1.0f / sqrtf((float)d.hd);
        const bool rows_are_slots = b.is_fast || rows_distinct_slots;
        hipStream_t st = s;
        if (rows_are_slots && !b.is_fast && fm_tuning().batched_fused_attn) {
            AttnDecArgs<T> aa{(const T*)m->qkv, d.nqkv(), b.rslot, b.rpos, d.nh, d.nkv, d.hd, d.qk_norm, eps,
                              (const T*)L.qn, (const T*)L.kn, b.rope, (T*)b.kc, (T*)b.vc, b.sstride, b.loff, b.Sc,
                              m->maxsplit, scale, m->part};
            aa.cap = attn2_frame_cap(d.hd, d.nh / d.nkv, E, true);
            aa.maxsplit = FM_CEIL(b.Sc, aa.cap);
            aa.cnt = m->attn_cnt;
            aa.dbg = fm_tuning().dbg;
            aa.out = (T*)m->att;
            aa.qslab = b.qslab;
            aa.qslab_kp = b.qslab_kp;
            aa.qbias = (const T*)L.bqkv;
            FMCHECK(!b.qslab || (fm_tuning().attn_fd && attn_fd_ok(d.hd, d.nh / d.nkv)), "bs_qkv_slab needs attn_fd");
            auto go = [st, aa, R] { attn_slow_on(st, aa, R); };
            m->prof.record("attn_slow", 0, go);  // the slow model's launches alone (fm_llm_kernel_bench)
            launch("attn", 0, 0, go);
        } else if (b.is_fast && fm_tuning().batched_fused_attn && b.fixed_pos >= 0 && b.fixed_pos < 16 && d.hd <= 256) {
            FastFusedArgs<T> fa{(const T*)m->qkv, d.nqkv(), b.rslot, d.nh, d.nkv, d.hd, d.qk_norm, eps,
                                (const T*)L.qn, (const T*)L.kn, b.rope, (T*)b.kc, (T*)b.vc, b.sstride, b.loff, b.Sc,
                                b.fixed_pos, scale, (T*)m->att};
            fa.dbg = fm_tuning().dbg;
            fa.qslab = b.qslab;
            fa.qslab_kp = b.qslab_kp;
            fa.qbias = (const T*)L.bqkv;
            launch("attn", 0, 0, [st, fa, R] { launch_fast_attn2<T>(st, fa, R); });
        } else {
            QkArgs<T> qa{(const T*)m->qkv, d.nqkv(), b.rslot, b.rpos, b.fixed_pos, d.nh, d.nkv, d.hd, d.qk_norm,
                         eps, (const T*)L.qn, (const T*)L.kn, b.rope, (T*)m->q, (T*)b.kc, (T*)b.vc, b.sstride, b.loff, b.Sc};
            qa.qslab = b.qslab;
            qa.qslab_kp = b.qslab_kp;
            qa.qbias = (const T*)L.bqkv;
            run_("rope", 0, 0, [&] { launch_qk_rope_cache<T>(s, qa, R); });
            if (b.is_fast) {
                FastAttnArgs<T> fa{(const T*)m->q, b.rslot, (const T*)b.kc, (const T*)b.vc, b.sstride, b.loff, b.Sc,
                                   d.nh, d.nkv, d.hd, b.fixed_pos, scale, (T*)m->att};
                run_("attn", 0, 0, [&] { launch_fast_attn<T>(s, fa, R); });
                return;
            }
            // rows [r0, r0 + len) in pieces of <= ATTN_PIECE rows (rows are independent given the cache)
            auto attn_rows = [&](int r0, int len, bool one_slot) {
                for (int p0 = r0; p0 < r0 + len; p0 += ATTN_PIECE) {
                    const int pn = std::min(ATTN_PIECE, r0 + len - p0);
                    const size_t o = (size_t)p0 * d.nh * d.hd;
                    AttnArgs<T> aa{(const T*)m->q + o, b.rslot + p0, b.rpos + p0, (const T*)b.kc, (const T*)b.vc, b.sstride,
                                   b.loff, b.Sc, d.nh, d.nkv, d.hd, ATTN_SPLIT, m->maxsplit, scale, m->part};
                    run_("attn", 0, 0, [&] { launch_attn<T>(s, aa, pn, m->maxsplit, (T*)m->att + o, one_slot); });
                }
            };
            if (!segs.empty())  // a batched prefill chunk: attention per prompt segment
                for (const auto& sg : segs) attn_rows(sg[0], sg[1], true);
            else
                attn_rows(0, R, !rows_are_slots);
        }
    }
    // h = x + wo(att), and xn = ffn_norm(h) where the next stage does not normalise itself
    void blk_wo(const Blk& b) {
        const StackDims& d = b.d;
        const LayerW& L = b.L;
        const int R = b.R;
        int kp = 0;
        if (b.chain) {
            BsExtra eo;  // finalised with its tile sums by the last K part
            eo.res = b.xb;
            eo.res_out = b.hb;
            eo.ss_out = m->ssH;
            FMCHECK(bs_linear(L.wo, L.bo, m->att, d.nq(), R, d.dim, d.nq(), nullptr, d.dim, m->bsA, EPI_SLABFIN, &kp, &eo),
                    "bsacc: no SLABFIN wo plan");
        } else if (b.bs && bs_linear(L.wo, nullptr, m->att, d.nq(), R, d.dim, d.nq(), nullptr, d.dim, m->bsA, EPI_SLAB, &kp)) {
            finalize_norm(m->bsA, kp, L.bo, b.xb, b.hb, L.fn, b.xnb, d.dim, R, L.wo.scale);
        } else if (!b.bs && prompt_slab(L.wo, m->att, d.nq(), R, d.dim, d.nq(), &kp, true)) {
            finalize_norm(m->skpart, kp, L.bo, b.xb, b.hb, L.fn, b.xnb, d.dim, R, L.wo.scale);
        } else {
            linear(L.wo, L.bo, m->att, d.nq(), R, d.dim, d.nq(), b.hb, d.dim, b.xb, d.dim, nullptr,
                   EPI_RESID, "linear");
            run_("norm", 0, 0, [&] {
                launch_rmsnorm<T>(s, (const T*)b.hb, d.dim, (const T*)L.fn, d.dim, m->c.norm_eps, (T*)b.xnb, d.dim, R);
            });
        }
    }
    // act = SwiGLU(w1 xn, w3 xn) on the row-interleaved W1 || W3
    void blk_w13(const Blk& b) {
        const StackDims& d = b.d;
        const LayerW& L = b.L;
        const int R = b.R;
        if (b.chain) {
            BsExtra e13;  // ffn_norm(h) in W1||W3's prologue
            e13.pro = PRO_PRENORM;
            e13.ss_in = m->ssH;
            e13.nw = L.fn;
            FMCHECK(bs_linear(L.w13, nullptr, b.hb, d.dim, R, 2 * d.inter, d.dim, m->act, d.inter, nullptr, EPI_SWIGLU8,
                              nullptr, &e13),
                    "bsacc: no PRENORM w13 plan");
            return;
        }
        if (b.bs && bs_linear(L.w13, nullptr, b.xnb, d.dim, R, 2 * d.inter, d.dim, m->act, d.inter, nullptr, EPI_SWIGLU8))
            return;
        // a prompt chunk's w1 || w3 with the SwiGLU in its split-K epilogue (skinny path), else the
        // stored output and the SwiGLU launch
        if (fm_tuning().prompt_swiglu && prompt_gemm(L.w13, nullptr, b.xnb, d.dim, R, 2 * d.inter, d.dim, m->act,
                                                     d.inter, nullptr, 0, EPI_SWIGLU8, "linear"))
            return;
        linear(L.w13, nullptr, b.xnb, d.dim, R, 2 * d.inter, d.dim, m->act2, 2 * d.inter, nullptr, 0, nullptr,
               EPI_STORE, "linear");
        run_("other", 0, 0,
             [&] { launch_swiglu_i8<T>(s, (const T*)m->act2, 2 * d.inter, (T*)m->act, d.inter, d.inter, R); });
    }
    // x = h + w2(act): as slabs it stays pending for the next block's norm launch (or flush())
    void blk_w2(const Blk& b) {
        const StackDims& d = b.d;
        const LayerW& L = b.L;
        const int R = b.R;
        int kp = 0;
        if (b.chain) {
            BsExtra e2;  // finalised with its tile sums
            e2.res = b.hb;
            e2.res_out = b.xb;
            e2.ss_out = m->ssX;
            FMCHECK(bs_linear(L.w2, nullptr, m->act, d.inter, R, d.dim, d.inter, nullptr, d.dim, m->bsB, EPI_SLABFIN, &kp,
                              &e2),
                    "bsacc: no SLABFIN w2 plan");
            x_ss = true;
        } else if (b.bs && bs_linear(L.w2, nullptr, m->act, d.inter, R, d.dim, d.inter, nullptr, d.dim, m->bsB, EPI_SLAB, &kp)) {
            set_pending(m->bsB, kp, d.dim, R, b.hb, b.xb, L.w2.scale);
        } else if (!b.bs && prompt_slab(L.w2, m->act, d.inter, R, d.dim, d.inter, &kp, true)) {
            set_pending(m->skpart, kp, d.dim, R, b.hb, b.xb, L.w2.scale);
        } else {
            linear(L.w2, nullptr, m->act, d.inter, R, d.dim, d.inter, b.xb, d.dim, b.hb, d.dim, nullptr,
                   EPI_RESID, "linear");
        }
    }
    // TransformerBlock.forward (llama.py:838-843) on R rows (a batched decode frame's, or a prompt chunk's);
    // x is updated in place
    void block(const StackDims& d, const LayerW& L, int R, const int* rslot, const int* rpos,
               int fixed_pos, bool is_fast, void* kc, void* vc, size_t sstride, size_t loff, int Sc,
               const float* rope, void* xb, void* hb, void* xnb) {
        const bool bs = bs_use(R, is_fast);
        Blk b{d, L, R, rslot, rpos, fixed_pos, is_fast, kc, vc, sstride, loff, Sc, rope, xb, hb, xnb, bs, bs && bs_chain(d, R)};
        blk_qkv(b);
        blk_attn(b);
        blk_wo(b);
        blk_w13(b);
        blk_w2(b);
    }

    // ---------------- small-batch (<= 8 streams) fused path --------------------------------
    GemvArgs<T> ga() {
        GemvArgs<T> a{};
        a.eps = m->c.norm_eps;
        a.dummy_tail = fm_tuning().gemv_dummy;
        return a;
    }
    // ---- batch-1 GEMV chain: consecutive GEMVs of one row are deferred and launched together
    // (gemv_chain_kernel), up to GEMV_CHAIN_MAX per launch; any other launch flushes them first
    struct ChainSt {
        const Linear* W;
        GemvArgs<T> a;
        int kind;
        int64_t bytes;
        double flops;
    };
    std::vector<ChainSt> chain;
    int chain_kind(const Linear& W, const GemvArgs<T>& a, int pro, int epi, int ksb) const {
        const FmTuning& t = fm_tuning();
        if (!t.gemv_chain || m->prof.on || ksb != 1 || a.R != 1 || W.q8 || !t.gemv_nt ||
            t.gemv_u != 8 || t.gemv_wpb != 4 || a.N % 16 || a.xidx)
            return -1;
        if (pro == PRO_PLAIN && epi == EPI_SLABFIN) return GEMV_CHAIN_WO_W2;
        if (a.xn_out || a.K > 4096 || pro != PRO_PRENORM) return a.xn_out && pro == PRO_PRENORM && epi == EPI_F32 &&
                                                                    a.K <= 4096 ? GEMV_CHAIN_HEAD : -1;
        if (epi == EPI_SWIGLU8) return GEMV_CHAIN_W13;
        if (epi == EPI_STORE) return GEMV_CHAIN_QKV;
        if (epi == EPI_F32) return GEMV_CHAIN_HEAD;
        return -1;
    }
    void chain_flush() {
        if (chain.empty()) return;
        std::vector<ChainSt> c;
        c.swap(chain);
        if (c.size() == 1) {
            static const int pro_of[4] = {PRO_PLAIN, PRO_PRENORM, PRO_PRENORM, PRO_PRENORM};
            static const int epi_of[4] = {EPI_SLABFIN, EPI_SWIGLU8, EPI_STORE, EPI_F32};
            gemv_now(*c[0].W, c[0].a, pro_of[c[0].kind], epi_of[c[0].kind], 1, "linear");
            return;
        }
        GemvChainArgs<T> g{};
        int64_t bytes = 0;
        double flops = 0;
        g.n = (int)c.size();
        for (int i = 0; i < g.n; ++i) {
            g.st[i] = c[i].a;
            if (!g.st[i].tickets) g.st[i].tickets = m->tickets;
            g.kind[i] = c[i].kind;
            bytes += c[i].bytes;
            flops += c[i].flops;
        }
        g.cnt = m->chain_cnt;
        g.err = m->chain_err;
        g.sleep = fm_tuning().chain_sleep;
        hipStream_t st = s;
        auto go = [st, g] { launch_gemv_chain<T>(st, g); };
        launch("linear", bytes, flops, go);
    }
    // One decode GEMV of the linear W on the 16-row tile kernel; a carries everything but the weight.
    void gemv(const Linear& W, GemvArgs<T> a, int pro, int epi, int ksb, const char* cls, int tile0 = 0) {
        const int kind = chain_kind(W, a, pro, epi, ksb);
        if (kind < 0 || tile0) {
            chain_flush();
            gemv_now(W, a, pro, epi, ksb, cls, tile0);
            return;
        }
        a.W = (const T*)W.frag;  // (chain_kind: not a quantised linear)
        const int64_t bytes = gemv_wbytes(0, a.N, a.K, E) + (int64_t)a.K * E;
        chain.push_back(ChainSt{&W, a, kind, bytes, 2.0 * a.N * a.K});
        if ((int)chain.size() >= std::min(GEMV_CHAIN_MAX, fm_tuning().chain_max) || kind == GEMV_CHAIN_HEAD)
            chain_flush();
    }
    // tile0 (fm_tune fast_dead_q bit 1; weight-only int8, whole K, STORE): the launch covers the 16-row tiles from
    // tile0 on -- rows [16 tile0, N) of the same linear: the kernel's tile b is the weight's tile tile0 + b (a
    // tile's codes are contiguous), so the codes, the row scales, the bias and Y move by the same rows and N
    // shrinks; the tiles are independent, every output row is the full launch's
    void gemv_now(const Linear& W, GemvArgs<T> a, int pro, int epi, int ksb, const char* cls, int tile0 = 0) {
        // the form: the code units where the linear has them (an int4 handle on its dequantised bf16 weights under
        // int4_stream 0 apart); a compact linear has nothing else
        const int form = W.q8 && (!W.sz || fm_tuning().int4_stream || !W.frag) ? (W.sz ? 2 : 1) : 0;
        FMCHECK(W.frag || (W.q8 && (W.sz || W.scale) && epi != EPI_SWIGLU), "compact linear without its decode-GEMV codes");
        a.W = (const T*)W.frag;
        if (tile0) {
            const int r0 = 16 * tile0;
            FMCHECK(form == 1 && ksb == 1 && epi == EPI_STORE && a.R == 1 && a.Y && tile0 > 0 && r0 < a.N && a.N % 16 == 0,
                    "GEMV from a tile offset: weight-only int8, whole K, one stored row");
            a.Y += r0;
            if (a.bias) a.bias += r0;
            a.N -= r0;
        }
        if (form == 2) {  // weight-only int4: 4-bit codes + group (scale, zero), whole 128-k units per slice
            a.Wq = W.q8;
            a.wsz = W.sz;
            a.wscale = nullptr;
            while (ksb > 1 && (a.K / ksb) % 128) ksb /= 2;
        } else if (form == 1) {  // weight-only int8: the int8 stream, whole 64-k units per slice
            a.Wq = W.q8 + (size_t)tile0 * 16 * a.K;
            a.wscale = (const T*)W.scale + 16 * tile0;
            while (ksb > 1 && (a.K / ksb) % 64) ksb /= 2;
        }
        const int64_t bytes = gemv_wbytes(form, a.N, a.K, E) + (int64_t)a.R * a.K * E;
        const double flops = 2.0 * a.R * a.N * a.K;
        hipStream_t st = s;
        if (!a.tickets) a.tickets = m->tickets;
        auto go = [st, a, pro, epi, ksb] { launch_gemv<T>(st, a, pro, epi, ksb); };
        launch(cls, bytes, flops, go);
    }
    // batch-1 bf16 wo / w2 on the row-block GEMV (fm_rowgemv.hip: one block per pair of rows, every
    // CU busy); their RMSNorm consumers then take the statistic from the row they stage (ss_gran 1)
    // the row-block GEMV's enabled linears (fm_tune rowgemv; int4 models: rowgemv_q4)
    int row_bits() const {
        const FmTuning& t = fm_tuning();
        return m->quant == FM_QUANT_INT4 ? t.rowgemv_q4 : t.rowgemv;
    }
    bool row_fin(int n) const {
        const FmTuning& t = fm_tuning();
        return sizeof(T) == 2 && n == 1 && m->row_ok && (row_bits() & 1) && !t.gemv_chain && !t.attn_wo &&
               m->streams_codes();
    }
    // ... and wqkv (norm prologue, 8 rows per block)
    bool row_qkv(int n) const {
        const FmTuning& t = fm_tuning();
        // (int8: the tile kernel's wqkv measured as fast, 3.12 vs 3.14 ms per frame)
        return sizeof(T) == 2 && n == 1 && m->row_qkv_ok && m->quant != FM_QUANT_INT8 && (row_bits() & 2) &&
               !t.gemv_chain && m->streams_codes();
    }
    // ... and w1 || w3 (norm prologue, SwiGLU epilogue, 4 + 4 rows per block)
    bool row_w13(int n) const {
        const FmTuning& t = fm_tuning();
        return sizeof(T) == 2 && n == 1 && m->row_w13_ok && (row_bits() & 4) && !t.gemv_chain &&
               m->streams_codes();
    }
    // the row-block GEMV's weight: bf16 row-major, or the int8 codes + row scales, or the int4 code words + group
    // (scale, zero) rows
    void row_weight(RowGemvArgs& r, const Linear& W) {
        FMCHECK(W.rm, "row GEMV: the linear has no row-major copy");
        if (m->quant == FM_QUANT_INT4) {
            r.Wq4 = (const uint32_t*)W.rm;
            r.wsz = W.rm_sz;
            r.gs = m->q4_gs;
        } else if (m->quant) {
            r.Wq = (const int8_t*)W.rm;
            r.wscale = (const bf16_t*)W.rm_scale;
        } else {
            r.W = (const bf16_t*)W.rm;
        }
    }
    // ... from its row row0 on (K columns): the rows, and with them the int4 code words and (scale, zero) rows or the
    // int8 codes and row scales, start row0 rows in; the caller moves bias, Y and N
    static void row_weight_from(RowGemvArgs& r, int row0, int K) {
        if (r.Wq4) {
            r.Wq4 += (size_t)row0 * (K / 8);
            r.wsz += (size_t)row0 * (K / r.gs);
        } else if (r.Wq) {
            r.Wq += (size_t)row0 * K;
            r.wscale += row0;
        } else {
            r.W += (size_t)row0 * K;
        }
    }
    static int64_t rowgemv_wbytes(const RowGemvArgs& a) { return row_wbytes(a.Wq4 ? 2 : (a.Wq ? 1 : 0), a.N, a.K, a.gs); }
    // the residual a wo GEMV adds: the layer's input row itself for a stack's first layer (a table row gathered
    // by xidx[xcol] at codebook > 0), else the residual row xb
    void row_residual(RowGemvArgs& r, bool first, const void* x_in, int ldx_in, const int32_t* xidx, int xcol,
                      const void* xb, int dim) {
        r.res = (const bf16_t*)(first ? x_in : xb);
        r.ldr = first ? ldx_in : dim;
        if (first) {
            r.residx = xidx;
            r.res_col = xcol;
            r.res_rows = xidx ? m->cb : 0;
        }
    }
    // KV prefetch operands of a QKV GEMV (GemvArgs / RowGemvArgs pf_*): the cached rows 0 .. *pos of *slot
    template <typename A, typename P>
    static void kv_prefetch(A& a, const P* kc, const P* vc, const int32_t* slot, const int32_t* pos, size_t slot_stride,
                            size_t layer_off, int S, int nkv, int hd) {
        a.pf_kc = kc;
        a.pf_vc = vc;
        a.pf_slot = slot;
        a.pf_pos = pos;
        a.pf_slot_stride = slot_stride;
        a.pf_layer_off = layer_off;
        a.pf_S = S;
        a.pf_nkv = nkv;
        a.pf_hd = hd;
    }
    void rowgemv(const RowGemvArgs& a, int kind) {
        hipStream_t st = s;
        auto go = [st, a, kind] { launch_rowgemv(st, a, kind); };
        launch("linear", rowgemv_wbytes(a) + (int64_t)a.K * 2, 2.0 * a.N * a.K, go);
    }
    template <typename F> void run_(const char* cls, int64_t bytes, double flops, F&& f) {
        chain_flush();
        m->prof.run(s, cls, bytes, flops, std::forward<F>(f));
    }
    // run one launch and record it for fm_llm_kernel_bench (under rec where that class differs from the
    // profiler's): `go` must capture by value (it is replayed later).  Pending chain GEMVs go first.
    template <typename F> void launch(const char* cls, int64_t bytes, double flops, const F& go, const char* rec = nullptr) {
        chain_flush();
        m->prof.record(rec ? rec : cls, bytes, go);
        m->prof.run(s, cls, bytes, flops, go);
    }
    struct KsbPlan {
        int wo, w2;
    };
    // wo / w2 finalise the residual rows (EPI_SLABFIN): whole K per block (local finalise, no
    // cross-block hand-off) whenever the x slice fits the LDS budget, else split K
    KsbPlan plan(const StackDims& d, int n) {
        auto fin_ksb = [&](int N, int K) {
            const int fk = fm_tuning().fin_ksb;  // developer override (split-K factor)
            if (fk > 0 && K % (32 * fk) == 0) return fk;
            // (splitting K further to fill more CUs measured slower at B = 1: 4.37 -> 4.74 ms per
            // frame at 320 blocks, the split-K hand-off costs more than the idle CUs)
            return gemv_lds_bytes(n, K, E) <= 120 * 1024 ? 1 : pick_ksb(N, K, n, E);
        };
        return KsbPlan{fin_ksb(d.dim, d.nq()), fin_ksb(d.dim, d.inter)};
    }
    // a layer's QKV projection (+ attention_norm) of one row on the row-block GEMV.  first: x is the layer's
    // input row itself (a table row gathered by xidx[xcol] when xidx), else the residual row xb.  a: the tile
    // form's arguments, whose KV prefetch fields carry over.  kv_rows (fm_tune rowgemv bit 6): rows [nq, nqkv)
    // only -- the same prologue and the same per-row sums, the Q rows of Y left as they were
    // two (fm_tune fast_pair): x and Y hold two rows; one launch, row 0's Q rows left out (RowGemvArgs::skip0)
    void qkv_row(const StackDims& d, const LayerW& L, const GemvArgs<T>& a, bool first, const void* x, int ldx,
                 const int32_t* xidx, int xcol, void* Y, bool kv_rows, bool two = false) {
        RowGemvArgs r{};
        row_weight(r, L.wqkv);  // (bf16 or int4: row_qkv excludes int8 models)
        r.X = (const bf16_t*)x;
        if (first) {
            r.ldx = ldx;
            r.xidx = xidx;
            r.xcol = xcol;
            r.xrows = xidx ? m->cb : 0;
        }
        r.bias = (const bf16_t*)L.bqkv;
        r.nw = (const bf16_t*)L.an;
        r.eps = m->c.norm_eps;
        r.Y = (bf16_t*)Y;
        r.N = d.nqkv();
        r.K = d.dim;
        if (two) {
            r.xr = 2;
            r.X1 = r.X + d.dim;
            r.Y1 = r.Y + d.nqkv();
            r.skip0 = d.nq();
        }
        if (kv_rows) {
            row_weight_from(r, d.nq(), d.dim);
            if (r.bias) r.bias += d.nq();
            r.Y += d.nq();
            r.N -= d.nq();
        }
        kv_prefetch(r, (const bf16_t*)a.pf_kc, (const bf16_t*)a.pf_vc, a.pf_slot, a.pf_pos, a.pf_slot_stride, a.pf_layer_off,
                    a.pf_S, a.pf_nkv, a.pf_hd);
        rowgemv(r, ROWGEMV_NORM_STORE);
    }
    bool qkv_first_row(int n) const { return row_qkv(n) && (row_bits() & 16); }
    // the FIRST layer's QKV of one row: the row form (rowgemv bits 1 and 4), else the PRO_NORM tile form.
    // block_small's launch, and -- one launch per code, xidx an iota array, Y the code's table row -- what
    // ensure_qkv0 fills the bit-5 table with: the same kernel on the same input row gives the same bytes
    void qkv_first(const StackDims& d, const LayerW& L, GemvArgs<T> a, int n, const void* x_in, int ldx_in,
                   const int32_t* xidx, int xcol, void* Y, bool kv_rows) {
        if (qkv_first_row(n)) {
            qkv_row(d, L, a, true, x_in, ldx_in, xidx, xcol, Y, kv_rows);
            return;
        }
        a.Y = (T*)Y;
        a.X = (const T*)x_in;
        a.ldx = ldx_in;
        a.xidx = xidx;
        a.xidx_ld = m->C1;
        a.xidx_col = xcol;
        a.xidx_rows = xidx ? m->cb : 0;
        // (kv_rows on the tile form: weight-only int8 only, small_path; the tiles from nq / 16 on)
        gemv(L.wqkv, a, PRO_NORM, EPI_STORE, 1, "linear", kv_rows ? d.nq() / 16 : 0);
    }
    // the tile form's arguments of a fast layer's QKV at one row, no prefetch (the table build)
    GemvArgs<T> qkv_args(const StackDims& d, const LayerW& L, int n) {
        GemvArgs<T> a = ga();
        a.bias = (const T*)L.bqkv;
        a.nw = (const T*)L.an;
        a.R = n;
        a.N = d.nqkv();
        a.K = d.dim;
        a.Y = (T*)m->qkv;
        a.ldy = d.nqkv();
        return a;
    }
    // fm_tune fast_dead_q's bits in force: weight-only int8 / int4 handles whose fast stack has no o-bias (the
    // quantised linears carry no bias, finalize; a model configured with one stays on the launches it has)
    static int dead_q_bits(const fm_llm* m) { return m->quant && !m->fdm.o_bias ? fm_tuning().fast_dead_q : 0; }
    // whether block_small may read the first fast layer's QKV from the table (bf16 compute: rowgemv bit 5 on
    // unquantised weights, fast_dead_q bit 0 on quantised ones)
    bool qkv0_live() const {
        return sizeof(T) == 2 && (m->quant ? (dead_q_bits(m) & 1) : (row_bits() & 32)) && m->qkv0 && m->qkv0_built &&
               m->qkv0_epoch == fm_tuning().epoch;
    }

    // One layer of block_small: its arguments ...
    // x_in: the first layer's input (plain rows, or an embedding table + xidx gather), whose norm is computed in
    // place.  xo: where W2 writes the block's output row (xb itself unless the chain alternates buffers)
    struct Small {
        const StackDims& d;
        const LayerW& L;
        int n;
        bool first;
        const void* x_in;
        int ldx_in;
        const int32_t* xidx;
        int xcol;
        void *xb, *hb;
        bool is_fast;
        int cpos, layer;
        KsbPlan kp;
        void* xo;
        // fm_tune fast_pair: codebook positions 0 and 1 as one two-row pass.  Row 0's input is x_in (the plain hidden
        // row), row 1's the row of x_in1 gathered by xidx[xcol]; cpos is row 1's position; row 1 of every activation
        // buffer follows row 0.  1: both rows run the layer; 2 (the last layer): row 0 ends at its K / V cache write
        // inside the fused launch, and wo, w1 || w3 and w2 run on row 1 alone
        int pair = 0;
        const void* x_in1 = nullptr;
    };
    // row 1 of a pair's buffer (w elements per row); the buffer itself outside the pair's last layer
    static const void* row1(const Small& c, const void* p, int w) {
        return (const char*)p + (c.pair == 2 ? (size_t)w * sizeof(T) : 0);
    }
    static void* row1(const Small& c, void* p, int w) { return (char*)p + (c.pair == 2 ? (size_t)w * sizeof(T) : 0); }
    // ... and the kernel path of each of its stages, chosen once (small_path)
    struct SmallPath {
        bool rf;        // wo / w2 on the row-block GEMV; their RMSNorm consumers take the statistic from the row they stage
        bool fw;        // fast model: attention + wo as one launch (fattn_wo_kernel), no attention launch
        bool att_wo;    // fast model: attention recomputed in the wo tile GEMV's prologue (PRO_FATT), no attention launch
        bool row_here;  // this layer's QKV on the row-block GEMV (a stack's first layer: only with rowgemv bit 4)
        bool tab;       // rowgemv bit 5 / fast_dead_q bit 0: the first fast layer at codebook > 0 inside fw: its q|k|v row comes from the table, no QKV launch
        bool kv0;       // rowgemv bit 6 / fast_dead_q bit 1: codebook 0: only K / V are projected (row path; int8: the tile path) and the attention reads no Q (one position: output = v)
        bool kv0_ok;    // weight-only handles: the K / V-only forms fast_dead_q bit 1 uses exist at this layer's shape (whether or not the bit is set)
        bool kv_only;   // the layer ends after its K / V cache write (fm_tune fast_tail: its output would be discarded)
        bool sw;        // slow model: attention + wo as one launch (slow_attn_wo_kernel), no attention launch (fm_tune slow_attn_wo / slow_attn_wo_q)
    };
    // fm_tune slow_attn_wo: one bf16 unquantised row of the slow stack whose attention is attn_fd at 8 waves and one q
    // head per block and whose wo runs on the row-block GEMV (so gemv_chain is off), at instantiated shapes; two layers
    // at least, so that consecutive writers of the tagged words always differ in tag, and at most 40 (the tag's
    // launch indices).  Anywhere else the layer keeps its two launches.
    // fm_tune slow_attn_wo_q: the same on weight-only int8 / int4 handles (compact ones too: the row GEMV's row-major
    // codes are not what compact frees), wo's row blocks on the codes with their row scales / group (scale, zero) rows;
    // a layer with an o-bias keeps its two launches (the code forms take none).  Each knob is inert on the other's handles.
    int slow_attn_wo_knob() const { return m->quant ? fm_tuning().slow_attn_wo_q : fm_tuning().slow_attn_wo; }
    bool slow_attn_wo_live(const Small& c, bool rf) const {
        const StackDims& d = c.d;
        const int qm = m->qmode();
        const Linear& wo = c.L.wo;
        const bool form = qm == 2 ? wo.rm_sz && !c.L.bo : (qm == 1 ? wo.rm_scale && !c.L.bo : !m->quant && !wo.rm_scale && !wo.rm_sz);
        if (!(sizeof(T) == 2 && !c.is_fast && c.n == 1 && rf && form && slow_attn_wo_knob() && m->sxt &&
              !fm_tuning().gemv_chain && d.n_layer >= 2 && d.n_layer <= 40))
            return false;
        const AttnSlowPlan ap = attn_slow_plan(1, d.hd, d.nh / d.nkv, attn2_frame_cap(d.hd, d.nh / d.nkv, E, false));
        return ap.kernel == 3 && ap.nwb == 8 && ap.hpb == 1 && slow_attn_wo_ok(d.nh, d.nkv, d.hd, d.dim, d.nq(), qm);
    }
    SmallPath small_path(const Small& c, bool kv_only) const {
        const StackDims& d = c.d;
        SmallPath p{};
        p.kv_only = kv_only;
        p.rf = row_fin(c.n);
        p.sw = !kv_only && slow_attn_wo_live(c, p.rf);
        const int fq = m->qmode();
        // (fw_any: the fused launch is this layer's form, whether or not this pass ends before it)
        const bool fw_any = c.is_fast && p.rf && fm_tuning().fattn_wo && m->fxt && m->fdm.n_layer * m->C >= 2 &&
                            m->fdm.n_layer * m->C <= 40 && fattn_wo_ok(d.nh, d.nkv, d.hd, c.cpos, d.dim, d.nq(), fq);
        p.fw = fw_any && !kv_only;
        // (fm_tune attn_wo; measured slower, kept under test)
        p.att_wo = c.is_fast && !kv_only && fm_tuning().attn_wo && !m->quant && c.n == 1 && c.cpos < 16 && d.hd % 16 == 0 &&
                   d.hd <= 128 && d.nh % d.nkv == 0 && (d.nq() / c.kp.wo) % d.hd == 0 && d.nqkv() % 8 == 0;
        p.row_here = row_qkv(c.n) && (!c.first || (row_bits() & 16));
        // bits 5 / 6: bf16, unquantised, batch 1; inert elsewhere (with kv0 the Q part of m->qkv is stale)
        const bool bits56 = sizeof(T) == 2 && !m->quant && c.is_fast && c.n == 1;
        // fm_tune fast_dead_q: the same two forms on weight-only int8 / int4 handles, only where the fused launch is
        // the layer's form and its table / K-V-only instantiation is one that stays resident (fattn_wo_dead_ok).
        // K / V only: int4 on the row form as bf16 (8 rows per block), int8 on the tile form from tile nq / 16
        const bool dqf = sizeof(T) == 2 && c.is_fast && c.n == 1 && fw_any && fattn_wo_dead_ok(d.nq(), fq);
        const int dq = dqf ? dead_q_bits(m) : 0;
        p.tab = (bits56 || (dq & 1)) && c.first && c.xidx && p.fw && qkv0_live();
        p.kv0 = bits56 && c.cpos == 0 && (row_bits() & 64) && p.row_here && !p.att_wo && d.hd <= 256 &&
                (d.nqkv() - d.nq()) % fm_tuning().row_qkv_rp == 0;
        p.kv0_ok = dqf && m->quant && !m->fdm.o_bias && c.cpos == 0 && !p.att_wo && d.hd <= 256 &&
                   (m->quant == FM_QUANT_INT4
                        ? p.row_here && (d.nqkv() - d.nq()) % fm_tuning().row_qkv_rp == 0 && (d.nqkv() - d.nq()) % 8 == 0
                        : !p.row_here && d.nq() % 16 == 0 && d.nqkv() % 16 == 0);
        if ((dq & 2) && c.cpos == 0 && !p.att_wo && d.hd <= 256) p.kv0 = p.kv0_ok;
        return p;
    }
    // the fast model's attention operands at this layer (the attention launch, fattn_wo, PRO_FATT)
    FastFusedArgs<T> small_fast_args(const Small& c, const SmallPath& p) const {
        const StackDims& d = c.d;
        FastFusedArgs<T> fa{(const T*)m->qkv, d.nqkv(), m->frame_slot, d.nh, d.nkv, d.hd, d.qk_norm,
                            m->c.norm_eps, (const T*)c.L.qn, (const T*)c.L.kn, m->frope, (T*)m->fkc,
                            (T*)m->fvc, m->fslot_stride, (size_t)c.layer * m->flayer_stride, m->C, c.cpos,
                            1.0f / sqrtf((float)d.hd), (T*)m->att};
        fa.dbg = fm_tuning().dbg;
        fa.noq = p.kv0;
        return fa;
    }
    // QKV (+ attention_norm)
    void small_qkv(const Small& c, const SmallPath& p) {
        if (p.tab && !c.pair) return;
        const StackDims& d = c.d;
        GemvArgs<T> a = qkv_args(d, c.L, c.n);
        if (!c.is_fast && c.n == 1 && fm_tuning().kv_prefetch)  // the attention's K / V rows into L2
            kv_prefetch(a, (const T*)m->kc, (const T*)m->vc, m->frame_slot, m->frame_pos, m->slot_stride,
                        (size_t)c.layer * m->layer_stride, m->S, d.nkv, d.hd);
        else if (c.is_fast && c.n == 1 && fm_tuning().fkv_prefetch && m->fiota && c.cpos < 16)
            // the fast attention's cached rows 0 .. cpos - 1 (fiota[cpos] = cpos - 1)
            kv_prefetch(a, (const T*)m->fkc, (const T*)m->fvc, m->frame_slot, m->fiota + c.cpos, m->fslot_stride,
                        (size_t)c.layer * m->flayer_stride, m->C, d.nkv, d.hd);
        if (c.first) {  // the layer's input row itself (a table row gathered by xidx[xcol] at codebook > 0)
            // (a pair: row 0's K / V rows, codebook 0's launch as it stands; row 1's row is the table's)
            qkv_first(d, c.L, a, c.n, c.x_in, c.ldx_in, c.pair ? nullptr : c.xidx, c.pair ? 0 : c.xcol, m->qkv,
                      p.kv0 || c.pair);
        } else if (p.row_here) {
            qkv_row(d, c.L, a, false, c.xb, 0, nullptr, 0, m->qkv, p.kv0, c.pair != 0);
        } else {
            a.X = (const T*)c.xb;
            a.ldx = d.dim;
            a.ss_in = m->ssX;
            a.ss_gran = p.rf ? 1 : 0;
            // (fm_tune fast_pair_q, int8: both rows through the whole wqkv -- row 0's Q outputs are stored and never read;
            // its K / V tiles are what the one-row launch from tile nq / 16 computes)
            if (c.pair) a.R = 2;
            gemv(c.L.wqkv, a, PRO_PRENORM, EPI_STORE, 1, "linear", p.kv0 ? d.nq() / 16 : 0);  // (kv0 here: weight-only int8)
        }
    }
    // attention launch (none where wo does it: fw, att_wo)
    // the slow model's decode attention operands at this layer (the attention launch, slow_attn_wo)
    AttnDecArgs<T> small_slow_args(const Small& c) const {
        const StackDims& d = c.d;
        AttnDecArgs<T> aa{(const T*)m->qkv, d.nqkv(), m->frame_slot, m->frame_pos, d.nh, d.nkv, d.hd,
                          d.qk_norm, m->c.norm_eps, (const T*)c.L.qn, (const T*)c.L.kn, m->rope, (T*)m->kc,
                          (T*)m->vc, m->slot_stride, (size_t)c.layer * m->layer_stride, m->S,
                          m->maxsplit, 1.0f / sqrtf((float)d.hd), m->part};
        aa.cap = attn2_frame_cap(d.hd, d.nh / d.nkv, E, false);
        aa.maxsplit = FM_CEIL(m->S, aa.cap);
        aa.cnt = m->attn_cnt;
        aa.dbg = fm_tuning().dbg;
        aa.out = (T*)m->att;
        return aa;
    }
    void small_attn(const Small& c, const SmallPath& p) {
        const StackDims& d = c.d;
        const int n = c.n;
        hipStream_t st = s;
        if (p.sw) return;
        if (!c.is_fast) {
            const AttnDecArgs<T> aa = small_slow_args(c);
            auto go = [st, aa, n] { attn_slow_on(st, aa, n); };
            m->prof.record("attn_slow", 0, go);  // the slow model's launches alone (fm_llm_kernel_bench)
            launch("attn", 0, 0, go);
        } else if (!p.att_wo && !p.fw) {
            const FastFusedArgs<T> fa = small_fast_args(c, p);
            const bool f2 = c.cpos < 16 && d.hd <= 256;
            launch("attn", 0, 0, [st, fa, n, f2] {
                if (f2)
                    launch_fast_attn2<T>(st, fa, n);
                else
                    launch_fast_attn_fused<T>(st, fa, n);
            });
        }
    }
    // wo: h = x + wo(att) (tile form: split-K, the last block of each tile finalises h and its sums of squares)
    void small_wo(const Small& c, const SmallPath& p) {
        const StackDims& d = c.d;
        const LayerW& L = c.L;
        if (p.fw || p.rf) {
            FattnWoArgs A{};
            RowGemvArgs& r = A.wo;
            row_weight(r, L.wo);
            r.X = (const bf16_t*)m->att;  // (fw: unused, x comes from the tagged words)
            r.bias = (const bf16_t*)L.bo;
            if (!c.pair) {
                row_residual(r, c.first, c.x_in, c.ldx_in, c.xidx, c.xcol, c.xb, d.dim);
                r.res_out = (bf16_t*)c.hb;
            } else {  // row 1's residual: its gathered input row at the first layer, else row 1 of xb
                RowGemvArgs r1{};
                row_residual(r1, c.first, c.x_in1, c.ldx_in, c.xidx, c.xcol, (const bf16_t*)c.xb + d.dim, d.dim);
                r.ldr = r1.ldr;
                r.residx = r1.residx;
                r.res_col = r1.res_col;
                r.res_rows = r1.res_rows;
                if (c.pair == 2) {
                    r.res = r1.res;
                    r.res_out = (bf16_t*)c.hb + d.dim;
                } else {
                    r.xr = 2;
                    r.res = (const bf16_t*)(c.first ? c.x_in : c.xb);
                    r.res1 = r1.res;
                    r.res_out = (bf16_t*)c.hb;
                    r.res_out1 = (bf16_t*)c.hb + d.dim;
                }
            }
            r.N = d.dim;
            r.K = d.nq();
            if (p.sw) {  // the slow attention blocks and wo's row blocks as one launch
                SlowAttnWoArgs W{};
                if constexpr (sizeof(T) == 2) {  // (p.sw is a bf16 frame's only: slow_attn_wo_live)
                    W.at = small_slow_args(c);
                    W.at.cap = attn_slow_plan(1, d.hd, d.nh / d.nkv, W.at.cap).cap;
                }
                W.wo = r;
                W.xt = m->sxt;
                // <= 40 (slow_attn_wo_live).  Consecutive launches of one stream always differ in tag.  A first layer
                // follows the last layer of the frame before it, which may be another slot's: the two tags meet only
                // where 41 (p' - p) = n_layer - 1 (mod 65535) -- S2-Pro's 36 layers: slots 15985 positions apart, past
                // any max_seq_len here; 25 layers: 1599 apart (the fast launches' formula has the same property)
                W.gen = 1 + c.layer;
                W.err = m->chain_err;
                W.rp = slow_attn_wo_knob() == 2 ? 4 : 2;
                W.delay_pct = fm_tuning().slow_aw_delay;
                W.sleep = fm_tuning().slow_aw_sleep;
                W.cheap = fm_tuning().slow_aw_cheap;
                hipStream_t st = s;
                auto go = [st, W] { launch_slow_attn_wo(st, W); };
                // a class of its own (attention + GEMV), booked with wo's weight bytes; the code forms in theirs
                launch(m->quant ? "slow_attn_wo_q" : "slow_attn_wo", rowgemv_wbytes(r), 2.0 * r.N * r.K, go);
                return;
            }
            if (!p.fw) {
                rowgemv(r, ROWGEMV_FIN);
                return;
            }
            const FastFusedArgs<T> fa = small_fast_args(c, p);
            A.at = *reinterpret_cast<const FastFusedArgs<bf16_t>*>(&fa);
            A.at.dbg = nullptr;
            A.at.row_pos = m->frame_pos;
            A.xt = m->fxt;
            A.gen = 1 + c.layer + m->fdm.n_layer * c.cpos;  // <= 40 (fattn_wo_ok: cpos < 16, n_layer * C checked)
            A.err = m->chain_err;
            A.delay = fm_tuning().fw_delay;
            A.cheap = fm_tuning().fw_cheap;
            A.prio = fm_tuning().fw_prio;
            A.ilp = fm_tuning().fattn_ilp;
            if (p.tab) {
                A.qtab = (const bf16_t*)m->qkv0;
                A.qidx = c.xidx;
                A.qcol = c.xcol;
                A.qrows = m->cb;
            }
            A.kv0 = p.kv0;
            A.pair = c.pair;
            hipStream_t st = s;
            auto go = [st, A] { launch_fattn_wo(st, A); };
            // (recorded as "attn_wo", not "linear": attention + GEMV, reported apart)
            launch("attn", rowgemv_wbytes(r), 2.0 * r.N * r.K, go, "attn_wo");
            return;
        }
        GemvArgs<T> a = ga();
        a.bias = (const T*)L.bo;
        a.X = (const T*)m->att;
        a.ldx = d.nq();
        a.R = c.n;
        a.N = d.dim;
        a.K = d.nq();
        a.Yf = m->slabA;
        a.ldy = d.dim;
        if (c.first) {
            a.res = (const T*)c.x_in;
            a.ldr = c.ldx_in;
            a.residx = c.xidx;
            a.xidx_ld = m->C1;
            a.xidx_col = c.xcol;
            a.xidx_rows = c.xidx ? m->cb : 0;
        } else {
            a.res = (const T*)c.xb;
            a.ldr = d.dim;
        }
        a.res_out = (T*)c.hb;
        a.ldro = d.dim;
        a.ss_out = m->ssH;
        a.tickets = m->tickets;
        if (p.att_wo) a.att = small_fast_args(c, p);
        gemv(L.wo, a, p.att_wo ? PRO_FATT : PRO_PLAIN, EPI_SLABFIN, c.kp.wo, "linear");
    }
    // W1 || W3 (+ ffn_norm) -> SwiGLU act
    void small_w13(const Small& c, const SmallPath& p) {
        const StackDims& d = c.d;
        if (row_w13(c.n)) {
            RowGemvArgs r{};
            row_weight(r, c.L.w13);
            r.X = (const bf16_t*)row1(c, c.hb, d.dim);
            r.nw = (const bf16_t*)c.L.fn;
            r.eps = m->c.norm_eps;
            r.Y = (bf16_t*)row1(c, m->act, d.inter);
            r.N = 2 * d.inter;
            r.K = d.dim;
            if (c.pair == 1) {  // (fm_tune fast_pair_q, int4: the two-row form; the pair's last layer runs row 1 alone)
                r.xr = 2;
                r.X1 = r.X + d.dim;
                r.Y1 = r.Y + d.inter;
            }
            rowgemv(r, ROWGEMV_NORM_SWIGLU);
            return;
        }
        GemvArgs<T> a = ga();
        a.nw = (const T*)c.L.fn;
        a.R = c.pair == 1 ? 2 : c.n;  // (a pair's two rows: the ss_gran 1 prologue's two-row instantiation)
        a.N = 2 * d.inter;
        a.K = d.dim;
        a.X = (const T*)row1(c, c.hb, d.dim);
        a.ldx = d.dim;
        a.ss_in = m->ssH;
        a.ss_gran = p.rf ? 1 : 0;
        a.Y = (T*)row1(c, m->act, d.inter);
        a.ldy = d.inter;
        gemv(c.L.w13, a, PRO_PRENORM, EPI_SWIGLU8, 1, "linear");
    }
    // W2: the block output x = h + w2(act) into xo (tile form: split-K, finalised with its sums of squares)
    void small_w2(const Small& c, const SmallPath& p) {
        const StackDims& d = c.d;
        if (p.rf) {
            RowGemvArgs r{};
            row_weight(r, c.L.w2);
            r.X = (const bf16_t*)row1(c, m->act, d.inter);
            r.res = (const bf16_t*)row1(c, c.hb, d.dim);
            r.ldr = d.dim;
            r.res_out = (bf16_t*)row1(c, c.xo, d.dim);
            if (c.pair == 1) {
                r.xr = 2;
                r.X1 = r.X + d.inter;
                r.res1 = r.res + d.dim;
                r.res_out1 = r.res_out + d.dim;
            }
            r.N = d.dim;
            r.K = d.inter;
            rowgemv(r, ROWGEMV_FIN);
            return;
        }
        GemvArgs<T> a = ga();
        a.X = (const T*)m->act;
        a.ldx = d.inter;
        a.R = c.n;
        a.N = d.dim;
        a.K = d.inter;
        a.Yf = m->slabB;
        a.ldy = d.dim;
        a.res = (const T*)c.hb;
        a.ldr = d.dim;
        a.res_out = (T*)c.xo;
        a.ldro = d.dim;
        a.ss_out = m->ssX;
        a.tickets = m->tickets;
        gemv(c.L.w2, a, PRO_PLAIN, EPI_SLABFIN, c.kp.w2, "linear");
    }
    // one pre-norm block (TransformerBlock.forward, llama.py:838-843) on n <= 8 rows.  Residual rows
    // are always finalised by the producing GEMV (EPI_SLABFIN: x / h in bf16 plus per-tile sums of
    // squares ssX / ssH), so every RMSNorm consumer is PRO_PRENORM.
    void block_small(const StackDims& d, const LayerW& L, int n, bool first, const void* x_in, int ldx_in,
                     const int32_t* xidx, int xcol, void* xb, void* hb, bool is_fast, int cpos, int layer,
                     const KsbPlan& kp, void* xo, bool kv_only = false, int pair = 0, const void* x_in1 = nullptr) {
        const Small c{d, L, n, first, x_in, ldx_in, xidx, xcol, xb, hb, is_fast, cpos, layer, kp, xo, pair, x_in1};
        const SmallPath p = small_path(c, kv_only);
        small_qkv(c, p);
        small_attn(c, p);
        if (p.kv_only) return;  // the attention wrote the K / V rows at cpos, all a later launch reads
        small_wo(c, p);
        small_w13(c, p);
        small_w2(c, p);
    }

    // the residual row of layer l: x (in place) or, in chain mode, x / x2 alternating
    void* xbuf(void* x0, void* x1, int l) const { return (fm_tuning().gemv_chain && (l & 1)) ? x1 : x0; }
    void* xfin = nullptr;  // the slow stack's output row (head_small's input when pending)
    void slow_small(int n) {
        const KsbPlan kp = plan(m->sd, n);
        for (int l = 0; l < m->sd.n_layer; ++l)
            block_small(m->sd, m->slow[l], n, l == 0, m->x, m->c.dim, nullptr, 0, xbuf(m->x, m->x2, l), m->h, false, 0,
                        l, kp, xbuf(m->x, m->x2, l + 1));
        xfin = xbuf(m->x, m->x2, m->sd.n_layer);
    }

    // final norm (+ pending residual) -> constrained head logits and the fast-model hidden
    const void* head_small(const void* xlast, bool pending, int n, int ksb_prev) {
        const fm_model_config& c = m->c;
        GemvArgs<T> a = ga();
        a.nw = (const T*)m->norm;
        a.R = n;
        a.N = m->Nhead;
        a.K = c.dim;
        a.Yf = m->logits;
        a.ldy = m->Nhead;
        a.xn_out = (T*)m->xnl;
        a.ldxo = c.dim;
        const void* xs = xfin ? xfin : m->x;
        if (pending) {  // the last slow layer's W2 finalised x (xs) and its sums of squares
            a.X = (const T*)xs;
            a.ldx = c.dim;
            a.ss_in = m->ssX;
            a.ss_gran = row_fin(n) ? 1 : 0;
            gemv(m->head_c, a, PRO_PRENORM, EPI_F32, 1, "linear");
        } else {
            a.X = (const T*)xlast;
            a.ldx = c.dim;
            gemv(m->head_c, a, PRO_NORM, EPI_F32, 1, "linear");
        }
        const void* hid = c.norm_fastlayer_input ? m->xnl : (pending ? xs : xlast);
        if (m->fproj_w) {
            GemvArgs<T> p = ga();
            p.bias = (const T*)m->fproj_b;
            p.X = (const T*)hid;
            p.ldx = c.dim;
            p.R = n;
            p.N = c.fast_dim;
            p.K = c.dim;
            p.Y = (T*)m->xl;
            p.ldy = c.fast_dim;
            gemv(m->fproj_w, p, PRO_PLAIN, EPI_STORE, 1, "linear");
            return m->xl;
        }
        return hid;
    }

    void fast_small(int n, int cc, bool with_head, const void* hidden) {
        const fm_model_config& c = m->c;
        const KsbPlan kp = plan(m->fdm, n);
        for (int l = 0; l < m->fdm.n_layer; ++l) {
            const bool first = l == 0;
            const void* xin = cc == 0 ? hidden : m->femb;
            const int32_t* xidx = cc == 0 ? nullptr : m->cols;
            // codebook 0's pass (no head: inference.py:148-149 discards its output) only fills the fast
            // KV cache, so its last layer stops once its K / V rows are cached (fm_tune fast_tail)
            const bool kv_only = !with_head && l == m->fdm.n_layer - 1 && fm_tuning().fast_tail;
            block_small(m->fdm, m->fast[l], n, first, xin, c.fast_dim, xidx, cc, xbuf(m->fx, m->fx2, l), m->fh, true,
                        cc, l, kp, xbuf(m->fx, m->fx2, l + 1), kv_only);
        }
        if (with_head) fast_head(n, xbuf(m->fx, m->fx2, m->fdm.n_layer));
    }
    // the codebook head on the fast stack's output row(s) x
    void fast_head(int n, const void* x) {
        const fm_model_config& c = m->c;
        if (sizeof(T) == 2 && n == 1 && m->fout.rm && (row_bits() & 8) && !fm_tuning().gemv_chain &&
            m->streams_codes()) {
            RowGemvArgs r{};  // the codebook head on the row-block GEMV (norm prologue, fp32 logits)
            row_weight(r, m->fout);
            r.X = (const bf16_t*)x;
            r.nw = (const bf16_t*)m->fnorm;
            r.eps = c.norm_eps;
            r.Yf = m->flogits;
            r.N = m->cb;
            r.K = c.fast_dim;
            rowgemv(r, ROWGEMV_NORM_F32);
        } else {
            GemvArgs<T> a = ga();
            a.nw = (const T*)m->fnorm;
            a.R = n;
            a.N = m->cb;
            a.K = c.fast_dim;
            a.Yf = m->flogits;
            a.ldy = m->cb;
            a.X = (const T*)x;
            a.ldx = c.fast_dim;
            a.ss_in = m->ssX;
            a.ss_gran = row_fin(n) ? 1 : 0;
            gemv(m->fout, a, PRO_PRENORM, EPI_F32, 1, "linear");
        }
    }

    // fm_tune fast_pair: whether codebook positions 0 and 1 run as one two-row pass.  Both input rows are known when
    // the fast passes start (the slow model's hidden row; fast_embeddings[cols[1]], drawn by the slow sampler) and row 1
    // needs of row 0 only its K / V per layer, so the pair is a causal two-token pass that reads every weight once.
    // It stands on bf16 unquantised weights at one row, fast_tail, the fused attention + wo of every layer at position
    // 1, the QKV table (rowgemv bit 5) and codebook 0's K / V-only form (bit 6) -- so bits 0 and 1 too -- w1 || w3 on
    // the tile kernel, and two-row kernel forms that exist at these depths; anywhere else the one-row passes run
    bool fast_pair_live(int n) const {
        const FmTuning& t = fm_tuning();
        const StackDims& d = m->fdm;
        if (m->quant) return fast_pair_q_live(n);  // (fast_pair itself is inert on weight-only handles)
        // (two fast layers at least: consecutive writers of the pair's row-1 tagged words then always differ in tag)
        if (!(sizeof(T) == 2 && !m->quant && n == 1 && m->C >= 2 && d.n_layer >= 2 && t.fast_pair && t.fast_tail && !t.gemv_chain &&
              !row_w13(n) && d.dim <= 4096 && rowgemv_pair_ok(-1, d.nq(), false) && rowgemv_pair_ok(ROWGEMV_FIN, d.nq(), true) &&
              rowgemv_pair_ok(ROWGEMV_FIN, d.inter, false) && rowgemv_pair_ok(ROWGEMV_NORM_STORE, d.dim, false)))
            return false;
        const KsbPlan kp{1, 1};
        for (int l = 0; l < d.n_layer; ++l) {
            const Small c0{d, m->fast[l], n, l == 0, nullptr, 0, nullptr, 0, nullptr, nullptr, true, 0, l, kp, nullptr};
            const Small c1{d, m->fast[l], n, l == 0, nullptr, 0, m->cols, 1, nullptr, nullptr, true, 1, l, kp, nullptr};
            const SmallPath p0 = small_path(c0, false), p1 = small_path(c1, false);
            if (!(p0.kv0 && p1.fw && p1.rf && !p1.att_wo && (l == 0 ? p1.tab : p1.row_here))) return false;
        }
        return true;
    }
    // fm_tune fast_pair_q: the same pass on a weight-only handle (a compact one too: the row-major codes and the GEMV
    // units are not what compact frees), bf16 compute, on the default routing of each mode.  Bit 0, int8: wo and w2 on the
    // row-block GEMV, wqkv and w1 || w3 on the tile kernel under ss_gran 1 (its two-row prologue stages K <= 4096).  Bit
    // 1, int4: every linear on the row-block GEMV (rowgemv_q4 bits 0, 1, 2 and 4 -- the first layer's K / V rows come
    // from its row form) streaming the codes.  Both: a fast stack without an o-bias, the QKV table (fast_dead_q bit 0)
    // live, the fused launch every layer's form at position 1, codebook 0's K / V-only launch available at the shape
    // (the forms of fast_dead_q bit 1, whether or not that bit is set) and two-row forms instantiated at the model's
    // depths.  Anywhere else the one-row passes run.
    bool fast_pair_q_live(int n) const {
        const FmTuning& t = fm_tuning();
        const StackDims& d = m->fdm;
        const int qm = m->qmode();
        if (!(sizeof(T) == 2 && qm && (t.fast_pair_q & qm) && n == 1 && m->C >= 2 && d.n_layer >= 2 && t.fast_tail &&
              !t.gemv_chain && !d.o_bias && row_fin(n) && rowgemv_pair_ok(-1, d.nq(), false, qm) &&
              rowgemv_pair_ok(ROWGEMV_FIN, d.nq(), true, qm) && rowgemv_pair_ok(ROWGEMV_FIN, d.inter, false, qm)))
            return false;
        if (qm == 2 ? !((row_bits() & 23) == 23 && row_qkv(n) && row_w13(n) && rowgemv_pair_ok(ROWGEMV_NORM_STORE, d.dim, false, qm) &&
                        rowgemv_pair_ok(ROWGEMV_NORM_SWIGLU, d.dim, false, qm))
                    : !(!row_qkv(n) && !row_w13(n) && d.dim <= 4096 && d.dim % 64 == 0 && t.q_u <= 8))  // (q_u 16: no two-row SwiGLU8 form)
            return false;
        const KsbPlan kp{1, 1};
        for (int l = 0; l < d.n_layer; ++l) {
            const Small c0{d, m->fast[l], n, l == 0, nullptr, 0, nullptr, 0, nullptr, nullptr, true, 0, l, kp, nullptr};
            const Small c1{d, m->fast[l], n, l == 0, nullptr, 0, m->cols, 1, nullptr, nullptr, true, 1, l, kp, nullptr};
            const SmallPath p0 = small_path(c0, false), p1 = small_path(c1, false);
            if (!(p0.kv0_ok && p1.fw && p1.rf && !p1.att_wo && (l == 0 ? p1.tab : p1.row_here == (qm == 2)))) return false;
        }
        return true;
    }
    // codebook positions 0 and 1 as one pass, and codebook 1's head (on row 1 of the stack's output)
    void fast_pair(const void* hidden) {
        const fm_model_config& c = m->c;
        const KsbPlan kp = plan(m->fdm, 1);
        const int nl = m->fdm.n_layer;
        for (int l = 0; l < nl; ++l)
            block_small(m->fdm, m->fast[l], 1, l == 0, hidden, c.fast_dim, m->cols, 1, m->fx, m->fh, true, 1, l, kp, m->fx,
                        false, l == nl - 1 ? 2 : 1, m->femb);
        fast_head(1, (const char*)m->fx + (size_t)c.fast_dim * sizeof(T));
    }
    // codebook 0's pass (it only fills the fast KV cache; logits discarded) and, where the pair engages, codebook 1's
    // with its head in the same pass: returns the next codebook to run
    int fast_open(int n, const void* hidden) {
        if (fast_pair_live(n)) {
            fast_pair(hidden);
            return 2;
        }
        fast_small(n, 0, false, hidden);
        return 1;
    }

    void frame_tail_small(int n, bool ras_enable, bool sample, const void* hidden) {
        if (sample) {
            SampleArgs a = sargs(true, ras_enable, 0);
            run_("sample", 0, 0, [&] { launch_sample_radix<T>(s, a, n); });
        }
        int cc = fast_open(n, hidden);
        if (cc == 2 && sample) {
            SampleArgs a = sargs(false, 0, 1);
            run_("sample", 0, 0, [&] { launch_sample_radix<T>(s, a, n); });
        }
        for (; cc < m->C; ++cc) {
            fast_small(n, cc, true, hidden);
            if (sample) {
                SampleArgs a = sargs(false, 0, cc);
                run_("sample", 0, 0, [&] { launch_sample_radix<T>(s, a, n); });
            }
        }
    }

    void decode_frame_small(int n) {
        run_("other", 0, 0, [&] {
            launch_embed<T>(s, m->tok_in, n, (const T*)m->emb, (const T*)m->cbemb, m->c.dim, m->C, m->cb,
                            m->c.semantic_begin_id, m->c.semantic_end_id, m->c.scale_codebook_embeddings,
                            (T*)m->x, m->frame_slot);
        });
        slow_small(n);
        const KsbPlan kp = plan(m->sd, n);
        const void* hid = head_small(nullptr, true, n, kp.w2);
        frame_tail_small(n, true, true, hid);
        chain_flush();
        launch_finish(s, n, m->frame_slot, m->frame_pos, m->cols, m->C1, m->tok_in, m->ras, m->C1 * 10, m->C1,
                      1, m->sp);
    }

    void slow_layers(int R, const int* rslot, const int* rpos) {
        x_ss = false;
        for (int l = 0; l < m->sd.n_layer; ++l)
            block(m->sd, m->slow[l], R, rslot, rpos, -1, false, m->kc, m->vc, m->slot_stride,
                  (size_t)l * m->layer_stride, m->S, m->rope, m->x, m->h, m->xn);
        flush();
    }

    // final norm -> constrained head logits; hidden for the fast model (llama.py:447-466, 826)
    void head_and_hidden(const void* xlast, int n) {
        const fm_model_config& c = m->c;
        chain_flush();
        run_("norm", 0, 0, [&] {
            launch_rmsnorm<T>(s, (const T*)xlast, c.dim, (const T*)m->norm, c.dim, c.norm_eps, (T*)m->xnl,
                              c.dim, n);
        });
        linear(m->head_c, nullptr, m->xnl, c.dim, n, m->Nhead, c.dim, nullptr, m->Nhead,
               nullptr, 0, m->logits, EPI_F32, "linear");
        const void* src = c.norm_fastlayer_input ? m->xnl : xlast;
        if (m->fproj_w)
            linear(m->fproj_w, m->fproj_b, src, c.dim, n, c.fast_dim, c.dim, m->fx, c.fast_dim,
                   nullptr, 0, nullptr, EPI_STORE, "linear");
        else
            HIPCHK(hipMemcpyAsync(m->fx, src, (size_t)n * c.dim * E, hipMemcpyDeviceToDevice, s));
    }

    void fast_pass(int n, int cpos, bool with_head) {
        const fm_model_config& c = m->c;
        x_ss = false;
        for (int l = 0; l < m->fdm.n_layer; ++l)
            block(m->fdm, m->fast[l], n, m->frame_slot, nullptr, cpos, true, m->fkc, m->fvc,
                  m->fslot_stride, (size_t)l * m->flayer_stride, m->C, m->frope, m->fx, m->fh, m->fxn);
        flush();
        if (with_head) {
            run_("norm", 0, 0, [&] {
                launch_rmsnorm<T>(s, (const T*)m->fx, c.fast_dim, (const T*)m->fnorm, c.fast_dim,
                                  c.norm_eps, (T*)m->fxn, c.fast_dim, n);
            });
            linear(m->fout, nullptr, m->fxn, c.fast_dim, n, m->cb, c.fast_dim, nullptr, m->cb,
                   nullptr, 0, m->flogits, EPI_F32, "linear");
        }
    }

    SampleArgs sargs(bool slow, int ras_enable, int c) {
        const fm_model_config& cc = m->c;
        SampleArgs a{};
        a.logits = slow ? m->logits : m->flogits;
        a.ldl = slow ? m->Nhead : m->cb;
        a.Nl = a.ldl;
        a.row_slot = m->frame_slot;
        a.sp = m->sp;
        a.ras = m->ras;
        a.ras_stride = m->C1 * 10;
        a.ras_enable = ras_enable;
        a.slow = slow;
        a.sb = cc.semantic_begin_id;
        a.se = cc.semantic_end_id;
        a.im_end = cc.im_end_id;
        a.cb = m->cb;
        a.draw = 1 + c;
        a.col_idx = c + 1;
        a.cols = m->cols;
        a.ldc = m->C1;
        a.dbg = fm_tuning().dbg;
        a.force_cols = m->force_cols;
        a.tap = slow ? m->tap_slow : m->tap_fast + (size_t)(c - 1) * m->cb;
        a.tap_ld = slow ? m->Nhead : (m->C - 1) * m->cb;
        return a;
    }

    // tail of decode_one_token_ar after the slow forward: sample, fast AR over codebooks
    void frame_tail(int n, bool ras_enable, bool sample) {
        if (sample) {
            SampleArgs a = sargs(true, ras_enable, 0);
            run_("sample", 0, 0, [&] { launch_sample_radix<T>(s, a, n); });
        }
        fast_pass(n, 0, false);  // position 0: fills the fast KV cache, logits discarded
        for (int cc = 1; cc < m->C; ++cc) {
            run_("other", 0, 0, [&] {
                launch_gather_rows<T>(s, m->cols, m->C1, cc, (const T*)m->femb, m->c.fast_dim, m->cb, n, (T*)m->fx);
            });
            fast_pass(n, cc, true);
            if (sample) {
                SampleArgs a = sargs(false, 0, cc);
                run_("sample", 0, 0, [&] { launch_sample_radix<T>(s, a, n); });
            }
        }
    }

    void decode_frame(int n) {
        if (n <= GEMV_MAX_ROWS) {
            decode_frame_small(n);
            return;
        }
        run_("other", 0, 0, [&] {
            launch_embed<T>(s, m->tok_in, n, (const T*)m->emb, (const T*)m->cbemb, m->c.dim, m->C, m->cb,
                            m->c.semantic_begin_id, m->c.semantic_end_id, m->c.scale_codebook_embeddings,
                            (T*)m->x, m->frame_slot);
        });
        rows_distinct_slots = true;
        bs_frame = true;
        slow_layers(n, m->frame_slot, m->frame_pos);
        rows_distinct_slots = false;
        head_and_hidden(m->x, n);
        frame_tail(n, true, true);
        bs_frame = false;
        chain_flush();
        launch_finish(s, n, m->frame_slot, m->frame_pos, m->cols, m->C1, m->tok_in, m->ras, m->C1 * 10,
                      m->C1, 1, m->sp);
    }

    // runs the prompt through the slow model (chunks), leaves the last row in m->x[row]
    const void* prefill_slow(int slot, const int32_t* tokens, int Tn, int pos0) {
        const int C1 = m->C1;
        std::vector<int32_t> rows((size_t)PREFILL_CHUNK * C1);
        std::vector<int> rs(PREFILL_CHUNK, slot), rp(PREFILL_CHUNK);
        int last = 0;
        for (int t0 = 0; t0 < Tn; t0 += PREFILL_CHUNK) {
            const int R = std::min(PREFILL_CHUNK, Tn - t0);
            for (int r = 0; r < R; ++r) {
                for (int q = 0; q < C1; ++q) rows[(size_t)r * C1 + q] = tokens[(size_t)q * Tn + t0 + r];
                rp[r] = pos0 + t0 + r;
            }
            chain_flush();
            HIPCHK(hipMemcpyAsync(m->ptok, rows.data(), (size_t)R * C1 * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(m->prow_slot, rs.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(m->prow_pos, rp.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
            launch_embed<T>(s, m->ptok, R, (const T*)m->emb, (const T*)m->cbemb, m->c.dim, m->C, m->cb,
                            m->c.semantic_begin_id, m->c.semantic_end_id, m->c.scale_codebook_embeddings,
                            (T*)m->x, nullptr);
            slow_layers(R, m->prow_slot, m->prow_pos);
            last = R - 1;
            HIPCHK(hipStreamSynchronize(s));  // host vectors reused by the next chunk
        }
        return (const char*)m->x + (size_t)last * m->c.dim * E;
    }

    // Several prompts (one slot each, positions from pos0[i], or from 0) through the slow stack together: their rows
    // packed into PREFILL_CHUNK-row chunks, so every linear is one GEMM over all of them (a prompt
    // may span chunks: its earlier rows are in the KV cache by then); the attention runs per prompt
    // segment (segs); the last row of prompt i is copied to plast row i.
    void prefill_multi(int n, const int32_t* slots, const int32_t* const* toks, const int* Ts, const int* pos0) {
        const int C1 = m->C1, dim = m->c.dim;
        std::vector<int32_t> rows((size_t)PREFILL_CHUNK * C1);
        std::vector<int> rs(PREFILL_CHUNK), rp(PREFILL_CHUNK);
        int i = 0, t = 0;  // next (prompt, position) to place
        while (i < n) {
            int R = 0;
            segs.clear();
            std::vector<std::array<int, 2>> lasts;  // (prompt, row) of prompts ending in this chunk
            while (R < PREFILL_CHUNK && i < n) {
                const int take = std::min(PREFILL_CHUNK - R, Ts[i] - t);
                segs.push_back({R, take});
                for (int r = 0; r < take; ++r) {
                    for (int q = 0; q < C1; ++q) rows[(size_t)(R + r) * C1 + q] = toks[i][(size_t)q * Ts[i] + t + r];
                    rs[R + r] = slots[i];
                    rp[R + r] = (pos0 ? pos0[i] : 0) + t + r;
                }
                R += take;
                t += take;
                if (t == Ts[i]) {
                    lasts.push_back({i, R - 1});
                    ++i;
                    t = 0;
                }
            }
            chain_flush();
            HIPCHK(hipMemcpyAsync(m->ptok, rows.data(), (size_t)R * C1 * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(m->prow_slot, rs.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(m->prow_pos, rp.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
            launch_embed<T>(s, m->ptok, R, (const T*)m->emb, (const T*)m->cbemb, dim, m->C, m->cb,
                            m->c.semantic_begin_id, m->c.semantic_end_id, m->c.scale_codebook_embeddings,
                            (T*)m->x, nullptr);
            slow_layers(R, m->prow_slot, m->prow_pos);
            chain_flush();
            for (const auto& l : lasts)
                HIPCHK(hipMemcpyAsync((char*)m->plast + (size_t)l[0] * dim * E, (const char*)m->x + (size_t)l[1] * dim * E,
                                      (size_t)dim * E, hipMemcpyDeviceToDevice, s));
            segs.clear();
            HIPCHK(hipStreamSynchronize(s));  // host vectors reused by the next chunk
        }
    }
};

template <typename F> static int with_prec(fm_llm* m, F&& f) {
    if (m->prec == FM_PREC_BF16) {
        Run<bf16_t> r(m);
        f(r);
        r.chain_flush();
    } else {
        Run<float> r(m);
        f(r);
        r.chain_flush();
    }
    return 0;
}

// fm_tune rowgemv bit 5: (re)build the table of the first fast layer's raw q|k|v rows, one launch of
// block_small's own first-layer QKV helper per code (Run::qkv_first: the kernel the frame would run, on
// the row fast_embeddings[code]), so the table holds the bytes that launch would have written.  Built at
// load time and again whenever an fm_tune call since could have changed the helper's kernel (the tuning
// epoch); never inside a capture.  Weight-only int8 / int4 handles build it the same way under fm_tune fast_dead_q
// bit 0 (int8: the PRO_NORM tile kernel on the int8 stream; int4: the row form with the gather), where the fused
// launch can run at all (row-major wo / w2 copies; int4: int4_stream).
void ensure_qkv0(fm_llm* m) {
    FmTuning& t = fm_tuning();
    const bool want = m->quant ? (Run<bf16_t>::dead_q_bits(m) & 1) && m->row_ok && m->streams_codes()
                               : (t.rowgemv & 32) != 0;
    if (!m->finalized || m->prec != FM_PREC_BF16 || !want || !m->fxt || m->C < 2 || !t.fattn_wo || t.gemv_chain ||
        m->fast.empty())
        return;
    if (m->qkv0_built && m->qkv0_epoch == t.epoch) return;
    const StackDims& d = m->fdm;
    if (!m->qkv0) {
        m->mem_cat = 4;  // fm_llm_memory_info: the table is a weight
        m->qkv0 = m->dalloc((size_t)m->cb * d.nqkv() * sizeof(bf16_t), false);
        m->mem_cat = 6;
        std::vector<int32_t> io((size_t)m->cb);
        for (size_t i = 0; i < io.size(); ++i) io[i] = (int32_t)i;
        m->qkv0_iota = (int32_t*)m->dalloc(io.size() * sizeof(int32_t), false);
        HIPCHK(hipMemcpy(m->qkv0_iota, io.data(), io.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // the build's launches are neither profiled nor recorded (debug_ts, fm_llm_profile)
    unsigned long long* dbg = t.dbg;
    const bool prof_on = m->prof.on;
    t.dbg = nullptr;
    m->prof.on = false;
    try {
        Run<bf16_t> r(m);
        const GemvArgs<bf16_t> a = r.qkv_args(d, m->fast[0], 1);
        for (int code = 0; code < m->cb; ++code)
            r.qkv_first(d, m->fast[0], a, 1, m->femb, m->c.fast_dim, m->qkv0_iota, code,
                        (bf16_t*)m->qkv0 + (size_t)code * d.nqkv(), false);
        r.chain_flush();
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
    } catch (...) {
        t.dbg = dbg;
        m->prof.on = prof_on;
        throw;
    }
    t.dbg = dbg;
    m->prof.on = prof_on;
    m->qkv0_epoch = t.epoch;
    m->qkv0_built = true;
}

// one decode frame for the uploaded rows (graph replay when enabled), async
void launch_frame(fm_llm* m, int n) {
    ensure_qkv0(m);
    if (m->use_graph && !m->prof.on) {
        auto it = m->graphs.find(n);
        if (it == m->graphs.end()) {
            hipGraph_t g;
            HIPCHK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
            with_prec(m, [&](auto& r) { r.decode_frame(n); });
            HIPCHK(hipStreamEndCapture(m->stream, &g));
            hipGraphExec_t ge;
            HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
            HIPCHK(hipGraphDestroy(g));
            it = m->graphs.emplace(n, ge).first;
        }
        HIPCHK(hipGraphLaunch(it->second, m->stream));
    } else {
        with_prec(m, [&](auto& r) { r.decode_frame(n); });
    }
}

void decode_frame_eager(fm_llm* m, int n) {
    with_prec(m, [&](auto& r) { r.decode_frame(n); });
}

void prefill_frame(fm_llm* m, int slot, const int32_t* tokens, int T, int pos0) {
    ensure_qkv0(m);
    with_prec(m, [&](auto& r) {
        const void* last = r.prefill_slow(slot, tokens, T, pos0);
        const void* hid = r.head_small(last, false, 1, 1);
        r.frame_tail_small(1, false, true, hid);
    });
}

void prefill_batch_frame(fm_llm* m, int n, const int32_t* slots, const int32_t* const* toks, const int32_t* T,
                         const int32_t* pos0) {
    ensure_qkv0(m);
    with_prec(m, [&](auto& r) {
        r.prefill_multi(n, slots, toks, T, pos0);
        if (n <= GEMV_MAX_ROWS) {
            const void* hid = r.head_small(m->plast, false, n, 1);
            r.frame_tail_small(n, false, true, hid);
        } else {
            r.bs_frame = true;
            r.head_and_hidden(m->plast, n);
            r.frame_tail(n, false, true);
            r.bs_frame = false;
        }
    });
}

void teacher_frame(fm_llm* m, int slot, const int32_t* x, int S, int pos0, const int32_t* next_col, float* lg,
                   float* hidden, float* fast_logits) {
    const fm_model_config& c = m->c;
    ensure_qkv0(m);
    with_prec(m, [&](auto& r) {
        const void* last = r.prefill_slow(slot, x, S, pos0);
        const void* hid = r.head_small(last, false, 1, 1);
        HIPCHK(hipMemcpyAsync(lg, m->logits, (size_t)m->Nhead * 4, hipMemcpyDeviceToHost, m->stream));
        if (hidden) {
            std::vector<uint8_t> hb((size_t)c.fast_dim * m->esz);
            HIPCHK(hipMemcpyAsync(hb.data(), hid, hb.size(), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));
            for (int i = 0; i < c.fast_dim; ++i) {
                if (m->esz == 2) {
                    uint32_t u = ((uint32_t)((uint16_t*)hb.data())[i]) << 16;
                    memcpy(&hidden[i], &u, 4);
                } else {
                    hidden[i] = ((float*)hb.data())[i];
                }
            }
        }
        if (next_col) {
            HIPCHK(hipMemcpyAsync(m->cols, next_col, (size_t)m->C1 * 4, hipMemcpyHostToDevice, m->stream));
            const int c0 = r.fast_open(1, hid);
            if (c0 == 2 && fast_logits)
                HIPCHK(hipMemcpyAsync(fast_logits, m->flogits, (size_t)m->cb * 4, hipMemcpyDeviceToHost, m->stream));
            for (int cc = c0; cc < m->C; ++cc) {
                r.fast_small(1, cc, true, hid);
                if (fast_logits)
                    HIPCHK(hipMemcpyAsync(fast_logits + (size_t)(cc - 1) * m->cb, m->flogits, (size_t)m->cb * 4,
                                          hipMemcpyDeviceToHost, m->stream));
            }
        }
    });
}
