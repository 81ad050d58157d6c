// fm_codec_ops.cpp -- per-op test hooks of the codec kernels (include/fishmi.h, "codec per-op hooks").
//
// Each hook runs ONE production launcher of fm_codec_kernels.hip on caller operands, prepared by the
// functions the model itself calls (fm_codec_prep.h), so tests/test_gpu_codec_ops.py can hold every
// output element to a float64 reference.  Conventions as fm_ops.cpp's: fp32 host arrays converted to
// the precision's storage type, every output in/out (what the kernel leaves alone comes back as the
// caller filled it), FM_ERR_ARG for a shape a launcher refuses.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fm_codec.h"
#include "fm_codec_prep.h"
#include "fm_kernels.h"
#include "fm_ops_util.h"
#include "fm_runtime.h"

using namespace fm_ops_util;

namespace {

constexpr size_t SLAB_GUARD = 4096;          // floats behind the split-K workspace
constexpr uint32_t GUARD_WORD = 0x7fc5a5a5u;  // a NaN no partial sum produces

template <typename T> std::vector<T> snapshot(const T* d, size_t n, hipStream_t s) {
    std::vector<T> h(n);
    if (!n) return h;
    HIPCHK(hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return h;
}
// words of an output that a repeated launch on the same scratch left different
template <typename T> int count_diff(const T* d, const std::vector<T>& first, hipStream_t s) {
    const std::vector<T> h = snapshot(d, first.size(), s);
    int n = 0;
    for (size_t i = 0; i < h.size(); ++i) n += memcmp(&h[i], &first[i], sizeof(T)) != 0;
    return n;
}

// `reps` launches on the same scratch (an in-place kernel gets the caller's values again before each): the
// output words the later launches left different from the first one's
template <typename T, typename F> int run_reps(DevBufs& b, InOut<T>& o, int reps, bool inplace, F&& launch) {
    std::vector<T> first;
    for (int i = 0; i < reps; ++i) {
        if (i && inplace) o.refill(b);
        launch();
        HIPCHK(hipGetLastError());
        if (i == 0 && reps > 1) first = snapshot(o.d, o.n, b.s);
    }
    return reps > 1 ? count_diff(o.d, first, b.s) : 0;
}

float* upload_f32(DevBufs& b, const float* h, size_t n) {
    float* d = (float*)b.alloc(n * 4);
    b.put(d, h, n * 4);
    return d;
}

// a Snake alpha vector as T plus its fp32 reciprocals, as the model's as_snake prepares it
template <typename T> const T* upload_snake(DevBufs& b, const float* alpha, int n, const float** ia) {
    T* d = b.upload<T>(alpha, (size_t)n);
    float* r = (float*)b.alloc((size_t)n * 4);
    launch_snake_inv<T>(b.s, d, n, r);
    HIPCHK(hipGetLastError());
    *ia = r;
    return d;
}

PackedW pack_host_weight(DevBufs& b, int prec, const float* w, size_t n, int kind, int Ci, int Co, int k, int st, int dil) {
    return pack_conv_weight(b.s, prec, upload_f32(b, w, n), kind, Ci, Co, k, st, dil,
                            [&b](size_t bytes) { return b.alloc(bytes); });
}

template <typename T>
void codec_conv_t(hipStream_t s, const fm_codec_conv_desc& d, const float* w, const float* bias, const float* x,
                  const float* gamma, const float* res, const float* alpha2, const float* normw, float* out, float* out2,
                  int* plan, int* dirty) {
    DevBufs b(s);
    const int prec = sizeof(T) == 2 ? FM_PREC_BF16 : FM_PREC_FP32;
    PackedW W;
    if (d.strided) {  // the encoder's strided conv as two taps over the [L/s][s*Ci] view
        const size_t n = (size_t)d.Co * d.Ci * 2 * d.stride;
        const std::vector<float> o = strided_as_two_taps(std::vector<float>(w, w + n), d.Ci, d.Co, d.stride);
        W = pack_host_weight(b, prec, o.data(), n, 0, d.stride * d.Ci, d.Co, 2, 1, 1);
    } else {
        const size_t taps = d.kind == 0 ? d.k : (d.kind == 1 ? 2 * d.stride : (d.kind == 2 ? d.stride : 1));
        W = pack_host_weight(b, prec, w, (size_t)d.Co * d.Ci * taps, d.kind, d.Ci, d.Co, d.k, d.stride, d.dil);
    }
    if (bias) W.bias = b.upload<T>(bias, (size_t)d.Co);
    small_m(W);
    if (d.ksplit > 0) W.ks = d.ksplit;
    FMCHECK(d.ldx >= W.Ci && d.ldx % 8 == 0, "x rows: ldx >= the layer's input width, a multiple of 8");
    const int cols = (d.flags & CE_SWIGLU) ? d.Co / 2 : d.Co, rows = d.Lq * W.stride;
    FMCHECK(!out || (d.ldo >= cols && d.out_rows >= rows), "out: [>= Lq * stride][ldo >= Co]");
    FMCHECK(!out2 || (d.ldo2 >= d.Co && d.out2_rows >= rows), "out2: [>= Lq * stride][ldo2 >= Co]");
    FMCHECK(!res || (d.ldr >= d.Co && d.res_rows >= rows), "res: [>= Lq * stride][ldr >= Co]");
    const bool f32 = d.flags & CE_F32OUT;
    T* xd = b.upload<T>(x, (size_t)(d.npre + d.Lx) * d.ldx);
    const float* ia2 = nullptr;
    const T* al = alpha2 ? upload_snake<T>(b, alpha2, d.Co, &ia2) : nullptr;
    const T* gm = gamma ? b.upload<T>(gamma, (size_t)d.Co) : nullptr;
    const T* rs = res ? b.upload<T>(res, (size_t)d.res_rows * d.ldr) : nullptr;
    InOut<T> ot(b, out, out && !f32 ? (size_t)d.out_rows * d.ldo : 0);
    InOut<float> of(b, out, out && f32 ? (size_t)d.out_rows * d.ldo : 0);
    InOut<T> o2(b, out2, out2 ? (size_t)d.out2_rows * d.ldo2 : 0);
    void* od = !out ? nullptr : (f32 ? (void*)of.d : (void*)ot.d);
    ConvArgs<T> a = conv_site_args<T>(W, xd + (size_t)d.npre * d.ldx, d.ldx, d.Lq, d.Lx, od, out ? d.ldo : 0, d.flags,
                                      rs, res ? d.ldr : 0, gm, al, ia2, out2 ? o2.d : nullptr, out2 ? d.ldo2 : 0, -d.npre);
    if (d.flags & CE_NORM) {
        a.normw = b.upload<T>(normw, (size_t)d.Co);
        a.norm_eps = d.norm_eps;
    }
    a.ksplit = fm_tuning().conv_splitk ? W.ks : 1;
    // the workspace: whole 64-row segments for Lq rows (or the rows asked for).  Everything behind the rows the
    // plan uses -- the tail of the last segment and SLAB_GUARD words more -- is filled with the guard word
    const size_t per_row = (size_t)std::max(a.ksplit, 1) * W.nphase * d.Co;
    a.slab_cap = (size_t)(d.slab_rows > 0 ? d.slab_rows : (d.Lq + 63) / 64 * 64) * per_row;
    a.slab = (float*)b.alloc((a.slab_cap + SLAB_GUARD) * 4);
    if (d.flags & CE_ROPE) {
        const auto tab = rope_table_host(d.rope_pos0 + d.Lq, d.rope_hd, d.rope_base);
        a.rope = upload_f32(b, tab.data(), tab.size());
        a.rope_pos0 = d.rope_pos0;
        a.rope_nqk = d.rope_nqk;
        a.rope_hd = d.rope_hd;
    }
    const ConvPlan p = conv_plan(a);
    const size_t used = p.epi == CEK_GEMM ? 0 : (size_t)std::min(p.seg_rows, d.Lq) * per_row;
    const std::vector<uint32_t> guard(a.slab_cap + SLAB_GUARD - used, GUARD_WORD);
    b.put(a.slab + used, guard.data(), guard.size() * 4);
    int changed = 0;
    std::vector<T> f1, f2;
    std::vector<float> ff;
    for (int i = 0; i < d.reps; ++i) {
        launch_conv_gemm<T>(s, a);
        HIPCHK(hipGetLastError());
        if (i == 0 && d.reps > 1) {
            f1 = snapshot(ot.d, ot.n, s);
            ff = snapshot(of.d, of.n, s);
            f2 = snapshot(o2.d, o2.n, s);
        }
    }
    if (d.reps > 1) changed = count_diff(ot.d, f1, s) + count_diff(of.d, ff, s) + count_diff(o2.d, f2, s);
    if (out) f32 ? of.get(s) : ot.get(s);
    if (out2) o2.get(s);
    const std::vector<float> g = snapshot(a.slab + used, guard.size(), s);
    *dirty = memcmp(g.data(), guard.data(), guard.size() * 4) != 0;
    plan[0] = p.kernel;
    plan[1] = p.ksplit;
    plan[2] = p.nseg;
    plan[3] = p.epi;
    plan[4] = changed;
    plan[5] = p.kernel_last;
}

void codec_resunit(hipStream_t s, int C, int L, int npre, int dil, const float* x, const float* w7, const float* b7,
                   const float* a2, const float* w1, const float* b1, const float* an, float* res, int res_rows,
                   int store_res, float* out2, int out2_rows, int reps, int* taken, int* changed) {
    using T = bf16_t;
    DevBufs b(s);
    const PackedW c7 = pack_host_weight(b, FM_PREC_BF16, w7, (size_t)C * C * 7, 0, C, C, 7, 1, dil);
    const PackedW c1 = pack_host_weight(b, FM_PREC_BF16, w1, (size_t)C * C, 0, C, C, 1, 1, 1);
    ResUnitArgs a{};
    T* xd = b.upload<T>(x, (size_t)(npre + L) * C);
    a.x = xd + (size_t)npre * C;
    a.L = L;
    a.lo = -npre;
    a.dil = dil;
    a.w7 = (const T*)c7.w;
    a.b7 = b.upload<T>(b7, (size_t)C);
    a.a2 = upload_snake<T>(b, a2, C, &a.ia2);
    a.w1 = (const T*)c1.w;
    a.b1 = b.upload<T>(b1, (size_t)C);
    InOut<T> rs(b, res, (size_t)res_rows * C);
    a.res = rs.d;
    a.store_res = store_res;
    a.an = upload_snake<T>(b, an, C, &a.ian);
    InOut<T> o2(b, out2, (size_t)out2_rows * C);
    a.out2 = o2.d;
    a.zeros = (const T*)b.alloc(256);
    resunit_init();
    std::vector<T> f1, f2;
    *taken = 1;
    *changed = 0;
    for (int i = 0; i < reps && *taken; ++i) {
        *taken = launch_resunit(s, a, C) ? 1 : 0;
        HIPCHK(hipGetLastError());
        if (i == 0 && reps > 1 && *taken) {
            f1 = snapshot(rs.d, rs.n, s);
            f2 = snapshot(o2.d, o2.n, s);
        }
    }
    if (reps > 1 && *taken) *changed = count_diff(rs.d, f1, s) + count_diff(o2.d, f2, s);
    rs.get(s);
    o2.get(s);
}

template <typename T>
void codec_window_attn_t(hipStream_t s, const float* qkv, int Tn, int H, int hd, int window, int npre, float* out,
                         int out_rows, int reps, int* changed) {
    DevBufs b(s);
    const size_t ld3 = (size_t)3 * H * hd;
    T* q = b.upload<T>(qkv, (size_t)(npre + Tn) * ld3);
    InOut<T> o(b, out, (size_t)out_rows * H * hd);
    *changed = run_reps(b, o, reps, false, [&] { launch_window_attn<T>(s, q + (size_t)npre * ld3, Tn, H, hd, window, o.d, npre); });
    o.get(s);
}

// the batched pass's attention and K/V state refresh on a table built like the model's (fm_codec_batch.h)
template <typename T>
void codec_window_attn_seg_t(hipStream_t s, int n, const int32_t* Tn, const int32_t* npre, int gap, const float* qkv, int H,
                             int hd, int window, float* state, int state_rows, float* out, int out_rows) {
    DevBufs b(s);
    const size_t ld3 = (size_t)3 * H * hd;
    const int span = (int)codec_batch_span(n, Tn, gap);
    T* q = b.upload<T>(qkv, (size_t)span * ld3);
    InOut<T> o(b, out, (size_t)out_rows * H * hd);
    std::vector<InOut<T>> st;
    std::vector<void*> ptr(n);
    std::vector<void* const*> bufs(n);
    st.reserve(n);
    for (int i = 0; i < n; ++i) {
        st.emplace_back(b, state + (size_t)i * state_rows * ld3, (size_t)state_rows * ld3);
        ptr[i] = st[i].d;
        bufs[i] = &ptr[i];
    }
    // (the table's pos0 only feeds npre = min(pos0, window - 1): the caller's npre stands in for it)
    std::vector<uint8_t> blob;
    CodecBatchLayout lay;
    codec_batch_fill(blob, lay, n, Tn, npre, gap, window - 1, 1, bufs.data());
    char* d = (char*)b.alloc(lay.bytes);
    b.put(d, blob.data(), lay.bytes);
    SegTable tb{(const CodecSeg*)(d + lay.seg_off), (const int32_t*)(d + lay.rowseg_off), (void* const*)(d + lay.st_off), n,
                span, 1};
    launch_window_attn_seg<T>(s, q, H, hd, window, o.d, tb, 0);
    HIPCHK(hipGetLastError());
    launch_kv_roll_seg<T>(s, q, H, hd, window, tb, 0);
    HIPCHK(hipGetLastError());
    o.get(s);
    for (int i = 0; i < n; ++i) st[i].get(s);
}

template <typename T>
void codec_rope_qk_t(hipStream_t s, float* qkv, int rows, int Tn, int H, int hd, float base, int pos0, int reps,
                     int* changed) {
    DevBufs b(s);
    InOut<T> q(b, qkv, (size_t)rows * 3 * H * hd);
    const auto tab = rope_table_host(pos0 + Tn, hd, base);
    const float* td = upload_f32(b, tab.data(), tab.size());
    *changed = run_reps(b, q, reps, true, [&] { launch_rope_qk<T>(s, q.d, Tn, H, hd, td, pos0); });
    q.get(s);
}

template <typename T>
void codec_dwconv_ln_t(hipStream_t s, const float* x, int L, int D, int npre, const float* dw, const float* db,
                       const float* lw, const float* lb, float* y, int y_rows, int reps, int* changed) {
    DevBufs b(s);
    T* xd = b.upload<T>(x, (size_t)(npre + L) * D);
    InOut<T> o(b, y, (size_t)y_rows * D);
    const T *dwd = b.upload<T>(dw, (size_t)D * 7), *dbd = b.upload<T>(db, (size_t)D), *lwd = b.upload<T>(lw, (size_t)D),
            *lbd = b.upload<T>(lb, (size_t)D);
    *changed = run_reps(b, o, reps, false, [&] { launch_dwconv_ln<T>(s, xd + (size_t)npre * D, L, D, dwd, dbd, lwd, lbd, o.d, -npre); });
    o.get(s);
}

template <typename T>
void codec_rvq_decode_t(hipStream_t s, const int32_t* codes, int Tn, int nq1, int sem, int cbs, int cd,
                        const float* cb_sem, const float* cb, const float* w, const float* bias, int D, float* z,
                        int z_rows, int reps, int* changed) {
    DevBufs b(s);
    int32_t* cdev = (int32_t*)b.alloc((size_t)nq1 * Tn * 4);
    b.put(cdev, codes, (size_t)nq1 * Tn * 4);
    RvqPtrs p{};
    const float* wd = upload_f32(b, w, (size_t)nq1 * D * cd);
    const float* bd = upload_f32(b, bias, (size_t)nq1 * D);
    p.cb[0] = upload_f32(b, cb_sem, (size_t)sem * cd);
    const float* cbd = nq1 > 1 ? upload_f32(b, cb, (size_t)(nq1 - 1) * cbs * cd) : nullptr;
    for (int q = 0; q < nq1 && q < 16; ++q) {  // (more stages: the launcher refuses)
        if (q) p.cb[q] = cbd + (size_t)(q - 1) * cbs * cd;
        p.w[q] = wd + (size_t)q * D * cd;
        p.b[q] = bd + (size_t)q * D;
    }
    InOut<T> o(b, z, (size_t)z_rows * D);
    *changed = run_reps(b, o, reps, false, [&] { launch_rvq_decode<T>(s, cdev, Tn, nq1, sem, cbs, cd, p, D, o.d); });
    o.get(s);
}

template <typename T>
void codec_snake_t(hipStream_t s, const float* x, int C, size_t n, const float* alpha, float* y, size_t y_len,
                   float* ialpha, int reps, int* changed) {
    DevBufs b(s);
    const float* ia = nullptr;
    const T* al = upload_snake<T>(b, alpha, C, &ia);
    InOut<T> o(b, y, y_len);
    const T* xd = b.upload<T>(x, n);
    *changed = run_reps(b, o, reps, false, [&] { launch_snake<T>(s, xd, C, n, al, o.d); });
    o.get(s);
    if (ialpha) {
        HIPCHK(hipMemcpyAsync(ialpha, ia, (size_t)C * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
}

template <typename T>
void codec_silu_mul_t(hipStream_t s, const float* g, float* y, size_t n, size_t y_len, int reps, int* changed) {
    DevBufs b(s);
    InOut<T> o(b, y, y_len);
    const T* gd = b.upload<T>(g, n);
    *changed = run_reps(b, o, reps, true, [&] { launch_silu_mul<T>(s, gd, o.d, n); });
    o.get(s);
}

}  // namespace

extern "C" {

int fm_op_codec_conv(int device, const fm_codec_conv_desc* d, const float* w, const float* bias, const float* x,
                     const float* gamma, const float* res, const float* alpha2, const float* normw, float* out,
                     float* out2, int* plan, int* dirty) {
    return fm_guard([&] {
        FMCHECK(d && w && x && plan && dirty, "null argument");
        FMCHECK(d->precision == FM_PREC_BF16 || d->precision == FM_PREC_FP32, "bad precision");
        FMCHECK(d->kind >= 0 && d->kind <= 3 && d->Ci >= 8 && d->Ci % 8 == 0 && d->Co >= 1 && d->Co <= 8192 && d->Ci <= 8192,
                "kind 0..3, Ci a multiple of 8, 1 <= Co");
        FMCHECK(d->stride >= 1 && d->stride <= 16 && d->dil >= 1 && d->dil <= 64 && d->k >= 1 && d->k <= 32,
                "stride 1..16, dil 1..64, k 1..32");
        FMCHECK(d->kind != 0 || d->strided || d->k <= 8, "Conv1d: at most 8 taps");
        FMCHECK(d->kind != 1 || d->k == 2 * d->stride, "ConvTranspose1d kind 1 has k = 2 * stride");
        FMCHECK(d->kind != 2 || d->k == d->stride, "ConvTranspose1d kind 2 has k = stride");
        FMCHECK(!d->strided || (d->kind == 0 && d->k == 2 * d->stride && d->dil == 1), "strided: Conv1d with k = 2 * stride");
        FMCHECK(d->Lq >= 1 && d->Lq <= (1 << 20) && d->Lx >= 1 && d->Lx <= (1 << 20) && d->npre >= 0 && d->npre <= 4096,
                "1 <= Lq, Lx <= 2^20, 0 <= npre <= 4096");
        const int all = CE_GELU | CE_RES | CE_GAMMA | CE_STORE | CE_TANH | CE_F32OUT | CE_SWIGLU | CE_ROPE | CE_NORM;
        FMCHECK((d->flags & ~all) == 0, "flags: GELU, RES, GAMMA, STORE, TANH, F32OUT, SWIGLU, ROPE, NORM (bias and Snake follow the operands)");
        FMCHECK(((d->flags & CE_STORE) != 0) == (out != nullptr), "out goes with CE_STORE");
        FMCHECK(((d->flags & CE_RES) != 0) == (res != nullptr), "res goes with CE_RES");
        FMCHECK(((d->flags & CE_GAMMA) != 0) == (gamma != nullptr) && (!gamma || res), "gamma goes with CE_RES | CE_GAMMA");
        FMCHECK(!(d->flags & CE_F32OUT) || out, "CE_F32OUT needs out");
        if (d->flags & CE_NORM)
            FMCHECK(normw && out2 && !alpha2, "CE_NORM: normw and out2 (the norm's output), no Snake");
        else
            FMCHECK(!normw && (out2 != nullptr) == (alpha2 != nullptr), "out2 goes with alpha2 (the Snake)");
        FMCHECK(!(d->flags & CE_ROPE) || (d->rope_hd >= 2 && d->rope_hd % 2 == 0 && d->rope_hd <= 256 && d->rope_pos0 >= 0 &&
                                          d->rope_pos0 <= (1 << 20) && d->rope_base > 0),
                "CE_ROPE: an even head_dim, pos0 >= 0, base > 0");
        FMCHECK(d->ksplit >= 0 && d->ksplit <= 64 && d->slab_rows >= 0 && d->reps >= 1 && d->reps <= 8,
                "0 <= ksplit <= 64, slab_rows >= 0, reps 1..8");
        StreamGuard g(device);
        if (d->precision == FM_PREC_BF16)
            codec_conv_t<bf16_t>(g.s, *d, w, bias, x, gamma, res, alpha2, normw, out, out2, plan, dirty);
        else
            codec_conv_t<float>(g.s, *d, w, bias, x, gamma, res, alpha2, normw, out, out2, plan, dirty);
    });
}

int fm_op_codec_resunit(int device, int C, int L, int npre, int dil, const float* x, const float* w7, const float* b7,
                        const float* a2, const float* w1, const float* b1, const float* an, float* res, int res_rows,
                        int store_res, float* out2, int out2_rows, int reps, int* taken, int* changed) {
    return fm_guard([&] {
        FMCHECK(x && w7 && b7 && a2 && w1 && b1 && an && res && out2 && taken && changed, "null argument");
        FMCHECK(C >= 8 && C % 8 == 0 && C <= 1024 && L >= 1 && L <= (1 << 20) && npre >= 0 && npre <= 4096 && dil >= 1 &&
                    dil <= 64,
                "C a multiple of 8 up to 1024, 1 <= L <= 2^20, 0 <= npre <= 4096, 1 <= dil <= 64");
        FMCHECK(res_rows >= L && out2_rows >= L && reps >= 1 && reps <= 8, "res, out2: at least L rows; reps 1..8");
        StreamGuard g(device);
        codec_resunit(g.s, C, L, npre, dil, x, w7, b7, a2, w1, b1, an, res, res_rows, store_res, out2, out2_rows, reps,
                      taken, changed);
    });
}

int fm_op_codec_window_attn(int device, int precision, const float* qkv, int Tn, int H, int hd, int window, int npre,
                            float* out, int out_rows, int reps, int* changed) {
    return fm_guard([&] {
        FMCHECK(qkv && out && changed && reps >= 1 && reps <= 8, "null argument, or reps outside 1..8");
        FMCHECK(Tn >= 1 && Tn <= (1 << 16) && H >= 1 && H <= 64 && hd >= 1 && hd <= 1024 && npre >= 0 && npre <= 4096 &&
                    out_rows >= Tn,
                "1 <= Tn <= 65536, 1 <= H <= 64, 0 <= npre <= 4096, out rows >= Tn");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) codec_window_attn_t<bf16_t>(g.s, qkv, Tn, H, hd, window, npre, out, out_rows, reps, changed);
        else codec_window_attn_t<float>(g.s, qkv, Tn, H, hd, window, npre, out, out_rows, reps, changed);
    });
}

int fm_op_codec_window_attn_seg(int device, int precision, int n, const int32_t* T, const int32_t* npre, int gap,
                                const float* qkv, int H, int hd, int window, float* state, int state_rows, float* out,
                                int out_rows) {
    return fm_guard([&] {
        FMCHECK(T && npre && qkv && state && out, "null argument");
        FMCHECK(n >= 1 && n <= 1024 && gap >= 0 && gap <= 64 && H >= 1 && H <= 64 && hd >= 1 && hd <= 1024 && window >= 2 &&
                    window <= 129 && state_rows >= window - 1 && state_rows <= 4096,
                "1 <= n <= 1024, 0 <= gap <= 64, 1 <= H <= 64, 2 <= window <= 129, window - 1 <= state rows <= 4096");
        for (int i = 0; i < n; ++i)
            FMCHECK(T[i] >= 1 && T[i] <= (1 << 16) && npre[i] >= 0 && npre[i] <= window - 1,
                    "1 <= T[i] <= 65536, 0 <= npre[i] <= window - 1");
        const int64_t span = codec_batch_span(n, T, gap);
        FMCHECK(span <= (1 << 20) && out_rows >= span && out_rows <= (1 << 21), "span <= 2^20 rows, out rows >= span");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            codec_window_attn_seg_t<bf16_t>(g.s, n, T, npre, gap, qkv, H, hd, window, state, state_rows, out, out_rows);
        else
            codec_window_attn_seg_t<float>(g.s, n, T, npre, gap, qkv, H, hd, window, state, state_rows, out, out_rows);
    });
}

int fm_op_codec_rope_qk(int device, int precision, float* qkv, int rows, int Tn, int H, int hd, float base, int pos0,
                        int reps, int* changed) {
    return fm_guard([&] {
        FMCHECK(qkv && Tn >= 1 && rows >= Tn && rows <= (1 << 16) && H >= 1 && H <= 64 && hd >= 1 && hd <= 1024 &&
                    base > 0 && pos0 <= (1 << 20),
                "1 <= Tn <= rows <= 65536, 1 <= H <= 64, base > 0, pos0 <= 2^20");
        FMCHECK(hd % 2 == 0 && pos0 >= 0, "rope: an even head_dim, pos0 >= 0");
        FMCHECK(changed && reps >= 1 && reps <= 8, "null argument, or reps outside 1..8");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) codec_rope_qk_t<bf16_t>(g.s, qkv, rows, Tn, H, hd, base, pos0, reps, changed);
        else codec_rope_qk_t<float>(g.s, qkv, rows, Tn, H, hd, base, pos0, reps, changed);
    });
}

int fm_op_codec_dwconv_ln(int device, int precision, const float* x, int L, int D, int npre, const float* dw,
                          const float* db, const float* lw, const float* lb, float* y, int y_rows, int reps, int* changed) {
    return fm_guard([&] {
        FMCHECK(x && dw && db && lw && lb && y && changed && reps >= 1 && reps <= 8, "null argument, or reps outside 1..8");
        FMCHECK(L >= 1 && L <= (1 << 16) && D >= 1 && D <= (1 << 16) && npre >= 0 && npre <= 4096 && y_rows >= L,
                "1 <= L, D <= 65536, 0 <= npre <= 4096, y rows >= L");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) codec_dwconv_ln_t<bf16_t>(g.s, x, L, D, npre, dw, db, lw, lb, y, y_rows, reps, changed);
        else codec_dwconv_ln_t<float>(g.s, x, L, D, npre, dw, db, lw, lb, y, y_rows, reps, changed);
    });
}

int fm_op_codec_rvq_decode(int device, int precision, const int32_t* codes, int Tn, int nq1, int sem, int cbs, int cd,
                           const float* cb_sem, const float* cb, const float* w, const float* bias, int D, float* z,
                           int z_rows, int reps, int* changed) {
    return fm_guard([&] {
        FMCHECK(codes && cb_sem && (cb || nq1 == 1) && w && bias && z && changed && reps >= 1 && reps <= 8,
                "null argument, or reps outside 1..8");
        FMCHECK(Tn >= 1 && Tn <= (1 << 16) && nq1 >= 1 && nq1 <= 64 && sem >= 1 && cbs >= 1 && cd >= 1 && cd <= 64 &&
                    D >= 1 && D <= (1 << 16) && z_rows >= Tn,
                "bad shape");
        for (size_t i = 0; i < (size_t)nq1 * Tn; ++i) FMCHECK(codes[i] >= 0, "codes must be non-negative (only the maximum is clamped)");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            codec_rvq_decode_t<bf16_t>(g.s, codes, Tn, nq1, sem, cbs, cd, cb_sem, cb, w, bias, D, z, z_rows, reps, changed);
        else
            codec_rvq_decode_t<float>(g.s, codes, Tn, nq1, sem, cbs, cd, cb_sem, cb, w, bias, D, z, z_rows, reps, changed);
    });
}

int fm_op_codec_snake(int device, int precision, const float* x, int C, int64_t n, const float* alpha, float* y,
                      int64_t y_len, float* ialpha, int reps, int* changed) {
    return fm_guard([&] {
        FMCHECK(x && alpha && y && C >= 1 && n >= 1 && n <= ((int64_t)1 << 28) && y_len >= n && y_len <= ((int64_t)1 << 28),
                "need x, alpha, y, C >= 1, 1 <= n <= y_len <= 2^28");
        FMCHECK(changed && reps >= 1 && reps <= 8, "null argument, or reps outside 1..8");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) codec_snake_t<bf16_t>(g.s, x, C, (size_t)n, alpha, y, (size_t)y_len, ialpha, reps, changed);
        else codec_snake_t<float>(g.s, x, C, (size_t)n, alpha, y, (size_t)y_len, ialpha, reps, changed);
    });
}

int fm_op_codec_silu_mul(int device, int precision, const float* g_, float* y, int64_t n, int64_t y_len, int reps,
                         int* changed) {
    return fm_guard([&] {
        FMCHECK(g_ && y && n >= 1 && y_len >= n && y_len <= ((int64_t)1 << 28), "need g, y, 1 <= n <= y_len <= 2^28");
        FMCHECK(changed && reps >= 1 && reps <= 8, "null argument, or reps outside 1..8");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) codec_silu_mul_t<bf16_t>(g.s, g_, y, (size_t)n, (size_t)y_len, reps, changed);
        else codec_silu_mul_t<float>(g.s, g_, y, (size_t)n, (size_t)y_len, reps, changed);
    });
}

int fm_op_codec_wn_fold(int device, const float* g_, const float* v, int rows, int per, float* w, int64_t w_len, int reps,
                        int* changed) {
    return fm_guard([&] {
        FMCHECK(g_ && v && w && rows >= 1 && rows <= (1 << 16) && per >= 1 && per <= (1 << 24) &&
                    w_len >= (int64_t)rows * per && w_len <= ((int64_t)1 << 28),
                "need g, v, w, 1 <= rows <= 65536, per >= 1, w_len >= rows * per");
        FMCHECK(changed && reps >= 1 && reps <= 8, "null argument, or reps outside 1..8");
        StreamGuard g(device);
        DevBufs b(g.s);
        InOut<float> o(b, w, (size_t)w_len);
        const float *gd = upload_f32(b, g_, (size_t)rows), *vd = upload_f32(b, v, (size_t)rows * per);
        *changed = run_reps(b, o, reps, false, [&] { launch_wn_fold(g.s, gd, vd, rows, per, o.d); });
        o.get(g.s);
    });
}

int fm_op_codec_vq_encode(int device, float* r, int Tn, int D, int nst, int cd, const float* wi, const float* bi,
                          const float* cb, const int32_t* cbn, const float* wo, const float* bo, int32_t* codes, int reps,
                          int* changed) {
    return fm_guard([&] {
        FMCHECK(r && wi && bi && cb && cbn && wo && bo && codes && changed && reps >= 1 && reps <= 8,
                "null argument, or reps outside 1..8");
        FMCHECK(Tn >= 1 && Tn <= (1 << 16) && D >= 1 && D <= (1 << 16) && nst >= 1 && nst <= 64 && cd >= 1 && cd <= 64,
                "bad shape");
        size_t total = 0;
        for (int q = 0; q < nst && q < 16; ++q) {
            FMCHECK(cbn[q] >= 1 && cbn[q] <= (1 << 20), "codebook sizes 1 .. 2^20");
            total += (size_t)cbn[q];
        }
        StreamGuard g(device);
        DevBufs b(g.s);
        VqEncPtrs p{};
        const float* wid = upload_f32(b, wi, (size_t)nst * cd * D);
        const float* bid = upload_f32(b, bi, (size_t)nst * cd);
        const float* cbd = upload_f32(b, cb, total * cd);
        const float* wod = upload_f32(b, wo, (size_t)nst * D * cd);
        const float* bod = upload_f32(b, bo, (size_t)nst * D);
        size_t off = 0;
        for (int q = 0; q < nst && q < 16; ++q) {
            p.wi[q] = wid + (size_t)q * cd * D;
            p.bi[q] = bid + (size_t)q * cd;
            p.cb[q] = cbd + off * cd;
            p.wo[q] = wod + (size_t)q * D * cd;
            p.bo[q] = bod + (size_t)q * D;
            p.cbn[q] = cbn[q];
            off += (size_t)cbn[q];
        }
        InOut<float> rr(b, r, (size_t)Tn * D);
        int32_t* cdev = (int32_t*)b.alloc((size_t)nst * Tn * 4);
        std::vector<int32_t> c1;  // the residual is updated in place: the caller's values again before each launch
        *changed = run_reps(b, rr, reps, true, [&] {
            if (!c1.empty()) HIPCHK(hipMemsetAsync(cdev, 0xff, (size_t)nst * Tn * 4, g.s));
            launch_vq_encode(g.s, rr.d, Tn, D, nst, cd, p, cdev);
            if (c1.empty() && reps > 1) c1 = snapshot(cdev, (size_t)nst * Tn, g.s);
        });
        if (reps > 1) *changed += count_diff(cdev, c1, g.s);
        rr.get(g.s);
        HIPCHK(hipMemcpyAsync(codes, cdev, (size_t)nst * Tn * 4, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
    });
}

}  // extern "C"
