// fm_ops.cpp -- per-op test hooks of libfishmi (include/fishmi.h, "per-op parity hooks").
//
// Each hook runs ONE production kernel of the decode path on caller-supplied operands, so the
// GPU tests can hold the fused forms to the reference's per-op goldens (tests/golden/ops.npz):
//   fm_op_rmsnorm   RMSNorm (llama.py:989-1000) as the decode path computes it: the GEMV
//                   prologue (first layer / head: statistic from the row itself; later layers:
//                   statistic from the producing GEMV's per-tile sums of squares), or the
//                   standalone row kernel of the batched / prefill path
//   fm_op_qk_rope   QK-norm (llama.py:861-863) + RoPE with the bf16 table (llama.py:1003-1037)
//                   inside the fused decode attention kernels (slow attn_fd / attn_decode2, fast attn2)
//   fm_op_decode_attn  the whole slow decode attention (QK-norm, RoPE, KV write, scaled dot-product
//                   attention over the cache, llama.py:883-945) on R rows with caller K/V caches
//   fm_op_prompt_attn  the prompt-chunk causal attention (llama.py:883-946) over a cache prefix,
//                   on the split kernel or the flash-form attn_prefill_kernel
//   fm_op_embed     the Dual-AR input embedding (llama.py:399-420)
//   fm_op_batched_linear_q8  the batched decode linear (bsacc_kernel) on weight-only int8 codes and on
//                   their bf16 fragment copy (fm_tune bstream_q8)
//   fm_op_batched_linear_q4  the same on weight-only int4 codes + group (scale, zero) and on the bf16
//                   fragments of the dequantised weights (fm_tune bstream_q4)
//   fm_op_linear / fm_op_gemv / fm_op_rowgemv / fm_op_bstream / fm_op_finalize_norm / fm_op_prompt_skinny
//                   the decode linears, one production launcher each (launch_linear, launch_gemv, launch_rowgemv,
//                   launch_bstream on bstream_plan's geometry, launch_finalize_norm, launch_prompt_skinny): outputs
//                   are in/out arrays with spare rows / columns, the launch can be repeated on the same scratch,
//                   and the ticket words left non-zero are counted (tests/test_gpu_linear_ops.py)
//   fm_op_prompt_skinny_q  launch_prompt_skinny on weight-only int8 / int4 codes and on their bf16 fragment
//                   copy (fm_tune prompt_skinny_q; tests/test_gpu_prompt_skinny_q.py)
//   fm_op_prompt_gemm_q  launch_conv_gemm, as the prompt pass calls it at more than 64 rows, on weight-only int8 /
//                   int4 codes and on their bf16 fragment copy (fm_tune prompt_gemm_q; tests/test_gpu_prompt_gemm_q.py)
//   fm_op_sample    the decode sampler (launch_sample_radix: sample_fast_kernel / sample_radix_kernel and
//                   their shared wide path) once on caller logits rows, slot table, RAS window and
//                   forced columns; cols and the tap are in/out (tests/test_gpu_sampler_ops.py)
//   fm_rope_table   the host-built bf16 cos/sin table (no device needed)
// Operands are fp32 host arrays, converted to the precision's storage type (bf16 rounding is the
// caller's business: pass bf16-valued floats for bit-level comparisons).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fm_codec.h"
#include "fm_kernels.h"
#include "fm_llm_model.h"
#include "fm_ops_util.h"
#include "fm_runtime.h"

using namespace fm_ops_util;

namespace {

// a knob set for one launch and put back whatever happens in between (a launcher's FMCHECK throws)
struct TuneScope {
    int& knob;
    const int keep;
    TuneScope(int& k, int v) : knob(k), keep(k) { knob = v; }
    ~TuneScope() { knob = keep; }
};

template <typename T>
void rmsnorm_t(hipStream_t s, int mode, const float* x, const float* w, int R, int d, float eps, float* y) {
    DevBufs b(s);
    T* xd = b.upload<T>(x, (size_t)R * d);
    T* wd = b.upload<T>(w, (size_t)d);
    T* yd = (T*)b.alloc((size_t)R * d * sizeof(T));
    if (mode == 2) {
        launch_rmsnorm<T>(s, xd, d, wd, d, eps, yd, d, R);
    } else {
        // a 16-row GEMV of zeros: only its prologue's X' (stored through xn_out) is looked at
        T* wz = (T*)b.alloc((size_t)16 * d * sizeof(T));
        T* yz = (T*)b.alloc((size_t)R * 16 * sizeof(T));
        int* tickets = (int*)b.alloc(4096);
        GemvArgs<T> a{};
        a.W = wz;
        a.nw = wd;
        a.eps = eps;
        a.R = R;
        a.N = 16;
        a.K = d;
        a.Y = yz;
        a.ldy = 16;
        a.xn_out = yd;
        a.ldxo = d;
        a.tickets = tickets;
        if (mode == 0) {  // PRO_NORM: first layer / head, statistic from the row itself
            a.X = xd;
            a.ldx = d;
            launch_gemv<T>(s, a, PRO_NORM, EPI_STORE, 1);
        } else {
            // PRO_PRENORM: a zero-weight EPI_SLABFIN GEMV finalises x = round(x + round(0)) and
            // its per-16-column sums of squares, exactly as the wo / w2 GEMVs do for the next norm
            T* xz = (T*)b.alloc((size_t)R * 32 * sizeof(T));
            T* wz2 = (T*)b.alloc((size_t)d * 32 * sizeof(T));
            float* slab = (float*)b.alloc((size_t)R * d * 4);
            float* ss = (float*)b.alloc((size_t)(d / 16) * R * 4);
            T* xf = (T*)b.alloc((size_t)R * d * sizeof(T));
            GemvArgs<T> f{};
            f.W = wz2;
            f.X = xz;
            f.ldx = 32;
            f.R = R;
            f.N = d;
            f.K = 32;
            f.Yf = slab;
            f.ldy = d;
            f.res = xd;
            f.ldr = d;
            f.res_out = xf;
            f.ldro = d;
            f.ss_out = ss;
            f.tickets = tickets;
            f.eps = eps;
            launch_gemv<T>(s, f, PRO_PLAIN, EPI_SLABFIN, 1);
            a.X = xf;
            a.ldx = d;
            a.ss_in = ss;
            launch_gemv<T>(s, a, PRO_PRENORM, EPI_STORE, 1);
        }
    }
    HIPCHK(hipGetLastError());
    download<T>(yd, (size_t)R * d, y, s);
}

template <typename T>
void qk_rope_t(hipStream_t s, int kernel, const float* qkv, int nh, int nkv, int hd, const float* qn,
               const float* kn, int qk_norm, float eps, float base, int pos, float* q_out, float* k_out) {
    DevBufs b(s);
    const int ld = (nh + 2 * nkv) * hd;
    T* raw = b.upload<T>(qkv, (size_t)ld);
    T* qnd = qk_norm ? b.upload<T>(qn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    T* knd = qk_norm ? b.upload<T>(kn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    const int S = (pos + 1 + 7) / 8 * 8;
    auto tab = rope_table_host(S, hd, base);
    float* rope = (float*)b.alloc(tab.size() * 4);
    b.put(rope, tab.data(), tab.size() * 4);
    const size_t stride = (size_t)nkv * S * hd;
    T* kc = (T*)b.alloc(stride * sizeof(T));
    T* vc = (T*)b.alloc(stride * sizeof(T));
    T* out = (T*)b.alloc((size_t)nh * hd * sizeof(T));
    float* qd = (float*)b.alloc((size_t)nh * hd * 4);
    int* row = (int*)b.alloc(8);
    const int rs[2] = {0, pos};
    b.put(row, rs, 8);
    const float scale = 1.0f / sqrtf((float)hd);
    if (kernel == 0 || kernel == 2 || kernel == 3) {  // slow decode attention
        AttnDecArgs<T> a{raw, ld, row, row + 1, nh, nkv, hd, qk_norm, eps, qnd, knd, rope, kc, vc, stride, 0, S,
                         1, scale, nullptr};
        a.cap = attn2_cap(hd, nh / nkv, sizeof(T));
        a.maxsplit = FM_CEIL(S, std::min(a.cap, 16));  // covers both kernels' split counts
        a.part = (float*)b.alloc((size_t)nh * a.maxsplit * (hd + 2) * 4);
        a.cnt = (int*)b.alloc((size_t)nh * 4);
        a.out = out;
        a.qdbg = qd;
        // kernel 0: attn_decode2 (the B <= 8 decode path), 2: attn_dec3 (the batched frame)
        if (kernel == 2) {
            launch_attn_decode3<T>(s, a, 1);
        } else if (kernel == 3) {  // attn_fd as the batch-1 decode runs it (8-wave blocks)
            FMCHECK(attn_fd_ok(hd, nh / nkv), "attn_fd: head_dim 32, 64 or 128, at most 4 q heads per kv head");
            a.cap = std::max(16, fm_tuning().fd_min16);
            a.nwb = fm_tuning().fd_nw;
            a.hpb = fd_hpb_rows(1);
            a.maxsplit = FM_CEIL(S, a.cap);
            launch_attn_fd<T>(s, a, 1);
        } else {
            a.maxsplit = FM_CEIL(S, a.cap);
            launch_attn_decode2<T>(s, a, 1);
        }
    } else {  // fast-model attention (one wave per q head) at codebook position pos
        FMCHECK(pos < 16, "fast attention positions are < 16");
        FastFusedArgs<T> a{raw, ld, row, nh, nkv, hd, qk_norm, eps, qnd, knd, rope, kc, vc, stride, 0, S, pos,
                           scale, out};
        a.qdbg = qd;
        launch_fast_attn2<T>(s, a, 1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q_out, qd, (size_t)nh * hd * 4, hipMemcpyDeviceToHost, s));
    for (int h = 0; h < nkv; ++h) download<T>(kc + (size_t)h * S * hd + (size_t)pos * hd, hd, k_out + (size_t)h * hd, s);
    HIPCHK(hipStreamSynchronize(s));
}

// R prompt rows of one slot at positions pos0 .. pos0 + R - 1 over caller caches [nkv][S][hd]
// (keys / values of every position <= pos0 + R - 1 already written, as qk_rope_cache leaves them)
template <typename T>
void prompt_attn_t(hipStream_t s, int kernel, const float* q, int R, int nh, int nkv, int hd, int pos0,
                   const float* kcache, const float* vcache, int S, float* out) {
    DevBufs b(s);
    T* qd = b.upload<T>(q, (size_t)R * nh * hd);
    T* kc = b.upload<T>(kcache, (size_t)nkv * S * hd);
    T* vc = b.upload<T>(vcache, (size_t)nkv * S * hd);
    T* o = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
    int* rows = (int*)b.alloc((size_t)2 * R * 4);
    std::vector<int> rs(2 * R);
    for (int r = 0; r < R; ++r) {
        rs[r] = 0;
        rs[R + r] = pos0 + r;
    }
    b.put(rows, rs.data(), rs.size() * 4);
    const int split = 64, maxsplit = FM_CEIL(S, split);
    AttnArgs<T> a{qd, rows, rows + R, kc, vc, (size_t)nkv * S * hd, 0, S, nh, nkv, hd, split, maxsplit,
                  1.0f / sqrtf((float)hd), (float*)b.alloc((size_t)R * nh * maxsplit * (hd + 2) * 4)};
    {
        const TuneScope knob(fm_tuning().prefill_attn, kernel);
        launch_attn<T>(s, a, R, maxsplit, o, true);
    }
    download<T>(o, (size_t)R * nh * hd, out, s);
}

// one decode attention launch over R rows (slot r = row r) with caller K/V caches [R][nkv][S][hd]
// holding rows < pos[r]; the kernel writes row pos[r] (normed + roped k, raw v) itself
template <typename T>
void decode_attn_t(hipStream_t s, int kernel, const float* qkv, int R, int nh, int nkv, int hd, const float* qn,
                   const float* kn, int qk_norm, float eps, float base, const int* pos, const float* kcache,
                   const float* vcache, int S, int min_split, float* out, float* kc_out, float* vc_out) {
    DevBufs b(s);
    const int ld = (nh + 2 * nkv) * hd;
    T* raw = b.upload<T>(qkv, (size_t)R * ld);
    T* qnd = qk_norm ? b.upload<T>(qn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    T* knd = qk_norm ? b.upload<T>(kn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    auto tab = rope_table_host(S, hd, base);
    float* rope = (float*)b.alloc(tab.size() * 4);
    b.put(rope, tab.data(), tab.size() * 4);
    const size_t stride = (size_t)nkv * S * hd;
    T* kc = b.upload<T>(kcache, (size_t)R * stride);
    T* vc = b.upload<T>(vcache, (size_t)R * stride);
    T* o = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
    int* rows = (int*)b.alloc((size_t)2 * R * 4);
    std::vector<int> rs(2 * R);
    for (int r = 0; r < R; ++r) {
        rs[r] = r;
        rs[R + r] = pos[r];
    }
    b.put(rows, rs.data(), rs.size() * 4);
    AttnDecArgs<T> a{raw, ld, rows, rows + R, nh, nkv, hd, qk_norm, eps, qnd, knd, rope, kc, vc, stride, 0, S,
                     1, 1.0f / sqrtf((float)hd), nullptr};
    const int g = nh / nkv;
    a.maxsplit = FM_CEIL(S, 16);
    a.part = (float*)b.alloc((size_t)R * nh * a.maxsplit * (hd + 2) * 4);
    a.cnt = (int*)b.alloc((size_t)R * nh * 4);
    a.out = o;
    if (kernel == 3) {
        FMCHECK(attn_fd_ok(hd, g), "attn_fd: head_dim 32, 64 or 128 and at most 4 q heads per kv head");
        a.cap = min_split;
        a.hpb = fd_hpb_rows(R);
        launch_attn_fd<T>(s, a, R);
    } else if (kernel == 2) {
        FMCHECK(hd % 32 == 0 && hd <= 128 && g <= 6, "attn_dec3: hd a multiple of 32 up to 128, g <= 6");
        launch_attn_decode3<T>(s, a, R);
    } else {
        a.cap = std::min(min_split, attn2_cap(hd, g, sizeof(T)));
        a.maxsplit = FM_CEIL(S, a.cap);
        launch_attn_decode2<T>(s, a, R);
    }
    HIPCHK(hipGetLastError());
    download<T>(o, (size_t)R * nh * hd, out, s);
    download<T>(kc, (size_t)R * stride, kc_out, s);
    download<T>(vc, (size_t)R * stride, vc_out, s);
}

// ---- attention hooks with slot indirection, layers and the frame's launch forms (tests/test_gpu_attn_ops.py) ----
int count_nonzero(const int* d, size_t n, hipStream_t s);
// fp32 host array as is (K-part slabs)
float* upload_raw(DevBufs& b, const float* h, size_t n) {
    float* d = (float*)b.alloc(n * 4);
    b.put(d, h, n * 4);
    return d;
}
int* upload_i32(DevBufs& b, const int* h, size_t n) {
    int* d = (int*)b.alloc(n * 4);
    b.put(d, h, n * 4);
    return d;
}
float* upload_rope(DevBufs& b, int S, int hd, float base) {
    auto tab = rope_table_host(S, hd, base);
    return upload_raw(b, tab.data(), tab.size());
}

struct DecodeAttnEx {
    int kernel;
    const float *qkv, *slab;
    int kp;
    const float* bias;
    int R, nh, nkv, hd;
    const float *qn, *kn;
    int qk_norm;
    float eps, base;
    const int *row_slot, *pos;
    int nslots, layers, layer;
    float *kc, *vc;
    int S, cap, nwb, frame, reps;
    float* out;
    int* info;
};
constexpr int PART_GUARD = 1024;  // sentinel words behind the split partials
// one slow decode attention launch (or o.reps of them) over R rows in slots row_slot[r] of caller caches
// [nslots][layers][nkv][S][hd], layer o.layer; o.frame: kernel, nwb and cap as a frame of R rows picks them
template <typename T> void decode_attn_ex_t(hipStream_t s, const DecodeAttnEx& o) {
    DevBufs b(s);
    const int R = o.R, nh = o.nh, nkv = o.nkv, hd = o.hd, S = o.S, g = nh / nkv;
    const int ld = (nh + 2 * nkv) * hd;
    const T* raw = o.qkv ? b.upload<T>(o.qkv, (size_t)R * ld) : nullptr;
    const float* slab = o.slab ? upload_raw(b, o.slab, (size_t)o.kp * R * ld) : nullptr;
    const T* bias = o.bias ? b.upload<T>(o.bias, (size_t)ld) : nullptr;
    T* qnd = o.qk_norm ? b.upload<T>(o.qn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    T* knd = o.qk_norm ? b.upload<T>(o.kn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    float* rope = upload_rope(b, S, hd, o.base);
    const size_t layer_stride = (size_t)nkv * S * hd, slot_stride = (size_t)o.layers * layer_stride;
    InOut<T> kc(b, o.kc, (size_t)o.nslots * slot_stride), vc(b, o.vc, (size_t)o.nslots * slot_stride);
    T* out = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
    std::vector<int> rs(2 * R);
    for (int r = 0; r < R; ++r) {
        rs[r] = o.row_slot[r];
        rs[R + r] = o.pos[r];
    }
    int* rows = upload_i32(b, rs.data(), rs.size());
    int kernel = o.kernel, nwb = o.nwb, cap = o.cap, hpb = fd_hpb_rows(R);  // (fd_hpb holds without o.frame too)
    const int cap2 = attn2_cap(hd, g, sizeof(T));
    if (o.frame) {  // as blk_attn / small_attn do
        const AttnSlowPlan p = attn_slow_plan(R, hd, g, attn2_frame_cap(hd, g, sizeof(T), R > GEMV_MAX_ROWS));
        kernel = p.kernel;
        nwb = p.nwb;
        cap = p.cap;
        hpb = p.hpb;
    }
    if (kernel == 0) cap = std::min(cap, cap2);
    FMCHECK(!slab || kernel == 3, "the slab form of the QKV input needs attn_fd");
    FMCHECK(kernel != 3 || attn_fd_ok(hd, g), "attn_fd: head_dim 32, 64 or 128 and at most 4 q heads per kv head");
    FMCHECK(kernel != 2 || (hd % 32 == 0 && hd <= 128 && g <= 6), "attn_dec3: hd a multiple of 32 up to 128, g <= 6");
    const int maxsplit = kernel == 3 ? std::min(FD_NSP, FM_CEIL(S, cap)) : (kernel == 2 ? FM_CEIL(S, 64) : FM_CEIL(S, cap));
    AttnDecArgs<T> a{raw, ld, rows, rows + R, nh, nkv, hd, o.qk_norm, o.eps, qnd, knd, rope, kc.d, vc.d, slot_stride,
                     (size_t)o.layer * layer_stride, S, maxsplit, 1.0f / sqrtf((float)hd), nullptr};
    // partials exactly as fm_kernels.h sizes them, poisoned (an unwritten partial must not be read), then the guard
    const size_t npart = (size_t)R * nh * maxsplit * (hd + 2);
    a.part = (float*)b.alloc((npart + PART_GUARD) * 4);
    HIPCHK(hipMemsetAsync(a.part, 0xff, npart * 4, s));
    const std::vector<uint32_t> guard(PART_GUARD, 0x5a5a5a5au);
    b.put(a.part + npart, guard.data(), PART_GUARD * 4);
    a.cnt = (int*)b.alloc((size_t)R * nh * 4);  // attn_fd: a ticket per (row, kv head, head group)
    a.out = out;
    a.cap = cap;
    a.nwb = nwb;
    a.hpb = hpb;
    a.qslab = slab;
    a.qslab_kp = o.kp;
    a.qbias = bias;
    for (int i = 0; i < o.reps; ++i) {
        if (kernel == 3)
            launch_attn_fd<T>(s, a, R);
        else if (kernel == 2)
            launch_attn_decode3<T>(s, a, R);
        else
            launch_attn_decode2<T>(s, a, R);
        HIPCHK(hipGetLastError());
    }
    download<T>(out, (size_t)R * nh * hd, o.out, s);
    kc.get(s);
    vc.get(s);
    std::vector<uint32_t> back(PART_GUARD);
    HIPCHK(hipMemcpyAsync(back.data(), a.part + npart, PART_GUARD * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int info[8] = {kernel, nwb, cap, maxsplit, count_nonzero(a.cnt, (size_t)R * nh, s), back == guard, FD_NSP, cap2};
    memcpy(o.info, info, sizeof(info));
}

struct SlotRows {
    const int *row_slot, *row_pos;  // row_pos null: fixed_pos
    int nslots, layers, layer;
};
// launch_qk_rope_cache on R rows (qkv, or kp slabs + bias): q out, caches in/out
template <typename T>
void qk_rope_cache_t(hipStream_t s, const float* qkv, const float* slabh, int kp, const float* biash, int R, int nh,
                     int nkv, int hd, const float* qn, const float* kn, int qk_norm, float eps, float base,
                     const SlotRows& sr, int fixed_pos, float* kch, float* vch, int S, float* q_out) {
    DevBufs b(s);
    const int ld = (nh + 2 * nkv) * hd;
    const T* raw = qkv ? b.upload<T>(qkv, (size_t)R * ld) : nullptr;
    const float* slab = slabh ? upload_raw(b, slabh, (size_t)kp * R * ld) : nullptr;
    const T* bias = biash ? b.upload<T>(biash, (size_t)ld) : nullptr;
    T* qnd = qk_norm ? b.upload<T>(qn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    T* knd = qk_norm ? b.upload<T>(kn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    float* rope = upload_rope(b, S, hd, base);
    const size_t layer_stride = (size_t)nkv * S * hd, slot_stride = (size_t)sr.layers * layer_stride;
    InOut<T> kc(b, kch, (size_t)sr.nslots * slot_stride), vc(b, vch, (size_t)sr.nslots * slot_stride);
    T* q = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
    std::vector<int> rs(2 * R, 0);
    for (int r = 0; r < R; ++r) {
        rs[r] = sr.row_slot[r];
        if (sr.row_pos) rs[R + r] = sr.row_pos[r];
    }
    int* rows = upload_i32(b, rs.data(), rs.size());
    QkArgs<T> a{raw, ld, rows, rows + R, fixed_pos, nh, nkv, hd, qk_norm, eps, qnd, knd, rope, q, kc.d, vc.d, slot_stride,
                (size_t)sr.layer * layer_stride, S};
    a.qslab = slab;
    a.qslab_kp = kp;
    a.qbias = bias;
    launch_qk_rope_cache<T>(s, a, R);
    HIPCHK(hipGetLastError());
    download<T>(q, (size_t)R * nh * hd, q_out, s);
    kc.get(s);
    vc.get(s);
}

// launch_attn on R prompt rows with their own (slot, pos) over caller caches [nslots][layers][nkv][S][hd]
template <typename T>
void prompt_attn_ex_t(hipStream_t s, int kernel, const float* q, int R, int nh, int nkv, int hd, const SlotRows& sr,
                      int one_slot, const float* kcache, const float* vcache, int S, float* out) {
    DevBufs b(s);
    T* qd = b.upload<T>(q, (size_t)R * nh * hd);
    const size_t layer_stride = (size_t)nkv * S * hd, slot_stride = (size_t)sr.layers * layer_stride;
    T* kc = b.upload<T>(kcache, (size_t)sr.nslots * slot_stride);
    T* vc = b.upload<T>(vcache, (size_t)sr.nslots * slot_stride);
    T* o = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
    std::vector<int> rs(2 * R);
    for (int r = 0; r < R; ++r) {
        rs[r] = sr.row_slot[r];
        rs[R + r] = sr.row_pos[r];
    }
    int* rows = upload_i32(b, rs.data(), rs.size());
    const int split = ATTN_SPLIT, maxsplit = FM_CEIL(S, split);
    const size_t npart = (size_t)R * nh * maxsplit * (hd + 2);
    float* part = (float*)b.alloc(npart * 4);
    HIPCHK(hipMemsetAsync(part, 0xff, npart * 4, s));  // an unwritten partial must not be read
    AttnArgs<T> a{qd, rows, rows + R, kc, vc, slot_stride, (size_t)sr.layer * layer_stride, S, nh, nkv, hd, split, maxsplit,
                  1.0f / sqrtf((float)hd), part};
    {
        const TuneScope knob(fm_tuning().prefill_attn, kernel);
        launch_attn<T>(s, a, R, maxsplit, o, one_slot != 0);
        HIPCHK(hipGetLastError());
    }
    download<T>(o, (size_t)R * nh * hd, out, s);
}

// the fast decoder's attention at codebook position cpos on R rows: kernel 0 fast_attn2, 1 fast_attn2 with noq,
// 2 fast_attn_fused, 3 qk_rope_cache(fixed_pos) + fast_attn_kernel (the unfused pair); caches in/out
template <typename T>
void fast_attn_t(hipStream_t s, int kernel, const float* qkv, int R, int nh, int nkv, int hd, const float* qn,
                 const float* kn, int qk_norm, float eps, float base, const SlotRows& sr, int cpos, float* kch, float* vch,
                 int S, float* outh) {
    DevBufs b(s);
    const int ld = (nh + 2 * nkv) * hd;
    const T* raw = b.upload<T>(qkv, (size_t)R * ld);
    T* qnd = qk_norm ? b.upload<T>(qn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    T* knd = qk_norm ? b.upload<T>(kn, (size_t)hd) : (T*)b.alloc((size_t)hd * sizeof(T));
    float* rope = upload_rope(b, S, hd, base);
    const size_t layer_stride = (size_t)nkv * S * hd, slot_stride = (size_t)sr.layers * layer_stride;
    const size_t layer_off = (size_t)sr.layer * layer_stride;
    InOut<T> kc(b, kch, (size_t)sr.nslots * slot_stride), vc(b, vch, (size_t)sr.nslots * slot_stride);
    T* out = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
    int* rows = upload_i32(b, sr.row_slot, (size_t)R);
    const float scale = 1.0f / sqrtf((float)hd);
    if (kernel == 3) {
        T* q = (T*)b.alloc((size_t)R * nh * hd * sizeof(T));
        QkArgs<T> qa{raw, ld, rows, nullptr, cpos, nh, nkv, hd, qk_norm, eps, qnd, knd, rope, q, kc.d, vc.d, slot_stride,
                     layer_off, S};
        launch_qk_rope_cache<T>(s, qa, R);
        HIPCHK(hipGetLastError());
        FastAttnArgs<T> fa{q, rows, kc.d, vc.d, slot_stride, layer_off, S, nh, nkv, hd, cpos, scale, out};
        launch_fast_attn<T>(s, fa, R);
    } else {
        FastFusedArgs<T> a{raw, ld, rows, nh, nkv, hd, qk_norm, eps, qnd, knd, rope, kc.d, vc.d, slot_stride, layer_off, S,
                           cpos, scale, out};
        a.noq = kernel == 1;
        if (kernel == 2)
            launch_fast_attn_fused<T>(s, a, R);
        else
            launch_fast_attn2<T>(s, a, R);
    }
    HIPCHK(hipGetLastError());
    download<T>(out, (size_t)R * nh * hd, outh, s);
    kc.get(s);
    vc.get(s);
}

// the batch-1 fast decoder's attention + wo: one launch_fattn_wo (fused), or the launches it replaces
// (launch_fast_attn2 + launch_rowgemv FIN) on the same device operands
struct FattnWoOp {
    int quant, gs, fused;
    const float *qkv, *qtab;
    int qrows;
    const int32_t* idx;
    int idx_n, idx_col, nh, nkv, hd;
    const float *qn, *kn;
    int qk_norm;
    float eps, base;
    int slot, cpos, nslots, layers, layer;
    float *kc, *vc;
    int S;
    const float *w, *bias, *res;
    int res_rows, ldr;
    const float* res0;
    int N, kv0, pair, ilp, gen, pos0;
    const uint32_t* xt_init;
    float* y;
    int* status;
};
void fattn_wo_op(hipStream_t s, const FattnWoOp& o) {
    DevBufs b(s);
    const int nh = o.nh, nkv = o.nkv, hd = o.hd, S = o.S, N = o.N, K = nh * hd, ld = (nh + 2 * nkv) * hd;
    const int qm = o.quant == FM_QUANT_INT4 ? 2 : (o.quant == FM_QUANT_INT8 ? 1 : 0);
    // "not dispatchable" is a status, not a launch: what small_path asks before it takes the fused launch
    // (status[0]: the dispatched depth -- rowgemv_u's chunks per wave -- or 0 where the form is not instantiated)
    o.status[0] = fattn_wo_ok(nh, nkv, hd, o.cpos, N, K, qm) && (!(o.qtab || o.kv0) || fattn_wo_dead_ok(K, qm)) &&
                          (!o.pair || rowgemv_pair_ok(-1, K, false, qm))
                      ? rowgemv_u(K, qm)
                      : 0;
    o.status[1] = 0;
    if (!o.status[0]) return;
    RowGemvArgs r{};
    const int Np = (N + 15) / 16 * 16;
    bf16_t* wd = (bf16_t*)b.alloc((size_t)Np * K * 2);
    HIPCHK(hipMemcpyAsync(wd, b.upload<bf16_t>(o.w, (size_t)N * K), (size_t)N * K * 2, hipMemcpyDeviceToDevice, s));
    if (qm == 1) {  // the quantizers of fm_llm_set_quant / _int4 on the device, as rowgemv_op and fm_op_quant4 run them
        int8_t* dq = (int8_t*)b.alloc((size_t)Np * K);
        bf16_t* ds = (bf16_t*)b.alloc((size_t)Np * 2);
        launch_quant_rows<bf16_t>(s, wd, N, K, dq, ds);
        r.Wq = dq;
        r.wscale = ds;
    } else if (qm == 2) {
        uint8_t* dq = (uint8_t*)b.alloc((size_t)Np * K);
        uint32_t* dsz = (uint32_t*)b.alloc((size_t)Np * (K / o.gs) * 4);
        uint32_t* words = (uint32_t*)b.alloc((size_t)Np * K / 2);
        launch_quant4(s, wd, N, K, o.gs, dq, dsz);
        launch_pack_q4_rows(s, dq, N, K, words);
        r.Wq4 = words;
        r.wsz = dsz;
        r.gs = o.gs;
    } else {
        r.W = wd;
    }
    HIPCHK(hipGetLastError());
    if (o.bias) r.bias = b.upload<bf16_t>(o.bias, (size_t)N);
    const int rows = o.pair ? 2 : 1;
    const bf16_t* raw = b.upload<bf16_t>(o.qkv, (size_t)rows * ld);
    const bf16_t* qtab = o.qtab ? b.upload<bf16_t>(o.qtab, (size_t)o.qrows * ld) : nullptr;
    const int32_t* idx = o.idx ? upload_i32(b, o.idx, (size_t)o.idx_n) : nullptr;
    bf16_t* qnd = o.qk_norm ? b.upload<bf16_t>(o.qn, (size_t)hd) : (bf16_t*)b.alloc((size_t)hd * 2);
    bf16_t* knd = o.qk_norm ? b.upload<bf16_t>(o.kn, (size_t)hd) : (bf16_t*)b.alloc((size_t)hd * 2);
    float* rope = upload_rope(b, S, hd, o.base);
    const size_t layer_stride = (size_t)nkv * S * hd, slot_stride = (size_t)o.layers * layer_stride;
    InOut<bf16_t> kc(b, o.kc, (size_t)o.nslots * slot_stride), vc(b, o.vc, (size_t)o.nslots * slot_stride);
    const int rs[2] = {o.slot, o.pos0};
    int* rows_d = upload_i32(b, rs, 2);
    bf16_t* att = (bf16_t*)b.alloc((size_t)K * 2);
    FastFusedArgs<bf16_t> at{raw, ld, rows_d, nh, nkv, hd, o.qk_norm, o.eps, qnd, knd, rope, kc.d, vc.d, slot_stride,
                             (size_t)o.layer * layer_stride, S, o.cpos, 1.0f / sqrtf((float)hd), att};
    at.row_pos = rows_d + 1;
    // residual(s): the table res [res_rows][ldr], row idx[idx_col] of it (clamped) when idx is given, else row 0
    const bf16_t* res = b.upload<bf16_t>(o.res, (size_t)o.res_rows * o.ldr);
    r.ldr = o.ldr;
    r.residx = idx;
    r.res_col = o.idx_col;
    r.res_rows = o.res_rows;
    r.N = N;
    r.K = K;
    InOut<bf16_t> y(b, o.y, (size_t)(o.pair == 1 ? 2 : 1) * N);
    r.res = res;
    r.res_out = y.d;
    if (o.pair == 1) {  // row 0's residual as it stands, row 1's from the table
        r.xr = 2;
        r.res = b.upload<bf16_t>(o.res0, (size_t)N);
        r.res1 = res;
        r.res_out1 = y.d + N;
    }
    int* err = (int*)b.alloc(16);
    if (o.fused) {
        FattnWoArgs A{};
        A.at = at;
        A.wo = r;
        A.wo.X = att;  // (unused: x comes from the tagged words)
        A.xt = (uint32_t*)b.alloc((size_t)2 * K * 4);
        if (o.xt_init) b.put(A.xt, o.xt_init, (size_t)2 * K * 4);
        A.gen = o.gen;
        A.err = err;
        A.delay = fm_tuning().fw_delay;
        A.cheap = fm_tuning().fw_cheap;
        A.prio = fm_tuning().fw_prio;
        A.ilp = o.ilp;
        if (qtab) {
            A.qtab = qtab;
            A.qidx = idx;
            A.qcol = o.idx_col;
            A.qrows = o.qrows;
        }
        A.kv0 = o.kv0;
        A.pair = o.pair;
        launch_fattn_wo(s, A);  // one launch, never repeated: its waits are bounded and set err
    } else {
        FMCHECK(!o.pair, "the unfused composition runs one row");
        if (qtab) {  // the QKV launch's output is the table row of the (clamped) index
            const int iv = o.idx[o.idx_col], xi = iv < 0 ? 0 : (iv >= o.qrows ? o.qrows - 1 : iv);
            at.qkv = qtab + (size_t)xi * ld;
        }
        at.noq = o.kv0;
        launch_fast_attn2<bf16_t>(s, at, 1);
        HIPCHK(hipGetLastError());
        r.X = att;
        launch_rowgemv(s, r, ROWGEMV_FIN);
    }
    HIPCHK(hipGetLastError());
    y.get(s);
    kc.get(s);
    vc.get(s);
    HIPCHK(hipMemcpyAsync(&o.status[1], err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
}

// the batch-1 slow layers' attention + wo at nrun (slot, position) pairs, one after the other on the same device
// operands: one launch_slow_attn_wo each (fused), or the two launches it replaces (launch_attn_fd as attn_slow_plan
// runs it at one row + launch_rowgemv FIN).  The tagged-word buffer lives through the call, so a run finds the words
// its predecessors left.  quant (fm_op_slow_attn_wo_q): w is quantised and packed on the device first, by the model's
// rule and pack launchers as fattn_wo_op does, and both compositions run on the row-major codes
struct SlowAttnWoOp {
    int quant, gs;
    int8_t* q_out;
    float *scale_out, *zero_out;
    int fused, rp;
    const float* qkv;
    int nh, nkv, hd;
    const float *qn, *kn;
    int qk_norm;
    float eps, base;
    const int32_t *slots, *pos, *gens;
    int nrun, restore, nslots, layers, layer;
    const float *kc, *vc;
    int S;
    const float *w, *bias, *res;
    int N;
    const uint32_t* xt_init;
    float *y, *krows, *vrows;
    int* status;
};
void slow_attn_wo_op(hipStream_t s, const SlowAttnWoOp& o) {
    DevBufs b(s);
    const int nh = o.nh, nkv = o.nkv, hd = o.hd, S = o.S, N = o.N, K = nh * hd, ld = (nh + 2 * nkv) * hd, g = nh / nkv;
    const AttnSlowPlan ap = attn_slow_plan(1, hd, g, attn2_frame_cap(hd, g, 2, false));
    // "not dispatchable" is a status, not a launch: what small_path asks before it takes the fused launch
    const int qm = o.quant == FM_QUANT_INT4 ? 2 : (o.quant == FM_QUANT_INT8 ? 1 : 0);
    o.status[0] = ap.kernel == 3 && ap.nwb == 8 && ap.hpb == 1 && slow_attn_wo_ok(nh, nkv, hd, N, K, qm) && !fm_tuning().gemv_chain;
    o.status[1] = 0;
    if (o.fused && !o.status[0]) return;
    FMCHECK(ap.kernel == 3, "the unfused composition runs attn_fd");
    RowGemvArgs r{};
    bf16_t* wd = b.upload<bf16_t>(o.w, (size_t)N * K);
    if (qm == 1) {  // the quantizers of fm_llm_set_quant / _int4 on the device, as rowgemv_op and fm_op_quant4 run them
        int8_t* dq = (int8_t*)b.alloc((size_t)N * K);
        bf16_t* ds = (bf16_t*)b.alloc((size_t)N * 2);
        launch_quant_rows<bf16_t>(s, wd, N, K, dq, ds);
        HIPCHK(hipGetLastError());
        r.Wq = dq;
        r.wscale = ds;
        if (o.q_out) {
            HIPCHK(hipMemcpyAsync(o.q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (o.scale_out) download<bf16_t>(ds, (size_t)N, o.scale_out, s);
    } else if (qm == 2) {
        const int ng = K / o.gs;
        uint8_t* dq = (uint8_t*)b.alloc((size_t)N * K);
        uint32_t* dsz = (uint32_t*)b.alloc((size_t)N * ng * 4);
        uint32_t* words = (uint32_t*)b.alloc((size_t)N * K / 2);
        launch_quant4(s, wd, N, K, o.gs, dq, dsz);
        launch_pack_q4_rows(s, dq, N, K, words);
        HIPCHK(hipGetLastError());
        r.Wq4 = words;
        r.wsz = dsz;
        r.gs = o.gs;
        if (o.q_out) {
            HIPCHK(hipMemcpyAsync(o.q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (o.scale_out || o.zero_out) {  // one word per (row, group): scale in the low half, zero in the high one
            std::vector<uint32_t> hs((size_t)N * ng);
            HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t i = 0; i < hs.size(); ++i) {
                const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
                if (o.scale_out) memcpy(&o.scale_out[i], &us, 4);
                if (o.zero_out) memcpy(&o.zero_out[i], &uz, 4);
            }
        }
    } else {
        r.W = wd;
    }
    if (o.bias) r.bias = b.upload<bf16_t>(o.bias, (size_t)N);
    r.res = b.upload<bf16_t>(o.res, (size_t)N);
    r.ldr = N;
    r.N = N;
    r.K = K;
    const bf16_t* raw = b.upload<bf16_t>(o.qkv, (size_t)o.nrun * ld);
    bf16_t* qnd = o.qk_norm ? b.upload<bf16_t>(o.qn, (size_t)hd) : (bf16_t*)b.alloc((size_t)hd * 2);
    bf16_t* knd = o.qk_norm ? b.upload<bf16_t>(o.kn, (size_t)hd) : (bf16_t*)b.alloc((size_t)hd * 2);
    float* rope = upload_rope(b, S, hd, o.base);
    const size_t layer_stride = (size_t)nkv * S * hd, slot_stride = (size_t)o.layers * layer_stride;
    const size_t cn = (size_t)o.nslots * slot_stride, layer_off = (size_t)o.layer * layer_stride;
    const bf16_t *kc0 = b.upload<bf16_t>(o.kc, cn), *vc0 = b.upload<bf16_t>(o.vc, cn);
    bf16_t *kc = (bf16_t*)b.alloc(cn * 2), *vc = (bf16_t*)b.alloc(cn * 2);
    HIPCHK(hipMemcpyAsync(kc, kc0, cn * 2, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(vc, vc0, cn * 2, hipMemcpyDeviceToDevice, s));
    int* rows_d = (int*)b.alloc(8);
    bf16_t* att = (bf16_t*)b.alloc((size_t)K * 2);
    bf16_t* yd = (bf16_t*)b.alloc((size_t)o.nrun * N * 2);
    bf16_t *kr = (bf16_t*)b.alloc((size_t)o.nrun * nkv * hd * 2), *vr = (bf16_t*)b.alloc((size_t)o.nrun * nkv * hd * 2);
    uint32_t* xt = (uint32_t*)b.alloc((size_t)K * 4);
    if (o.xt_init) b.put(xt, o.xt_init, (size_t)K * 4);
    int* err = (int*)b.alloc(16);
    AttnDecArgs<bf16_t> at{raw, ld, rows_d, rows_d + 1, nh, nkv, hd, o.qk_norm, o.eps, qnd, knd, rope, kc, vc, slot_stride,
                           layer_off, S, 1, 1.0f / sqrtf((float)hd), nullptr};
    at.cap = ap.cap;
    at.nwb = ap.nwb;
    at.hpb = ap.hpb;
    at.maxsplit = std::min(FD_NSP, FM_CEIL(S, at.cap));
    at.part = (float*)b.alloc((size_t)nh * at.maxsplit * (hd + 2) * 4);
    at.cnt = (int*)b.alloc((size_t)nh * 4);
    at.out = att;
    for (int i = 0; i < o.nrun; ++i) {
        if (o.restore && i) {
            HIPCHK(hipMemcpyAsync(kc, kc0, cn * 2, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(vc, vc0, cn * 2, hipMemcpyDeviceToDevice, s));
        }
        const int rs[2] = {o.slots[i], o.pos[i]};
        b.put(rows_d, rs, 8);
        at.qkv = raw + (size_t)i * ld;
        r.res_out = yd + (size_t)i * N;
        r.X = att;
        if (o.fused) {
            SlowAttnWoArgs A{};
            A.at = at;
            A.wo = r;  // (X: unused, x comes from the tagged words)
            A.xt = xt;
            A.gen = o.gens[i];
            A.err = err;
            A.rp = o.rp;
            A.delay_pct = fm_tuning().slow_aw_delay;
            A.sleep = fm_tuning().slow_aw_sleep;
            A.cheap = fm_tuning().slow_aw_cheap;
            launch_slow_attn_wo(s, A);  // one launch, never repeated: its waits are bounded and set err
        } else {
            launch_attn_fd<bf16_t>(s, at, 1);
            HIPCHK(hipGetLastError());
            launch_rowgemv(s, r, ROWGEMV_FIN);
        }
        HIPCHK(hipGetLastError());
        // the K / V rows this run wrote: position pos[i] of every kv head of (slot, layer)
        const size_t row0 = (size_t)o.slots[i] * slot_stride + layer_off + (size_t)o.pos[i] * hd;
        HIPCHK(hipMemcpy2DAsync(kr + (size_t)i * nkv * hd, (size_t)hd * 2, kc + row0, (size_t)S * hd * 2, (size_t)hd * 2, nkv,
                                hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(vr + (size_t)i * nkv * hd, (size_t)hd * 2, vc + row0, (size_t)S * hd * 2, (size_t)hd * 2, nkv,
                                hipMemcpyDeviceToDevice, s));
    }
    download<bf16_t>(yd, (size_t)o.nrun * N, o.y, s);
    download<bf16_t>(kr, (size_t)o.nrun * nkv * hd, o.krows, s);
    download<bf16_t>(vr, (size_t)o.nrun * nkv * hd, o.vrows, s);
    HIPCHK(hipMemcpyAsync(&o.status[1], err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
}

template <typename T>
void embed_t(hipStream_t s, const int32_t* tok, int R, const float* emb, int V, const float* cbemb, int d, int C,
             int cb, int sb, int se, int scale, float* x) {
    DevBufs b(s);
    T* e = b.upload<T>(emb, (size_t)V * d);
    T* ce = b.upload<T>(cbemb, (size_t)C * cb * d);
    int32_t* td = (int32_t*)b.alloc((size_t)R * (C + 1) * 4);
    b.put(td, tok, (size_t)R * (C + 1) * 4);
    T* xd = (T*)b.alloc((size_t)R * d * sizeof(T));
    launch_embed<T>(s, td, R, e, ce, d, C, cb, sb, se, scale, xd, nullptr);
    HIPCHK(hipGetLastError());
    download<T>(xd, (size_t)R * d, x, s);
}

// ---- linear hooks (fm_op_linear .. fm_op_prompt_skinny) -----------------------------------------
int count_nonzero(const int* d, size_t n, hipStream_t s) {
    std::vector<int> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), d, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return (int)std::count_if(h.begin(), h.end(), [](int v) { return v != 0; });
}

// row-major fp32 host weight [N][K] -> the packed MFMA-fragment layout, rows padded to 16 (zeros)
template <typename T> T* upload_packed(DevBufs& b, const float* w, int N, int K) {
    T* t = b.upload<T>(w, (size_t)N * K);
    T* pk = (T*)b.alloc((size_t)((N + 15) / 16 * 16) * K * sizeof(T));
    launch_pack<T>(b.s, t, N, K, pk);
    HIPCHK(hipGetLastError());
    return pk;
}

template <typename T>
void linear_op_t(hipStream_t s, int epi, const float* w, const float* w2, const float* bias, const float* x, int ldx,
                 const float* res, int ldr, int R, int N, int K, int split, float* y, int ldy, int y_rows, int reps,
                 int* ksb_out, int* dirty) {
    DevBufs b(s);
    const bool f32 = epi == EPI_F32;
    LinearArgs<T> a{};
    a.W = upload_packed<T>(b, w, N, K);
    if (epi == EPI_SWIGLU) a.W2 = upload_packed<T>(b, w2, N, K);
    if (bias) a.bias = b.upload<T>(bias, (size_t)N);
    a.X = b.upload<T>(x, (size_t)R * ldx);
    a.ldx = ldx;
    a.R = R;
    a.N = N;
    a.K = K;
    a.ldy = ldy;
    if (epi == EPI_RESID) {
        a.res = b.upload<T>(res, (size_t)R * ldr);
        a.ldr = ldr;
    }
    InOut<T> yt(b, y, f32 ? 1 : (size_t)y_rows * ldy);
    InOut<float> yf(b, y, f32 ? (size_t)y_rows * ldy : 1);
    a.Y = f32 ? nullptr : yt.d;
    a.Yf = f32 ? yf.d : nullptr;
    const int nacc = epi == EPI_SWIGLU ? 2 : 1, tiles = (N + 15) / 16;
    const bool can_split = split && R > 8 && R <= 64;  // as the batched decode frame offers it
    const int ksb = linear_ksb(N, K, R, nacc, can_split);
    int* tickets = (int*)b.alloc((size_t)tiles * 4);
    if (can_split) {
        a.part = (float*)b.alloc((size_t)ksb * nacc * R * N * 4);
        a.tickets = tickets;
    }
    for (int i = 0; i < reps; ++i) launch_linear<T>(s, a, epi);
    HIPCHK(hipGetLastError());
    if (f32) yf.get(s);
    else yt.get(s);
    *ksb_out = ksb;
    *dirty = count_nonzero(tickets, (size_t)tiles, s);
}

struct GemvOp {
    int pro, epi, ksb;
    const float *w, *w2, *bias, *nw;
    float eps;
    const float* x;
    int x_rows, ldx;
    const int32_t* idx;
    int idx_ld, idx_col, idx_rows;
    const float* res;
    int res_rows, ldr, ss_gran, R, N, K;
    float* y;
    int ldy, y_rows;
    float* ss_out;
    int reps;
    int* dirty;
};

template <typename T> void gemv_op_t(hipStream_t s, const GemvOp& o) {
    DevBufs b(s);
    const int R = o.R, N = o.N, K = o.K, tiles = (N + 15) / 16;
    const bool f32 = o.epi == EPI_F32 || o.epi == EPI_SLAB;
    GemvArgs<T> a{};
    a.W = upload_packed<T>(b, o.w, N, K);
    if (o.epi == EPI_SWIGLU) a.W2 = upload_packed<T>(b, o.w2, N, K);
    if (o.bias) a.bias = b.upload<T>(o.bias, (size_t)N);
    if (o.nw) a.nw = b.upload<T>(o.nw, (size_t)K);
    a.eps = o.eps;
    a.ldx = o.ldx;
    a.R = R;
    a.N = N;
    a.K = K;
    a.dummy_tail = fm_tuning().gemv_dummy;
    int* tickets = (int*)b.alloc((size_t)(tiles + 16) * 4);
    a.tickets = tickets;
    T* xd = b.upload<T>(o.x, (size_t)o.x_rows * o.ldx);
    a.X = xd;
    if (o.idx) {
        int32_t* id = (int32_t*)b.alloc((size_t)R * o.idx_ld * 4);
        b.put(id, o.idx, (size_t)R * o.idx_ld * 4);
        if (o.pro == PRO_NORM) a.xidx = id;
        else a.residx = id;
        a.xidx_ld = o.idx_ld;
        a.xidx_col = o.idx_col;
        a.xidx_rows = o.idx_rows;
    }
    if (o.pro == PRO_PRENORM) {
        // as rmsnorm_t: a zero-weight EPI_SLABFIN GEMV finalises x = round(x + round(0)) and leaves the
        // per-16-column sums of squares [K/16][R] the way the wo / w2 GEMVs do for the next norm
        T* xz = (T*)b.alloc((size_t)R * 32 * sizeof(T));
        T* wz = (T*)b.alloc((size_t)K * 32 * sizeof(T));
        float* slab = (float*)b.alloc((size_t)R * K * 4);
        float* ss = (float*)b.alloc((size_t)(K / 16) * R * 4);
        T* xf = b.upload<T>(o.x, (size_t)R * o.ldx);
        GemvArgs<T> f{};
        f.W = wz;
        f.X = xz;
        f.ldx = 32;
        f.R = R;
        f.N = K;
        f.K = 32;
        f.Yf = slab;
        f.ldy = K;
        f.res = xd;
        f.ldr = o.ldx;
        f.res_out = xf;
        f.ldro = o.ldx;
        f.ss_out = ss;
        f.tickets = tickets;
        f.eps = o.eps;
        launch_gemv<T>(s, f, PRO_PLAIN, EPI_SLABFIN, 1);
        HIPCHK(hipGetLastError());
        a.X = xf;
        a.ss_in = ss;
        a.ss_gran = o.ss_gran;
    }
    const int ycols_rows = o.y_rows;
    InOut<T> yt(b, o.y, f32 ? 1 : (size_t)ycols_rows * o.ldy);
    InOut<float> yf(b, o.y, f32 ? (size_t)ycols_rows * o.ldy : 1);
    std::vector<float> one(1, 0.f);
    InOut<float> ss(b, o.epi == EPI_SLABFIN ? o.ss_out : one.data(), o.epi == EPI_SLABFIN ? (size_t)(N / 16) * R : 1);
    a.ldy = o.ldy;
    if (o.epi == EPI_SLABFIN) {
        a.res = b.upload<T>(o.res, (size_t)o.res_rows * o.ldr);
        a.ldr = o.ldr;
        a.res_out = yt.d;
        a.ldro = o.ldy;
        a.ss_out = ss.d;
        a.Yf = (float*)b.alloc((size_t)o.ksb * R * N * 4);  // K-slice partials (scratch)
        a.ldy = N;
    } else if (f32) {
        a.Yf = yf.d;
    } else {
        a.Y = yt.d;
    }
    for (int i = 0; i < o.reps; ++i) launch_gemv<T>(s, a, o.pro, o.epi, o.ksb);
    HIPCHK(hipGetLastError());
    if (f32) yf.get(s);
    else yt.get(s);
    if (o.epi == EPI_SLABFIN) ss.get(s);
    *o.dirty = count_nonzero(tickets, (size_t)tiles + 16, s);
}

struct BstreamOp {
    int pro, epi;
    const float *w, *bias, *nw;
    float eps;
    const float* x;
    int ldx;
    const float* res;
    int ldr, R, N, K;
    float* y;
    int ldy, y_rows;
    float* ss_out;
    int reps;
    int* plan;
    int* dirty;
};

template <typename T> void bstream_op_t(hipStream_t s, const BstreamOp& o) {
    DevBufs b(s);
    bsacc_init();
    const int R = o.R, N = o.N, K = o.K, tiles = (N + 15) / 16;
    const BstreamPlan p = bstream_plan(N, K, R, o.epi, sizeof(T));
    FMCHECK(p.ok, "bstream: no plan for this shape");
    FMCHECK((o.epi != EPI_SLABFIN && o.pro != PRO_PRENORM) || p.acc, "bstream: SLABFIN / PRENORM run on bsacc_kernel only");
    const int slabs = (o.epi == EPI_SLAB) ? p.kparts : 1;
    FMCHECK(o.y_rows >= slabs * R, "bstream: the output holds fewer rows than [kparts][R]");
    const bool f32 = o.epi == EPI_F32 || o.epi == EPI_SLAB;
    BstreamArgs<T> a{};
    a.W = upload_packed<T>(b, o.w, N, K);
    if (o.bias) a.bias = b.upload<T>(o.bias, (size_t)N);
    T* xd = b.upload<T>(o.x, (size_t)R * o.ldx);
    a.X = xd;
    a.ldx = o.ldx;
    a.R = R;
    a.N = N;
    a.K = K;
    a.eps = o.eps;
    const size_t ntk = (size_t)tiles + 1024;  // one word per tile group (at most one per CU), the producer's too
    int* tickets = (int*)b.alloc(ntk * 4);
    if constexpr (sizeof(T) == 2) {
        if (o.pro == PRO_PRENORM) {
            // the producer's sums of squares [R][K/16]: a zero-weight bsacc EPI_SLABFIN launch (N = K, 8 k-steps)
            // finalises x = round(x + round(0)) and its per-tile sums as the batched wo / w2 do
            const BstreamPlan pz = bstream_plan(K, 256, R, EPI_SLABFIN, sizeof(T));
            FMCHECK(pz.ok && pz.acc && pz.kparts == 1, "bstream: no plan for the sums-of-squares producer");
            BstreamArgs<T> f{};
            f.W = (T*)b.alloc((size_t)K * 256 * sizeof(T));
            f.X = (T*)b.alloc((size_t)R * 256 * sizeof(T));
            f.ldx = 256;
            f.R = R;
            f.N = K;
            f.K = 256;
            f.Yf = (float*)b.alloc((size_t)R * K * 4);
            f.ldy = K;
            f.res = xd;
            f.ldr = o.ldx;
            T* xf = b.upload<T>(o.x, (size_t)R * o.ldx);
            f.res_out = xf;
            f.ldro = o.ldx;
            float* ss = (float*)b.alloc((size_t)R * (K / 16) * 4);
            f.ss_out = ss;
            f.tickets = tickets;
            FMCHECK(launch_bstream<T>(s, f, EPI_SLABFIN, pz), "bstream: no kernel for the producer's plan");
            HIPCHK(hipGetLastError());
            a.X = xf;
            a.pro = PRO_PRENORM;
            a.ss_in = ss;
            a.nw = b.upload<T>(o.nw, (size_t)K);
        }
    }
    InOut<T> yt(b, o.y, f32 ? 1 : (size_t)o.y_rows * o.ldy);
    InOut<float> yf(b, o.y, f32 ? (size_t)o.y_rows * o.ldy : 1);
    std::vector<float> one(1, 0.f);
    InOut<float> ss(b, o.epi == EPI_SLABFIN ? o.ss_out : one.data(), o.epi == EPI_SLABFIN ? (size_t)R * tiles : 1);
    a.ldy = o.ldy;
    if (o.epi == EPI_SLABFIN) {
        a.res = b.upload<T>(o.res, (size_t)R * o.ldr);
        a.ldr = o.ldr;
        a.res_out = yt.d;
        a.ldro = o.ldy;
        a.ss_out = ss.d;
        a.tickets = tickets;
        a.Yf = (float*)b.alloc((size_t)p.kparts * R * N * 4);  // K-part partials (scratch)
        a.ldy = N;
    } else if (f32) {
        a.Yf = yf.d;
    } else {
        a.Y = yt.d;
    }
    for (int i = 0; i < o.reps; ++i)
        FMCHECK(launch_bstream<T>(s, a, o.epi, p), "bstream: no kernel for the plan");
    HIPCHK(hipGetLastError());
    if (f32) yf.get(s);
    else yt.get(s);
    if (o.epi == EPI_SLABFIN) ss.get(s);
    const int pl[7] = {p.acc, p.kparts, p.nw, p.spw, p.tpi, p.ntm, p.grid};
    memcpy(o.plan, pl, sizeof(pl));
    *o.dirty = count_nonzero(tickets, ntk, s);
}

struct FinalizeOp {
    const float* slab;
    int kparts, lds;
    const float *bias, *res;
    int ldr;
    const float *nw, *wscale;
    float eps;
    int d, R;
    float* x_out;
    int ldx, x_rows;
    float* xn_out;
    int ldxn, xn_rows, reps;
    int *split, *err, *dirty;
};

template <typename T> void finalize_op_t(hipStream_t s, const FinalizeOp& o) {
    DevBufs b(s);
    const int R = o.R, d = o.d;
    FinalizeArgs<T> f{};
    float* slab = (float*)b.alloc((size_t)o.kparts * R * o.lds * 4);
    b.put(slab, o.slab, (size_t)o.kparts * R * o.lds * 4);
    f.slab = slab;
    f.kparts = o.kparts;
    f.lds = o.lds;
    if (o.bias) f.bias = b.upload<T>(o.bias, (size_t)d);
    f.res = b.upload<T>(o.res, (size_t)R * o.ldr);
    f.ldr = o.ldr;
    InOut<T> xo(b, o.x_out, (size_t)o.x_rows * o.ldx);
    f.x_out = xo.d;
    f.ldx = o.ldx;
    std::vector<float> one(1, 0.f);
    InOut<T> xn(b, o.nw ? o.xn_out : one.data(), o.nw ? (size_t)o.xn_rows * o.ldxn : 1);
    if (o.nw) {
        f.nw = b.upload<T>(o.nw, (size_t)d);
        f.xn_out = xn.d;
        f.ldxn = o.ldxn;
    }
    f.eps = o.eps;
    f.d = d;
    f.R = R;
    if (o.wscale) f.wscale = b.upload<T>(o.wscale, (size_t)d);
    // the split form as the batched frame arms it (fm_tune fin_split): counters, partial sums, err word
    const int ch = fm_tuning().fin_split;
    int* cnt = (int*)b.alloc((size_t)2 * R * 4);
    int* err = (int*)b.alloc(4);
    if (ch > 1) {
        f.ch = ch;
        f.cnt = cnt;
        f.ss_part = (float*)b.alloc((size_t)R * ch * 4);
        f.err = err;
    }
    *o.split = ch > 1 && R * ch <= 1024 && (d / 8 + ch - 1) / ch <= 64;  // launch_finalize_norm's own condition
    for (int i = 0; i < o.reps; ++i) launch_finalize_norm<T>(s, f);
    HIPCHK(hipGetLastError());
    xo.get(s);
    if (o.nw) xn.get(s);
    HIPCHK(hipMemcpyAsync(o.err, err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *o.dirty = count_nonzero(cnt, (size_t)2 * R, s);
}

struct RowGemvOp {
    int kind, q8;
    const float *w, *bias, *nw;
    float eps;
    const float* x;
    int x_rows, ldx;
    const float* res;
    int res_rows, ldr;
    const int32_t* idx;
    int idx_n, idx_col, N, K;
    float* y;
    int y_len, reps;
    int8_t* q_out;
    float* scale_out;
};

void rowgemv_op(hipStream_t s, const RowGemvOp& o) {
    DevBufs b(s);
    const int N = o.N, K = o.K;
    const bool f32 = o.kind == ROWGEMV_NORM_F32, fin = o.kind == ROWGEMV_FIN;
    RowGemvArgs a{};
    bf16_t* wd = b.upload<bf16_t>(o.w, (size_t)N * K);
    if (o.q8) {  // the int8 rule on the device, as fm_llm_set_quant applies it: codes row-major, bf16 row scales
        int8_t* dq = (int8_t*)b.alloc((size_t)N * K);
        bf16_t* ds = (bf16_t*)b.alloc((size_t)N * 2);
        launch_quant_rows<bf16_t>(s, wd, N, K, dq, ds);
        HIPCHK(hipGetLastError());
        a.Wq = dq;
        a.wscale = ds;
        if (o.q_out) {
            HIPCHK(hipMemcpyAsync(o.q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (o.scale_out) download<bf16_t>(ds, (size_t)N, o.scale_out, s);
    } else {
        a.W = wd;
    }
    a.X = b.upload<bf16_t>(o.x, (size_t)o.x_rows * o.ldx);
    a.ldx = o.ldx;
    if (o.bias) a.bias = b.upload<bf16_t>(o.bias, (size_t)N);
    if (o.nw) a.nw = b.upload<bf16_t>(o.nw, (size_t)K);
    a.eps = o.eps;
    int32_t* id = nullptr;
    if (o.idx) {
        id = (int32_t*)b.alloc((size_t)o.idx_n * 4);
        b.put(id, o.idx, (size_t)o.idx_n * 4);
    }
    if (fin) {
        a.res = b.upload<bf16_t>(o.res, (size_t)o.res_rows * o.ldr);
        a.ldr = o.ldr;
        a.residx = id;
        a.res_col = o.idx_col;
        a.res_rows = o.res_rows;
    } else {
        a.xidx = id;
        a.xcol = o.idx_col;
        a.xrows = o.x_rows;
    }
    a.N = N;
    a.K = K;
    InOut<bf16_t> yt(b, o.y, f32 ? 1 : (size_t)o.y_len);
    InOut<float> yf(b, o.y, f32 ? (size_t)o.y_len : 1);
    if (fin) a.res_out = yt.d;
    else if (f32) a.Yf = yf.d;
    else a.Y = yt.d;
    for (int i = 0; i < o.reps; ++i) launch_rowgemv(s, a, o.kind);
    HIPCHK(hipGetLastError());
    if (f32) yf.get(s);
    else yt.get(s);
}

// the two-row forms of launch_rowgemv (RowGemvArgs::xr = 2): x [2][K]; fin: row 0's residual res0 [N], row 1's
// row idx[idx_col] of res1 [res_rows][ldr] (row 0 of it without idx); y [2][y_ld] in/out
struct RowGemvPairOp {
    int kind;
    const float *w, *bias, *nw;
    float eps;
    const float *x, *res0, *res1;
    int res_rows, ldr;
    const int32_t* idx;
    int idx_n, idx_col, skip0, N, K;
    float* y;
    int y_ld;
};

void rowgemv_pair_op(hipStream_t s, const RowGemvPairOp& o) {
    DevBufs b(s);
    const int N = o.N, K = o.K;
    RowGemvArgs a{};
    a.W = b.upload<bf16_t>(o.w, (size_t)N * K);
    a.X = b.upload<bf16_t>(o.x, (size_t)2 * K);
    a.X1 = a.X + K;
    a.ldx = K;
    if (o.bias) a.bias = b.upload<bf16_t>(o.bias, (size_t)N);
    if (o.nw) a.nw = b.upload<bf16_t>(o.nw, (size_t)K);
    a.eps = o.eps;
    a.N = N;
    a.K = K;
    a.xr = 2;
    InOut<bf16_t> yt(b, o.y, (size_t)2 * o.y_ld);
    if (o.kind == ROWGEMV_FIN) {
        a.res = b.upload<bf16_t>(o.res0, (size_t)N);
        a.res1 = b.upload<bf16_t>(o.res1, (size_t)o.res_rows * o.ldr);
        a.ldr = o.ldr;
        if (o.idx) {
            int32_t* id = (int32_t*)b.alloc((size_t)o.idx_n * 4);
            b.put(id, o.idx, (size_t)o.idx_n * 4);
            a.residx = id;
            a.res_col = o.idx_col;
            a.res_rows = o.res_rows;
        }
        a.res_out = yt.d;
        a.res_out1 = yt.d + o.y_ld;
    } else {
        a.Y = yt.d;
        a.Y1 = yt.d + o.y_ld;
        a.skip0 = o.skip0;
    }
    launch_rowgemv(s, a, o.kind);
    HIPCHK(hipGetLastError());
    yt.get(s);
}

// the two-row forms on weight-only codes (fm_tune fast_pair_q): w quantised on the device by the model's rule (int8:
// launch_quant_rows; int4: launch_quant4 + launch_pack_q4_rows), then on the same device operands the two-row launch
// (y2 [2][y_ld]) and the one-row production launcher once per row (y1 [2][y_ld]; row 0 with skip0 > 0 still computes
// every output: the caller compares from skip0 on).  Both outputs in/out.
struct RowGemvPairQOp {
    int quant, gs, kind;
    const float *w, *nw;
    float eps;
    const float *x, *res0, *res1;
    int res_rows, ldr;
    const int32_t* idx;
    int idx_n, idx_col, skip0, N, K;
    float *y2, *y1;
    int y_ld;
    int8_t* q_out;
    float *scale_out, *zero_out;
};

void rowgemv_pair_q_op(hipStream_t s, const RowGemvPairQOp& o) {
    DevBufs b(s);
    const int N = o.N, K = o.K;
    const bool q4 = o.quant == FM_QUANT_INT4, fin = o.kind == ROWGEMV_FIN;
    RowGemvArgs a{};
    bf16_t* wd = b.upload<bf16_t>(o.w, (size_t)N * K);
    if (q4) {
        const int ng = K / o.gs;
        uint8_t* dq = (uint8_t*)b.alloc((size_t)N * K);
        uint32_t* dsz = (uint32_t*)b.alloc((size_t)N * ng * 4);
        uint32_t* words = (uint32_t*)b.alloc((size_t)N * K / 2);
        launch_quant4(s, wd, N, K, o.gs, dq, dsz);
        launch_pack_q4_rows(s, dq, N, K, words);
        HIPCHK(hipGetLastError());
        a.Wq4 = words;
        a.wsz = dsz;
        a.gs = o.gs;
        if (o.q_out) {
            HIPCHK(hipMemcpyAsync(o.q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (o.scale_out || o.zero_out) {
            std::vector<uint32_t> hs((size_t)N * ng);
            HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t i = 0; i < hs.size(); ++i) {
                const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
                if (o.scale_out) memcpy(&o.scale_out[i], &us, 4);
                if (o.zero_out) memcpy(&o.zero_out[i], &uz, 4);
            }
        }
    } else {
        int8_t* dq = (int8_t*)b.alloc((size_t)N * K);
        bf16_t* ds = (bf16_t*)b.alloc((size_t)N * 2);
        launch_quant_rows<bf16_t>(s, wd, N, K, dq, ds);
        HIPCHK(hipGetLastError());
        a.Wq = dq;
        a.wscale = ds;
        if (o.q_out) {
            HIPCHK(hipMemcpyAsync(o.q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (o.scale_out) download<bf16_t>(ds, (size_t)N, o.scale_out, s);
    }
    const bf16_t* X = b.upload<bf16_t>(o.x, (size_t)2 * K);
    a.ldx = K;
    if (o.nw) a.nw = b.upload<bf16_t>(o.nw, (size_t)K);
    a.eps = o.eps;
    a.N = N;
    a.K = K;
    const bf16_t *r0 = nullptr, *r1 = nullptr;
    int32_t* id = nullptr;
    if (fin) {
        r0 = b.upload<bf16_t>(o.res0, (size_t)N);
        r1 = b.upload<bf16_t>(o.res1, (size_t)o.res_rows * o.ldr);
        if (o.idx) {
            id = (int32_t*)b.alloc((size_t)o.idx_n * 4);
            b.put(id, o.idx, (size_t)o.idx_n * 4);
        }
    }
    InOut<bf16_t> y2(b, o.y2, (size_t)2 * o.y_ld), y1(b, o.y1, (size_t)2 * o.y_ld);
    {  // the two-row launch
        RowGemvArgs t = a;
        t.X = X;
        t.X1 = X + K;
        t.xr = 2;
        if (fin) {
            t.res = r0;
            t.res1 = r1;
            t.ldr = o.ldr;
            t.residx = id;
            t.res_col = o.idx_col;
            t.res_rows = id ? o.res_rows : 0;
            t.res_out = y2.d;
            t.res_out1 = y2.d + o.y_ld;
        } else {
            t.Y = y2.d;
            t.Y1 = y2.d + o.y_ld;
            t.skip0 = o.kind == ROWGEMV_NORM_STORE ? o.skip0 : 0;
        }
        launch_rowgemv(s, t, o.kind);
        HIPCHK(hipGetLastError());
    }
    for (int r = 0; r < 2; ++r) {  // the one-row production launcher, row by row
        RowGemvArgs t = a;
        t.X = X + (size_t)r * K;
        if (fin) {
            t.res = r ? r1 : r0;
            t.ldr = r ? o.ldr : N;
            if (r) {
                t.residx = id;
                t.res_col = o.idx_col;
                t.res_rows = id ? o.res_rows : 0;
            }
            t.res_out = y1.d + (size_t)r * o.y_ld;
        } else {
            t.Y = y1.d + (size_t)r * o.y_ld;
        }
        launch_rowgemv(s, t, o.kind);
        HIPCHK(hipGetLastError());
    }
    y2.get(s);
    y1.get(s);
}

void prompt_skinny_op(hipStream_t s, const float* w, const float* x, int ldx, int R, int N, int K, int ks, int act,
                      float* out, int out_rows, int ldo, int reps) {
    DevBufs b(s);
    PromptSkinnyArgs p{};
    p.w = upload_packed<bf16_t>(b, w, N, K);
    p.x = b.upload<bf16_t>(x, (size_t)R * ldx);
    p.ldx = ldx;
    p.R = R;
    p.N = N;
    p.K = K;
    InOut<float> slab(b, out, act ? 1 : (size_t)out_rows * N);
    InOut<bf16_t> av(b, out, act ? (size_t)out_rows * ldo : 1);
    p.slab = slab.d;  // (the launcher wants it set in the direct form too; the kernel does not write it then)
    if (act) {
        p.act = av.d;
        p.lda = ldo;
    }
    for (int i = 0; i < reps; ++i) launch_prompt_skinny(s, p, ks);
    HIPCHK(hipGetLastError());
    if (act) av.get(s);
    else slab.get(s);
}

}  // namespace

extern "C" {

int fm_op_rmsnorm(int device, int precision, int mode, const float* x, const float* w, int R, int d, float eps,
                  float* y) {
    return fm_guard([&] {
        FMCHECK(x && w && y, "null argument");
        FMCHECK(mode >= 0 && mode <= 2, "mode must be 0 (PRO_NORM), 1 (PRO_PRENORM) or 2 (row kernel)");
        FMCHECK(R >= 1 && d >= 32 && d % 32 == 0, "need R >= 1 and d a multiple of 32");
        FMCHECK(mode == 2 || (R <= 8 && d <= 4096), "GEMV prologue modes need R <= 8 and d <= 4096");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            rmsnorm_t<bf16_t>(g.s, mode, x, w, R, d, eps, y);
        else
            rmsnorm_t<float>(g.s, mode, x, w, R, d, eps, y);
    });
}

int fm_op_prompt_attn(int device, int precision, int kernel, const float* q, int R, int nh, int nkv, int hd, int pos0,
                      const float* kcache, const float* vcache, int S, float* out) {
    return fm_guard([&] {
        FMCHECK(q && kcache && vcache && out, "null argument");
        FMCHECK(kernel == 0 || kernel == 1, "kernel must be 0 (split + combine) or 1 (attn_prefill_kernel)");
        FMCHECK(R >= 1 && R <= 1024 && nh % nkv == 0 && pos0 >= 0 && pos0 + R <= S, "bad rows / positions");
        FMCHECK(kernel == 0 || (precision == FM_PREC_BF16 && hd == 128 && nh / nkv <= 4),
                "attn_prefill_kernel: bf16, head_dim 128, at most 4 q heads per kv head");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            prompt_attn_t<bf16_t>(g.s, kernel, q, R, nh, nkv, hd, pos0, kcache, vcache, S, out);
        else
            prompt_attn_t<float>(g.s, kernel, q, R, nh, nkv, hd, pos0, kcache, vcache, S, out);
    });
}

int fm_op_decode_attn(int device, int precision, int kernel, const float* qkv, int R, int nh, int nkv, int hd,
                      const float* qn, const float* kn, int qk_norm, float eps, float rope_base, const int* pos,
                      const float* kcache, const float* vcache, int S, int min_split, float* out, float* kc_out,
                      float* vc_out) {
    return fm_guard([&] {
        FMCHECK(qkv && pos && kcache && vcache && out && kc_out && vc_out, "null argument");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(kernel == 0 || kernel == 2 || kernel == 3, "kernel must be 0 (attn_decode2), 2 (attn_dec3) or 3 (attn_fd)");
        FMCHECK(R >= 1 && R <= 64 && nh >= 1 && nkv >= 1 && nh % nkv == 0, "bad rows / head counts");
        FMCHECK(hd >= 32 && hd <= 128 && hd % 32 == 0, "head_dim a multiple of 32 up to 128");
        FMCHECK(S >= 16 && S <= 65536 && min_split >= 16 && min_split % 16 == 0, "bad S / min_split");
        for (int r = 0; r < R; ++r) FMCHECK(pos[r] >= 0 && pos[r] < S, "position outside the cache");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            decode_attn_t<bf16_t>(g.s, kernel, qkv, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, pos, kcache, vcache,
                                  S, min_split, out, kc_out, vc_out);
        else
            decode_attn_t<float>(g.s, kernel, qkv, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, pos, kcache, vcache,
                                 S, min_split, out, kc_out, vc_out);
    });
}

// rows in distinct slots of [0, nslots), positions (if given) inside the cache, a layer of the cache
static void check_slot_rows(int R, const int* row_slot, const int* row_pos, int nslots, int layers, int layer, int S) {
    FMCHECK(row_slot && nslots >= 1 && layers >= 1 && layer >= 0 && layer < layers, "bad slots / layers");
    for (int r = 0; r < R; ++r) {
        FMCHECK(row_slot[r] >= 0 && row_slot[r] < nslots, "row_slot outside the cache");
        FMCHECK(!row_pos || (row_pos[r] >= 0 && row_pos[r] < S), "position outside the cache");
    }
}

int fm_op_decode_attn_ex(int device, int precision, int kernel, const float* qkv, const float* slab, int kp,
                         const float* bias, int R, int nh, int nkv, int hd, const float* qn, const float* kn,
                         int qk_norm, float eps, float rope_base, const int* row_slot, const int* pos, int nslots,
                         int layers, int layer, float* kcache, float* vcache, int S, int cap, int nwb, int frame,
                         int reps, float* out, int* info) {
    return fm_guard([&] {
        FMCHECK((qkv != nullptr) != (slab != nullptr) && pos && kcache && vcache && out && info,
                "need qkv or slab (one of them), positions, caches, out and info");
        FMCHECK(!slab || (kp >= 1 && kp <= 16), "1 to 16 slab parts");
        FMCHECK(!bias || slab, "a bias goes with the slab form");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(frame || kernel == 0 || kernel == 2 || kernel == 3,
                "kernel must be 0 (attn_decode2), 2 (attn_dec3) or 3 (attn_fd)");
        FMCHECK(R >= 1 && R <= 64 && nh >= 1 && nkv >= 1 && nh % nkv == 0 && nh / nkv <= 16, "bad rows / head counts");
        FMCHECK(hd >= 32 && hd <= 128 && hd % 32 == 0, "head_dim a multiple of 32 up to 128");
        FMCHECK(S >= 16 && S <= 65536 && reps >= 1 && reps <= 4, "bad S / reps");
        FMCHECK(frame || (cap >= 16 && cap % 16 == 0 && (nwb == 4 || nwb == 8 || nwb == 16)), "bad cap / nwb");
        check_slot_rows(R, row_slot, pos, nslots, layers, layer, S);
        for (int r = 0; r < R; ++r)
            for (int q = 0; q < r; ++q) FMCHECK(row_slot[q] != row_slot[r], "two rows in one slot");
        StreamGuard g(device);
        const DecodeAttnEx o{kernel, qkv, slab, kp, bias, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, row_slot, pos,
                             nslots, layers, layer, kcache, vcache, S, cap, nwb, frame, reps, out, info};
        if (precision == FM_PREC_BF16)
            decode_attn_ex_t<bf16_t>(g.s, o);
        else
            decode_attn_ex_t<float>(g.s, o);
    });
}

int fm_op_prompt_attn_ex(int device, int precision, int kernel, const float* q, int R, int nh, int nkv, int hd,
                         const int* row_slot, const int* row_pos, int one_slot, int nslots, int layers, int layer,
                         const float* kcache, const float* vcache, int S, float* out) {
    return fm_guard([&] {
        FMCHECK(q && row_pos && kcache && vcache && out, "null argument");
        FMCHECK(kernel == 0 || kernel == 1, "kernel must be 0 (split + combine) or 1 (attn_prefill_kernel)");
        FMCHECK(R >= 1 && R <= ATTN_PIECE && nh >= 1 && nkv >= 1 && nh % nkv == 0, "bad rows / head counts");
        FMCHECK(hd >= 32 && hd <= 256 && hd % 32 == 0 && S >= 16 && S <= 65536, "bad head_dim / S");
        check_slot_rows(R, row_slot, row_pos, nslots, layers, layer, S);
        if (one_slot)
            for (int r = 1; r < R; ++r)
                FMCHECK(row_slot[r] == row_slot[0] && row_pos[r] == row_pos[0] + r, "one_slot: consecutive rows of one slot");
        FMCHECK(kernel == 0 || (one_slot && precision == FM_PREC_BF16 && hd == 128 && nh / nkv <= 4),
                "attn_prefill_kernel: rows of one slot, bf16, head_dim 128, at most 4 q heads per kv head");
        StreamGuard g(device);
        const SlotRows sr{row_slot, row_pos, nslots, layers, layer};
        if (precision == FM_PREC_BF16)
            prompt_attn_ex_t<bf16_t>(g.s, kernel, q, R, nh, nkv, hd, sr, one_slot, kcache, vcache, S, out);
        else
            prompt_attn_ex_t<float>(g.s, kernel, q, R, nh, nkv, hd, sr, one_slot, kcache, vcache, S, out);
    });
}

int fm_op_qk_rope_cache(int device, int precision, const float* qkv, const float* slab, int kp, const float* bias, int R,
                        int nh, int nkv, int hd, const float* qn, const float* kn, int qk_norm, float eps,
                        float rope_base, const int* row_slot, const int* row_pos, int fixed_pos, int nslots, int layers,
                        int layer, float* kcache, float* vcache, int S, float* q_out) {
    return fm_guard([&] {
        FMCHECK((qkv != nullptr) != (slab != nullptr) && kcache && vcache && q_out, "need qkv or slab (one of them), caches, q_out");
        FMCHECK(!slab || (kp >= 1 && kp <= 16), "1 to 16 slab parts");
        FMCHECK(!bias || slab, "a bias goes with the slab form");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(R >= 1 && R <= 1024 && nh >= 1 && nkv >= 1, "bad rows / head counts");
        FMCHECK(hd >= 8 && hd <= 256 && hd % 8 == 0 && S >= 1 && S <= 65536, "bad head_dim / S");
        FMCHECK((fixed_pos >= 0 && fixed_pos < S) || (fixed_pos < 0 && row_pos), "fixed_pos inside the cache, or row positions");
        check_slot_rows(R, row_slot, fixed_pos >= 0 ? nullptr : row_pos, nslots, layers, layer, S);
        StreamGuard g(device);
        const SlotRows sr{row_slot, fixed_pos >= 0 ? nullptr : row_pos, nslots, layers, layer};
        if (precision == FM_PREC_BF16)
            qk_rope_cache_t<bf16_t>(g.s, qkv, slab, kp, bias, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, sr, fixed_pos,
                                    kcache, vcache, S, q_out);
        else
            qk_rope_cache_t<float>(g.s, qkv, slab, kp, bias, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, sr, fixed_pos,
                                   kcache, vcache, S, q_out);
    });
}

int fm_op_fast_attn(int device, int precision, int kernel, const float* qkv, int R, int nh, int nkv, int hd,
                    const float* qn, const float* kn, int qk_norm, float eps, float rope_base, const int* row_slot,
                    int cpos, int nslots, int layers, int layer, float* kcache, float* vcache, int S, float* out) {
    return fm_guard([&] {
        FMCHECK(qkv && kcache && vcache && out, "null argument");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(kernel >= 0 && kernel <= 3,
                "kernel must be 0 (fast_attn2), 1 (fast_attn2, noq), 2 (fast_attn_fused) or 3 (qk_rope_cache + fast_attn)");
        FMCHECK(R >= 1 && R <= 64 && nh >= 1 && nkv >= 1 && nh % nkv == 0, "bad rows / head counts");
        FMCHECK(hd >= 8 && hd <= 256 && hd % 8 == 0, "head_dim a multiple of 8 up to 256");
        FMCHECK(S >= 1 && S <= 63 && cpos >= 0 && cpos < S, "1 to 63 codebooks, cpos among them");
        FMCHECK(kernel > 1 || cpos < 16, "fast_attn2 positions are < 16");
        FMCHECK(kernel != 1 || cpos == 0, "noq is the codebook-0 form");
        FMCHECK(kernel != 2 || (size_t)2 * S * hd * 4 + (size_t)4 * hd * 4 + 1024 <= 64 * 1024, "fast_attn_fused: LDS tile too large");
        check_slot_rows(R, row_slot, nullptr, nslots, layers, layer, S);
        for (int r = 0; r < R; ++r)
            for (int q = 0; q < r; ++q) FMCHECK(row_slot[q] != row_slot[r], "two rows in one slot");
        StreamGuard g(device);
        const SlotRows sr{row_slot, nullptr, nslots, layers, layer};
        if (precision == FM_PREC_BF16)
            fast_attn_t<bf16_t>(g.s, kernel, qkv, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, sr, cpos, kcache, vcache, S, out);
        else
            fast_attn_t<float>(g.s, kernel, qkv, R, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, sr, cpos, kcache, vcache, S, out);
    });
}

int fm_op_fattn_wo(int device, int quant, int gs, int fused, const float* qkv, const float* qtab, int qrows,
                   const int32_t* idx, int idx_n, int idx_col, int nh, int nkv, int hd, const float* qn, const float* kn,
                   int qk_norm, float eps, float rope_base, int slot, int cpos, int nslots, int layers, int layer,
                   float* kcache, float* vcache, int S, const float* w, const float* bias, const float* res,
                   int res_rows, int ldr, const float* res0, int N, int kv0, int pair, int ilp, int gen, int pos0,
                   const uint32_t* xt_init, float* y, int* status) {
    return fm_guard([&] {
        FMCHECK(qkv && kcache && vcache && w && res && y && status, "null argument");
        FMCHECK(quant == FM_QUANT_NONE || quant == FM_QUANT_INT8 || quant == FM_QUANT_INT4, "bad quant");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(nh >= 1 && nkv >= 1 && nh % nkv == 0 && hd >= 8 && hd <= 128 && hd % 8 == 0, "bad heads / head_dim");
        FMCHECK(S >= 1 && S <= 63 && cpos >= 0 && cpos < S && N >= 16 && N % 16 == 0, "bad S / cpos / N");
        FMCHECK(quant == FM_QUANT_NONE || !bias, "the int8 / int4 row forms take no bias");
        FMCHECK(quant != FM_QUANT_INT4 || (gs >= 8 && gs % 8 == 0 && (nh * hd) % gs == 0), "bad int4 group size");
        FMCHECK(!idx || (idx_n >= 1 && idx_col >= 0 && idx_col < idx_n), "bad index column");
        FMCHECK(res_rows >= 1 && ldr >= N && gen >= 1 && gen <= 40 && pos0 >= 0, "bad residual table / gen / position");
        FMCHECK(!qtab || (idx && !kv0 && qrows >= 1 && qrows == res_rows), "the table form is gathered by the residual's index");
        FMCHECK(!kv0 || (!idx && cpos == 0), "the K / V-only form runs at codebook 0, no gather");
        FMCHECK(pair >= 0 && pair <= 2, "pair must be 0, 1 or 2");
        FMCHECK(!pair || (fused && !kv0 && cpos == 1 && (qtab != nullptr) == (idx != nullptr) &&
                          (pair == 1 ? res0 != nullptr : !qtab)),
                "pair form: fused, positions 0 and 1, row 0's residual (pair 1), no table in the last layer (pair 2)");
        check_slot_rows(1, &slot, nullptr, nslots, layers, layer, S);
        StreamGuard g(device);
        const FattnWoOp o{quant, gs, fused, qkv, qtab, qrows, idx, idx_n, idx_col, nh, nkv, hd, qn, kn, qk_norm, eps,
                          rope_base, slot, cpos, nslots, layers, layer, kcache, vcache, S, w, bias, res, res_rows, ldr,
                          res0, N, kv0, pair, ilp, gen, pos0, xt_init, y, status};
        fattn_wo_op(g.s, o);
    });
}

int fm_op_slow_attn_wo(int device, int fused, int rp, const float* qkv, int nh, int nkv, int hd, const float* qn,
                       const float* kn, int qk_norm, float eps, float rope_base, const int32_t* slots, const int32_t* pos,
                       const int32_t* gens, int nrun, int restore, int nslots, int layers, int layer, const float* kcache,
                       const float* vcache, int S, const float* w, const float* bias, const float* res, int N,
                       const uint32_t* xt_init, float* y, float* k_rows, float* v_rows, int* status) {
    return fm_guard([&] {
        FMCHECK(qkv && slots && pos && gens && kcache && vcache && w && res && y && k_rows && v_rows && status, "null argument");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(nh >= 1 && nkv >= 1 && nh % nkv == 0 && hd >= 8 && hd <= 128 && hd % 8 == 0, "bad heads / head_dim");
        FMCHECK(S >= 16 && S % 16 == 0 && S <= 65536 && N >= 16 && N % 16 == 0 && nrun >= 1 && nrun <= 4096, "bad S / N / runs");
        FMCHECK(rp == 2 || rp == 4, "rp must be 2 or 4");
        for (int i = 0; i < nrun; ++i) {
            FMCHECK(pos[i] >= 0 && pos[i] < S && gens[i] >= 1 && gens[i] <= 40, "bad position / gen");
            check_slot_rows(1, &slots[i], nullptr, nslots, layers, layer, S);
        }
        StreamGuard g(device);
        const SlowAttnWoOp o{FM_QUANT_NONE, 0, nullptr, nullptr, nullptr, fused, rp, qkv, nh, nkv, hd, qn, kn, qk_norm, eps,
                             rope_base, slots, pos, gens, nrun, restore, nslots, layers, layer, kcache, vcache, S, w, bias,
                             res, N, xt_init, y, k_rows, v_rows, status};
        slow_attn_wo_op(g.s, o);
    });
}

int fm_op_slow_attn_wo_q(int device, int quant, int gs, int fused, int rp, const float* qkv, int nh, int nkv, int hd,
                         const float* qn, const float* kn, int qk_norm, float eps, float rope_base, const int32_t* slots,
                         const int32_t* pos, const int32_t* gens, int nrun, int restore, int nslots, int layers, int layer,
                         const float* kcache, const float* vcache, int S, const float* w, const float* bias,
                         const float* res, int N, const uint32_t* xt_init, float* y, float* k_rows, float* v_rows,
                         int* status, int8_t* q_out, float* scale_out, float* zero_out) {
    return fm_guard([&] {
        FMCHECK(qkv && slots && pos && gens && kcache && vcache && w && res && y && k_rows && v_rows && status, "null argument");
        FMCHECK(quant == FM_QUANT_INT8 || quant == FM_QUANT_INT4, "quant must be int8 or int4");
        FMCHECK(!bias, "the int8 / int4 row forms take no bias");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(nh >= 1 && nkv >= 1 && nh % nkv == 0 && hd >= 8 && hd <= 128 && hd % 8 == 0, "bad heads / head_dim");
        FMCHECK(S >= 16 && S % 16 == 0 && S <= 65536 && N >= 16 && N % 16 == 0 && nrun >= 1 && nrun <= 4096, "bad S / N / runs");
        FMCHECK(rp == 2 || rp == 4, "rp must be 2 or 4");
        // what launch_rowgemv asks of the code forms: K in whole 512-k chunks at an instantiated depth, int4 groups of
        // whole 8-code words that divide K
        FMCHECK(rowgemv_u(nh * hd, 1) > 0, "the int8 / int4 row forms need K = nh * hd in whole 512-k chunks");
        FMCHECK(quant != FM_QUANT_INT4 || (gs >= 8 && gs % 8 == 0 && (nh * hd) % gs == 0), "bad int4 group size");
        for (int i = 0; i < nrun; ++i) {
            FMCHECK(pos[i] >= 0 && pos[i] < S && gens[i] >= 1 && gens[i] <= 40, "bad position / gen");
            check_slot_rows(1, &slots[i], nullptr, nslots, layers, layer, S);
        }
        StreamGuard g(device);
        const SlowAttnWoOp o{quant, gs, q_out, scale_out, zero_out, fused, rp, qkv, nh, nkv, hd, qn, kn, qk_norm, eps,
                             rope_base, slots, pos, gens, nrun, restore, nslots, layers, layer, kcache, vcache, S, w, nullptr,
                             res, N, xt_init, y, k_rows, v_rows, status};
        slow_attn_wo_op(g.s, o);
    });
}

int fm_op_qk_rope(int device, int precision, int kernel, const float* qkv, int nh, int nkv, int hd, const float* qn,
                  const float* kn, int qk_norm, float eps, float rope_base, int pos, float* q_out, float* k_out) {
    return fm_guard([&] {
        FMCHECK(qkv && q_out && k_out, "null argument");
        FMCHECK(!qk_norm || (qn && kn), "qk_norm needs both norm weights");
        FMCHECK(kernel >= 0 && kernel <= 3,
                "kernel must be 0 (slow attn_decode2), 1 (fast attn2), 2 (slow attn_dec3) or 3 (slow attn_fd)");
        FMCHECK(nh >= 1 && nkv >= 1 && nh % nkv == 0 && nh / nkv <= 16, "bad head counts");
        FMCHECK(hd >= 8 && hd <= 256 && hd % 8 == 0, "bad head_dim");
        FMCHECK(pos >= 0 && pos < 65536, "bad position");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            qk_rope_t<bf16_t>(g.s, kernel, qkv, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, pos, q_out, k_out);
        else
            qk_rope_t<float>(g.s, kernel, qkv, nh, nkv, hd, qn, kn, qk_norm, eps, rope_base, pos, q_out, k_out);
    });
}

int fm_op_embed(int device, int precision, const int32_t* tok, int R, const float* emb, int vocab,
                const float* cbemb, int dim, int num_codebooks, int codebook_size, int semantic_begin_id,
                int semantic_end_id, int scale_codebook_embeddings, float* x) {
    return fm_guard([&] {
        FMCHECK(tok && emb && cbemb && x && R >= 1 && dim % 8 == 0, "bad arguments");
        for (int r = 0; r < R; ++r) {
            FMCHECK(tok[(size_t)r * (num_codebooks + 1)] >= 0 && tok[(size_t)r * (num_codebooks + 1)] < vocab,
                    "token id out of range");
            for (int q = 1; q <= num_codebooks; ++q) {
                const int v = tok[(size_t)r * (num_codebooks + 1) + q];
                FMCHECK(v >= 0 && v < codebook_size, "codebook token out of range");
            }
        }
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            embed_t<bf16_t>(g.s, tok, R, emb, vocab, cbemb, dim, num_codebooks, codebook_size, semantic_begin_id,
                            semantic_end_id, scale_codebook_embeddings, x);
        else
            embed_t<float>(g.s, tok, R, emb, vocab, cbemb, dim, num_codebooks, codebook_size, semantic_begin_id,
                           semantic_end_id, scale_codebook_embeddings, x);
    });
}

// weight-only int4: the device quantizer (launch_quant4) on a caller bf16 matrix, then the decode
// GEMV on R rows of x three ways: the streamed int4 codes (when gs % 128 == 0), the bf16 weights it
// dequantised to, and (for reference) nothing else -- y_q4 / y_bf16 are [R][N] fp32 (EPI_F32)
int fm_op_quant4(int device, const float* w, int N, int K, int gs, uint8_t* q, float* scale, float* zero,
                 float* w_deq, const float* x, int R, float* y_q4, float* y_bf16) {
    return fm_guard([&] {
        FMCHECK(w && q && scale && zero && w_deq && N >= 1 && gs >= 2 && K % gs == 0, "bad arguments");
        FMCHECK(!x || (R >= 1 && R <= 8 && K % 32 == 0 && y_bf16), "bad GEMV arguments");
        StreamGuard g(device);
        DevBufs b(g.s);
        const int Np = (N + 15) / 16 * 16;
        bf16_t* dw = (bf16_t*)b.alloc((size_t)Np * K * 2);
        {
            bf16_t* t = b.upload<bf16_t>(w, (size_t)N * K);
            HIPCHK(hipMemcpyAsync(dw, t, (size_t)N * K * 2, hipMemcpyDeviceToDevice, g.s));
        }
        uint8_t* dq = (uint8_t*)b.alloc((size_t)Np * K);
        uint32_t* dsz = (uint32_t*)b.alloc((size_t)Np * (K / gs) * 4);
        launch_quant4(g.s, dw, N, K, gs, dq, dsz);
        HIPCHK(hipGetLastError());
        std::vector<uint16_t> hw((size_t)N * K);
        std::vector<uint32_t> hs((size_t)N * (K / gs));
        HIPCHK(hipMemcpyAsync(q, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipMemcpyAsync(hw.data(), dw, hw.size() * 2, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
        for (size_t i = 0; i < hw.size(); ++i) {
            const uint32_t u = (uint32_t)hw[i] << 16;
            memcpy(&w_deq[i], &u, 4);
        }
        for (size_t i = 0; i < hs.size(); ++i) {
            const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
            memcpy(&scale[i], &us, 4);
            memcpy(&zero[i], &uz, 4);
        }
        if (!x) return;
        // the decode GEMV: packed bf16 fragments of the dequantised weights, and the int4 stream
        bf16_t* pk = (bf16_t*)b.alloc((size_t)Np * K * 2);
        launch_pack<bf16_t>(g.s, dw, N, K, pk);
        bf16_t* dx = b.upload<bf16_t>(x, (size_t)R * K);
        float* dy = (float*)b.alloc((size_t)R * N * 4);
        int* tk = (int*)b.alloc((size_t)(Np / 16 + 16) * 4);
        GemvArgs<bf16_t> a{};
        a.W = pk;
        a.X = dx;
        a.ldx = K;
        a.R = R;
        a.N = N;
        a.K = K;
        a.Yf = dy;
        a.ldy = N;
        a.tickets = tk;
        a.eps = 1e-6f;
        launch_gemv<bf16_t>(g.s, a, PRO_PLAIN, EPI_F32, 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(y_bf16, dy, (size_t)R * N * 4, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
        if (y_q4 && gs % 128 == 0 && K % 128 == 0) {
            uint8_t* q4 = (uint8_t*)b.alloc((size_t)Np * K / 2);
            uint32_t* sz4 = (uint32_t*)b.alloc((size_t)(Np / 16) * (K / 128) * 16 * 4);
            launch_pack_q4(g.s, dq, N, K, q4);
            launch_pack_sz4(g.s, dsz, N, K, gs, sz4);
            a.Wq = q4;
            a.wsz = sz4;
            launch_gemv<bf16_t>(g.s, a, PRO_PLAIN, EPI_F32, 1);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(y_q4, dy, (size_t)R * N * 4, hipMemcpyDeviceToHost, g.s));
            HIPCHK(hipStreamSynchronize(g.s));
        }
    });
}

// weight-only int8 on the batched decode linear: the device quantizer (launch_quant_rows), then the
// same bstream plan / launch on the bf16 fragment copy of the codes and on the step-granular int8
// copy (BstreamArgs::Wq8).  Outputs as fp32: [R][N] (EPI_STORE / EPI_F32), [R][N / 2] (EPI_SWIGLU8),
// raw slabs [kparts][R][N] (EPI_SLAB).
int fm_op_batched_linear_q8(int device, const float* w, int N, int K, const float* x, int R, int epi,
                            float* y_q8, float* y_bf16, int* kparts, int8_t* q_out, float* scale_out) {
    return fm_guard([&] {
        FMCHECK(w && x && y_q8 && y_bf16 && N >= 1 && K >= 32 && K % 32 == 0 && R > 8 && R <= 32, "bad arguments");
        FMCHECK(epi == EPI_STORE || epi == EPI_F32 || epi == EPI_SLAB || (epi == EPI_SWIGLU8 && N % 16 == 0),
                "epi must be 0 (store), 3 (fp32), 4 (slabs) or 7 (SwiGLU, whole 16-row tiles)");
        StreamGuard g(device);
        DevBufs b(g.s);
        bsacc_init();
        const BstreamPlan p = bstream_plan(N, K, R, epi, 2);
        FMCHECK(bsacc_q8_ok(p, epi, PRO_PLAIN, 2), "no int8-code batched kernel for this shape");
        const int Np = (N + 15) / 16 * 16;
        bf16_t* dw = (bf16_t*)b.alloc((size_t)Np * K * 2);
        {
            bf16_t* t = b.upload<bf16_t>(w, (size_t)N * K);
            HIPCHK(hipMemcpyAsync(dw, t, (size_t)N * K * 2, hipMemcpyDeviceToDevice, g.s));
        }
        int8_t* dq = (int8_t*)b.alloc((size_t)Np * K);
        bf16_t* ds = (bf16_t*)b.alloc((size_t)Np * 2);
        launch_quant_rows<bf16_t>(g.s, dw, N, K, dq, ds);  // dw <- bf16(q)
        bf16_t* pk = (bf16_t*)b.alloc((size_t)Np * K * 2);
        launch_pack<bf16_t>(g.s, dw, N, K, pk);
        int8_t* pq = (int8_t*)b.alloc((size_t)Np * K);
        launch_pack_q8s(g.s, dq, N, K, pq);
        HIPCHK(hipGetLastError());
        if (q_out) HIPCHK(hipMemcpyAsync(q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
        if (scale_out) download<bf16_t>(ds, (size_t)N, scale_out, g.s);
        bf16_t* dx = b.upload<bf16_t>(x, (size_t)R * K);
        const int No = epi == EPI_SWIGLU8 ? N / 2 : N;
        const bool f32 = epi == EPI_F32 || epi == EPI_SLAB;
        const size_t ny = (size_t)(epi == EPI_SLAB ? p.kparts : 1) * R * No;
        for (int form = 0; form < 2; ++form) {
            void* dy = b.alloc(ny * (f32 ? 4 : 2));
            BstreamArgs<bf16_t> a{pk, nullptr, dx, K, R, N, K, f32 ? nullptr : (bf16_t*)dy, No, f32 ? (float*)dy : nullptr};
            a.wscale = ds;
            if (form) a.Wq8 = (const unsigned char*)pq;
            FMCHECK(launch_bstream<bf16_t>(g.s, a, epi, p), "bstream: no kernel for the plan");
            HIPCHK(hipGetLastError());
            float* out = form ? y_q8 : y_bf16;
            if (f32) {
                HIPCHK(hipMemcpyAsync(out, dy, ny * 4, hipMemcpyDeviceToHost, g.s));
                HIPCHK(hipStreamSynchronize(g.s));
            } else {
                download<bf16_t>((const bf16_t*)dy, ny, out, g.s);
            }
        }
        if (kparts) *kparts = p.kparts;
    });
}

// weight-only int4 on the batched decode linear: the device quantizer (launch_quant4, group size gs),
// then the same bstream plan / launch on the packed bf16 fragments of the weights it dequantised to
// and on the step-granular int4 copy with the (scale, zero) table (BstreamArgs::Wq4 / wsz).  Outputs
// as fm_op_batched_linear_q8's.
int fm_op_batched_linear_q4(int device, const float* w, int N, int K, int gs, const float* x, int R, int epi,
                            float* y_q4, float* y_bf16, int* kparts, uint8_t* q_out, float* scale_out,
                            float* zero_out, float* w_deq) {
    return fm_guard([&] {
        FMCHECK(w && x && y_q4 && y_bf16 && N >= 1 && K >= 128 && R > 8 && R <= 32, "bad arguments");
        FMCHECK(gs >= 128 && gs % 128 == 0 && K % 128 == 0 && K % gs == 0,
                "the int4 batched stream needs a group size and K in whole 128-k units, K a multiple of the group size");
        FMCHECK(epi == EPI_STORE || epi == EPI_F32 || epi == EPI_SLAB || (epi == EPI_SWIGLU8 && N % 16 == 0),
                "epi must be 0 (store), 3 (fp32), 4 (slabs) or 7 (SwiGLU, whole 16-row tiles)");
        StreamGuard g(device);
        DevBufs b(g.s);
        bsacc_init();
        const BstreamPlan p = bstream_plan(N, K, R, epi, 2);
        FMCHECK(bsacc_q4_ok(p, epi, PRO_PLAIN, 2, K), "no int4-code batched kernel for this shape");
        const int Np = (N + 15) / 16 * 16, ng = K / gs;
        bf16_t* dw = (bf16_t*)b.alloc((size_t)Np * K * 2);
        {
            bf16_t* t = b.upload<bf16_t>(w, (size_t)N * K);
            HIPCHK(hipMemcpyAsync(dw, t, (size_t)N * K * 2, hipMemcpyDeviceToDevice, g.s));
        }
        uint8_t* dq = (uint8_t*)b.alloc((size_t)Np * K);
        uint32_t* dsz = (uint32_t*)b.alloc((size_t)Np * ng * 4);
        launch_quant4(g.s, dw, N, K, gs, dq, dsz);  // dw <- bf16(fma(q - 8, scale, zero))
        bf16_t* pk = (bf16_t*)b.alloc((size_t)Np * K * 2);
        launch_pack<bf16_t>(g.s, dw, N, K, pk);
        uint32_t* pq = (uint32_t*)b.alloc((size_t)Np * K / 2);
        launch_pack_q4s(g.s, dq, N, K, pq);
        uint32_t* sz4 = (uint32_t*)b.alloc((size_t)(Np / 16) * (K / 128) * 16 * 4);
        launch_pack_sz4(g.s, dsz, N, K, gs, sz4);
        HIPCHK(hipGetLastError());
        if (q_out) HIPCHK(hipMemcpyAsync(q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
        if (w_deq) download<bf16_t>(dw, (size_t)N * K, w_deq, g.s);
        if (scale_out || zero_out) {
            std::vector<uint32_t> hs((size_t)N * ng);
            HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, g.s));
            HIPCHK(hipStreamSynchronize(g.s));
            for (size_t i = 0; i < hs.size(); ++i) {
                const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
                if (scale_out) memcpy(&scale_out[i], &us, 4);
                if (zero_out) memcpy(&zero_out[i], &uz, 4);
            }
        }
        bf16_t* dx = b.upload<bf16_t>(x, (size_t)R * K);
        const int No = epi == EPI_SWIGLU8 ? N / 2 : N;
        const bool f32 = epi == EPI_F32 || epi == EPI_SLAB;
        const size_t ny = (size_t)(epi == EPI_SLAB ? p.kparts : 1) * R * No;
        for (int form = 0; form < 2; ++form) {
            void* dy = b.alloc(ny * (f32 ? 4 : 2));
            BstreamArgs<bf16_t> a{pk, nullptr, dx, K, R, N, K, f32 ? nullptr : (bf16_t*)dy, No, f32 ? (float*)dy : nullptr};
            if (form) {
                a.Wq4 = pq;
                a.wsz = sz4;
            }
            FMCHECK(launch_bstream<bf16_t>(g.s, a, epi, p), "bstream: no kernel for the plan");
            HIPCHK(hipGetLastError());
            float* out = form ? y_q4 : y_bf16;
            if (f32) {
                HIPCHK(hipMemcpyAsync(out, dy, ny * 4, hipMemcpyDeviceToHost, g.s));
                HIPCHK(hipStreamSynchronize(g.s));
            } else {
                download<bf16_t>((const bf16_t*)dy, ny, out, g.s);
            }
        }
        if (kparts) *kparts = p.kparts;
    });
}

// weight-only int8 / int4 on launch_linear (the 16-row MFMA tile kernel, any R): the model's own device quantizer,
// then the same launch on the packed bf16 fragments of the quantised weights (y_bf16) and on linear_kernel's
// code-reading form -- the step-granular codes alone, no bf16 weight (y_q).  Outputs in/out like fm_op_linear's.
int fm_op_linear_q(int device, int quant, int gs, const float* w, int N, int K, const float* bias, const float* x,
                   int ldx, const float* res, int ldr, int R, int epi, int split, float* y_q, float* y_bf16, int ldy,
                   int y_rows, int reps, int* ksb, int* dirty, int8_t* q_out, float* scale_out, float* zero_out) {
    return fm_guard([&] {
        FMCHECK(w && x && y_q && y_bf16 && ksb && dirty, "null argument");
        FMCHECK(quant == FM_QUANT_INT8 || quant == FM_QUANT_INT4, "quant must be int8 or int4");
        FMCHECK(epi == EPI_STORE || epi == EPI_RESID || epi == EPI_F32, "epi must be 0 (store), 1 (residual) or 3 (fp32)");
        FMCHECK((epi == EPI_RESID) == (res != nullptr), "res goes with EPI_RESID (1) only");
        FMCHECK(R >= 1 && R <= 1024 && N >= 1 && K >= 32 && K % 32 == 0, "need 1 <= R <= 1024, N >= 1, K a multiple of 32");
        FMCHECK(ldx >= K && ldx % 8 == 0 && ldy >= N && y_rows >= R && (!res || ldr >= N), "bad row strides / output rows");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        const bool q4 = quant == FM_QUANT_INT4;
        FMCHECK(!q4 || (gs >= 128 && gs % 128 == 0 && K % 128 == 0 && K % gs == 0),
                "the int4 code form needs a group size and K in whole 128-k units, K a multiple of the group size");
        FMCHECK(!q4 || !bias, "the int4 linears are bias-free");
        StreamGuard g(device);
        DevBufs b(g.s);
        const int Np = (N + 15) / 16 * 16, ng = q4 ? K / gs : 1;
        bf16_t* dw = (bf16_t*)b.alloc((size_t)Np * K * 2);
        {
            bf16_t* t = b.upload<bf16_t>(w, (size_t)N * K);
            HIPCHK(hipMemcpyAsync(dw, t, (size_t)N * K * 2, hipMemcpyDeviceToDevice, g.s));
        }
        uint8_t* dq = (uint8_t*)b.alloc((size_t)Np * K);
        LinearArgs<bf16_t> a{};
        void* pq = nullptr;       // the step-granular codes
        uint32_t* sz4 = nullptr;  // int4: their (scale, zero) table
        if (q4) {
            uint32_t* dsz = (uint32_t*)b.alloc((size_t)Np * ng * 4);
            launch_quant4(g.s, dw, N, K, gs, dq, dsz);  // dw <- bf16(fma(q - 8, scale, zero))
            pq = b.alloc((size_t)Np * K / 2);
            launch_pack_q4s(g.s, dq, N, K, (uint32_t*)pq);
            sz4 = (uint32_t*)b.alloc((size_t)(Np / 16) * (K / 128) * 16 * 4);
            launch_pack_sz4(g.s, dsz, N, K, gs, sz4);
            HIPCHK(hipGetLastError());
            if (scale_out || zero_out) {
                std::vector<uint32_t> hs((size_t)N * ng);
                HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, g.s));
                HIPCHK(hipStreamSynchronize(g.s));
                for (size_t i = 0; i < hs.size(); ++i) {
                    const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
                    if (scale_out) memcpy(&scale_out[i], &us, 4);
                    if (zero_out) memcpy(&zero_out[i], &uz, 4);
                }
            }
        } else {
            bf16_t* ds = (bf16_t*)b.alloc((size_t)Np * 2);
            launch_quant_rows<bf16_t>(g.s, dw, N, K, (int8_t*)dq, ds);  // dw <- bf16(q)
            pq = b.alloc((size_t)Np * K);
            launch_pack_q8s(g.s, (const int8_t*)dq, N, K, (int8_t*)pq);
            HIPCHK(hipGetLastError());
            a.wscale = ds;
            if (scale_out) download<bf16_t>(ds, (size_t)N, scale_out, g.s);
        }
        if (q_out) HIPCHK(hipMemcpyAsync(q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
        bf16_t* pk = (bf16_t*)b.alloc((size_t)Np * K * 2);
        launch_pack<bf16_t>(g.s, dw, N, K, pk);
        HIPCHK(hipGetLastError());
        if (bias) a.bias = b.upload<bf16_t>(bias, (size_t)N);
        a.X = b.upload<bf16_t>(x, (size_t)R * ldx);
        a.ldx = ldx;
        a.R = R;
        a.N = N;
        a.K = K;
        a.ldy = ldy;
        if (epi == EPI_RESID) {
            a.res = b.upload<bf16_t>(res, (size_t)R * ldr);
            a.ldr = ldr;
        }
        const bool f32 = epi == EPI_F32;
        const int tiles = Np / 16;
        const bool can_split = split && R > 8 && R <= 64;  // as the batched decode frame offers it
        const int nk = linear_ksb(N, K, R, 1, can_split);
        int* tickets = (int*)b.alloc((size_t)tiles * 4);
        if (can_split) {
            a.part = (float*)b.alloc((size_t)nk * R * N * 4);
            a.tickets = tickets;
        }
        int left = 0;
        for (int form = 0; form < 2; ++form) {
            float* y = form ? y_q : y_bf16;
            InOut<bf16_t> yt(b, y, f32 ? 1 : (size_t)y_rows * ldy);
            InOut<float> yf(b, y, f32 ? (size_t)y_rows * ldy : 1);
            LinearArgs<bf16_t> l = a;
            l.Y = f32 ? nullptr : yt.d;
            l.Yf = f32 ? yf.d : nullptr;
            if (!form) {
                l.W = pk;
            } else if (q4) {
                l.Wq4s = (const uint32_t*)pq;
                l.wsz = sz4;
            } else {
                l.Wq8s = (const unsigned char*)pq;
            }
            for (int i = 0; i < reps; ++i) launch_linear<bf16_t>(g.s, l, epi);
            HIPCHK(hipGetLastError());
            if (f32) yf.get(g.s);
            else yt.get(g.s);
            left += count_nonzero(tickets, (size_t)tiles, g.s);
        }
        *ksb = nk;
        *dirty = left;
    });
}

// ---- the decode linears, one production launcher each (include/fishmi.h) -------------------------
int fm_op_linear(int device, int precision, int epi, const float* w, const float* w2, const float* bias,
                 const float* x, int ldx, const float* res, int ldr, int R, int N, int K, int split, float* y, int ldy,
                 int y_rows, int reps, int* ksb, int* dirty) {
    return fm_guard([&] {
        FMCHECK(w && x && y && ksb && dirty, "null argument");
        FMCHECK(epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SWIGLU || epi == EPI_F32, "epi must be 0..3");
        FMCHECK((epi == EPI_SWIGLU) == (w2 != nullptr), "w2 goes with EPI_SWIGLU (2) only");
        FMCHECK((epi == EPI_RESID) == (res != nullptr), "res goes with EPI_RESID (1) only");
        FMCHECK(R >= 1 && R <= 1024 && N >= 1 && K >= 32 && K % 32 == 0, "need 1 <= R <= 1024, N >= 1, K a multiple of 32");
        FMCHECK(ldx >= K && ldx % 8 == 0 && ldy >= N && y_rows >= R && (!res || ldr >= N), "bad row strides / output rows");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        StreamGuard g(device);
        if (precision == FM_PREC_BF16)
            linear_op_t<bf16_t>(g.s, epi, w, w2, bias, x, ldx, res, ldr, R, N, K, split, y, ldy, y_rows, reps, ksb, dirty);
        else
            linear_op_t<float>(g.s, epi, w, w2, bias, x, ldx, res, ldr, R, N, K, split, y, ldy, y_rows, reps, ksb, dirty);
    });
}

int fm_op_gemv(int device, int precision, int pro, int epi, int ksb, const float* w, const float* w2, const float* bias,
               const float* nw, float eps, const float* x, int ldx, const int32_t* idx, int idx_ld, int idx_col,
               int idx_rows, const float* res, int ldr, int ss_gran, int R, int N, int K, float* y, int ldy, int y_rows,
               float* ss_out, int reps, int* dirty) {
    return fm_guard([&] {
        FMCHECK(w && x && y && dirty, "null argument");
        const bool plain = pro == PRO_PLAIN, norm = pro == PRO_NORM, pre = pro == PRO_PRENORM;
        // the (prologue, epilogue) pairs launch_gemv dispatches (PRO_FATT needs attention state: not here)
        FMCHECK((plain && (epi == EPI_STORE || epi == EPI_SLABFIN || epi == EPI_F32 || epi == EPI_SLAB)) ||
                    (norm && (epi == EPI_STORE || epi == EPI_SWIGLU || epi == EPI_F32)) ||
                    (pre && (epi == EPI_STORE || epi == EPI_SWIGLU || epi == EPI_F32 || epi == EPI_SWIGLU8)),
                "no GEMV kernel for this prologue / epilogue");
        FMCHECK(R >= 1 && R <= 8 && N >= 1 && K >= 32 && K % 32 == 0, "need 1 <= R <= 8, N >= 1, K a multiple of 32");
        const bool slabs = epi == EPI_SLAB || epi == EPI_SLABFIN;
        FMCHECK(ksb >= 1 && ksb <= 16 && K % (32 * ksb) == 0 && (slabs || ksb == 1), "ksb: whole k-steps per slice; > 1 only into slabs");
        FMCHECK((epi == EPI_SWIGLU) == (w2 != nullptr), "w2 goes with EPI_SWIGLU (2) only");
        FMCHECK(plain == (nw == nullptr), "the norm weight goes with PRO_NORM / PRO_PRENORM");
        FMCHECK((epi != EPI_SLABFIN && epi != EPI_SWIGLU8) || N % 16 == 0, "EPI_SLABFIN / EPI_SWIGLU8 need whole 16-row tiles");
        FMCHECK(epi != EPI_SLABFIN || (res && ss_out && ldr >= N), "EPI_SLABFIN needs res and ss_out");
        FMCHECK(!norm || K <= 8192, "PRO_NORM stages at most 8192 columns");
        FMCHECK(!pre || (K <= 4096 && (ss_gran == 0 || (ss_gran == 1 && R == 1 && K <= 3 * 8 * 256) ||
                                       (ss_gran == 1 && R == 2 && epi == EPI_SWIGLU8 && precision == FM_PREC_BF16))),
                "PRO_PRENORM: K <= 4096; ss_gran 1 needs one row and K <= 6144 (bf16 epi 7: two rows too)");
        FMCHECK(!idx || ((norm || epi == EPI_SLABFIN) && idx_rows >= 1 && idx_ld >= 1 && idx_col >= 0 && idx_col < idx_ld),
                "a row gather needs PRO_NORM (x) or EPI_SLABFIN (res), its table's row count and a column of idx");
        FMCHECK(ldx >= K && ldx % 8 == 0 && ldy >= (epi == EPI_SWIGLU8 ? N / 2 : N), "bad row strides");
        FMCHECK(y_rows >= (epi == EPI_SLAB ? ksb * R : R) && reps >= 1 && reps <= 8, "too few output rows, or reps outside 1..8");
        FMCHECK(gemv_lds_bytes(R, K / ksb, precision == FM_PREC_BF16 ? 2 : 4) <= 160 * 1024, "the x slice does not fit LDS");
        GemvOp o{pro, epi, ksb, w, w2, bias, nw, eps, x, (idx && norm) ? idx_rows : R, ldx, idx, idx_ld, idx_col, idx_rows,
                 res, (idx && !norm) ? idx_rows : R, ldr, ss_gran, R, N, K, y, ldy, y_rows, ss_out, reps, dirty};
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) gemv_op_t<bf16_t>(g.s, o);
        else gemv_op_t<float>(g.s, o);
    });
}

int fm_op_rowgemv(int device, int kind, int q8, const float* w, const float* bias, const float* nw, float eps,
                  const float* x, int x_rows, int ldx, const float* res, int res_rows, int ldr, const int32_t* idx,
                  int idx_n, int idx_col, int N, int K, float* y, int y_len, int reps, int8_t* q_out, float* scale_out) {
    return fm_guard([&] {
        FMCHECK(w && x && y, "null argument");
        FMCHECK(kind >= ROWGEMV_FIN && kind <= ROWGEMV_NORM_F32, "kind must be 0 (fin), 1 (norm, store), 2 (norm, swiglu) or 3 (norm, f32)");
        const bool fin = kind == ROWGEMV_FIN;
        const int U = rowgemv_u(K, q8 ? 1 : 0);
        FMCHECK(U > 0 && (fin || U <= 8), "K: whole chunks of 256 (int8: 512), at most 12 per wave (norm kinds: 8)");
        const int rp = fin ? 2 : (kind == ROWGEMV_NORM_STORE && !q8 ? fm_tuning().row_qkv_rp : 8);
        FMCHECK(N >= rp && N % rp == 0, "N must be whole row blocks (fin 2, else 8; wqkv: fm_tune row_qkv_rp)");
        FMCHECK(fin == (nw == nullptr) && fin == (res != nullptr), "fin takes a residual, the other kinds a norm weight");
        FMCHECK(!bias || (!q8 && kind != ROWGEMV_NORM_SWIGLU), "no bias on int8 codes or with the SwiGLU kind");
        FMCHECK(x_rows >= 1 && ldx >= K && ldx % 8 == 0 && (!fin || (res_rows >= 1 && ldr >= N)), "bad tables / strides");
        FMCHECK(!idx || (idx_n >= 1 && idx_col >= 0 && idx_col < idx_n && kind != ROWGEMV_NORM_F32), "bad gather (none on the f32 kind)");
        FMCHECK(idx || ((fin || x_rows == 1) && (!fin || res_rows == 1)), "a table of several rows needs idx");
        FMCHECK(!fin || x_rows == 1, "fin does not gather x");
        FMCHECK(y_len >= (kind == ROWGEMV_NORM_SWIGLU ? N / 2 : N) && reps >= 1 && reps <= 8, "output too short, or reps outside 1..8");
        RowGemvOp o{kind, q8, w, bias, nw, eps, x, x_rows, ldx, res, res_rows, ldr, idx, idx_n, idx_col, N, K, y, y_len, reps,
                    q_out, scale_out};
        StreamGuard g(device);
        rowgemv_op(g.s, o);
    });
}

int fm_op_rowgemv_pair(int device, int kind, const float* w, const float* bias, const float* nw, float eps, const float* x,
                       const float* res0, const float* res1, int res_rows, int ldr, const int32_t* idx, int idx_n,
                       int idx_col, int skip0, int N, int K, float* y, int y_ld) {
    return fm_guard([&] {
        FMCHECK(w && x && y, "null argument");
        FMCHECK(kind == ROWGEMV_FIN || kind == ROWGEMV_NORM_STORE, "kind must be 0 (fin) or 1 (norm, store)");
        const bool fin = kind == ROWGEMV_FIN;
        FMCHECK(rowgemv_pair_ok(kind, K, fin && idx != nullptr), "no two-row form at this depth (K: whole chunks of 256)");
        const int rp = fin ? 2 : 8;
        FMCHECK(N >= rp && N % rp == 0 && y_ld >= N, "N must be whole row blocks (fin 2, else 8), y rows at least N wide");
        FMCHECK(fin == (nw == nullptr) && fin == (res0 != nullptr) && fin == (res1 != nullptr),
                "fin takes both residual rows, norm + store a norm weight");
        FMCHECK(!fin || (res_rows >= 1 && ldr >= N && (idx || res_rows == 1)), "bad residual table / stride");
        FMCHECK(!idx || (fin && idx_n >= 1 && idx_col >= 0 && idx_col < idx_n), "bad gather (fin only)");
        FMCHECK(fin || (skip0 >= 0 && skip0 <= N), "skip0 outside 0..N");
        RowGemvPairOp o{kind, w, bias, nw, eps, x, res0, res1, res_rows, ldr, idx, idx_n, idx_col, skip0, N, K, y, y_ld};
        StreamGuard g(device);
        rowgemv_pair_op(g.s, o);
    });
}

int fm_op_rowgemv_pair_q(int device, int quant, int gs, int kind, const float* w, const float* nw, float eps, const float* x,
                         const float* res0, const float* res1, int res_rows, int ldr, const int32_t* idx, int idx_n,
                         int idx_col, int skip0, int N, int K, float* y2, float* y1, int y_ld, int8_t* q_out, float* scale_out,
                         float* zero_out) {
    return fm_guard([&] {
        FMCHECK(w && x && y2 && y1, "null argument");
        FMCHECK(quant == FM_QUANT_INT8 || quant == FM_QUANT_INT4, "quant must be int8 or int4");
        const bool q4 = quant == FM_QUANT_INT4, fin = kind == ROWGEMV_FIN;
        FMCHECK(fin || kind == ROWGEMV_NORM_STORE || kind == ROWGEMV_NORM_SWIGLU, "kind must be 0 (fin), 1 (norm, store) or 2 (norm, swiglu)");
        FMCHECK(!q4 || (gs >= 8 && gs % 8 == 0 && K % gs == 0), "int4: a group size in whole 8-k lane runs that divides K");
        FMCHECK(rowgemv_pair_ok(kind, K, fin && idx != nullptr, q4 ? 2 : 1),
                "no two-row code form of this kind at this depth (K: whole chunks of 512; int8: fin only, at most 5 per wave; int4: "
                "fin at most 5, the norm kinds at most 3)");
        const int rp = fin ? 2 : 8;
        FMCHECK(N >= rp && N % rp == 0 && y_ld >= (kind == ROWGEMV_NORM_SWIGLU ? N / 2 : N),
                "N must be whole row blocks (fin 2, else 8), y rows at least as wide as the outputs");
        FMCHECK(fin == (nw == nullptr) && fin == (res0 != nullptr) && fin == (res1 != nullptr),
                "fin takes both residual rows, the norm kinds a norm weight");
        FMCHECK(!fin || (res_rows >= 1 && ldr >= N && (idx || res_rows == 1)), "bad residual table / stride");
        FMCHECK(!idx || (fin && idx_n >= 1 && idx_col >= 0 && idx_col < idx_n), "bad gather (fin only)");
        FMCHECK(kind != ROWGEMV_NORM_STORE || (skip0 >= 0 && skip0 <= N), "skip0 outside 0..N");
        RowGemvPairQOp o{quant, gs, kind, w, nw, eps, x, res0, res1, res_rows, ldr, idx, idx_n, idx_col, skip0, N, K, y2, y1, y_ld,
                         q_out, scale_out, zero_out};
        StreamGuard g(device);
        rowgemv_pair_q_op(g.s, o);
    });
}

// the tile kernel's two-row ss_gran 1 form on weight-only int8 codes (fm_tune fast_pair_q): w quantised on the device
// by the model's rule (launch_quant_rows) and packed by the model's launcher (launch_pack_q8); then on the same device
// operands the two-row launch (y2) and the one-row production launch once per row (y1)
int fm_op_gemv_pair_q(int device, int quant, int epi, const float* w, const float* nw, float eps, const float* x, int N,
                      int K, float* y2, int y2_rows, float* y1, int ldy, int8_t* q_out, float* scale_out) {
    return fm_guard([&] {
        FMCHECK(w && nw && x && y2 && y1, "null argument");
        FMCHECK(quant == FM_QUANT_INT8, "the two-row tile form exists on int8 codes (int4 models run these linears on the row GEMV)");
        FMCHECK(epi == EPI_STORE || epi == EPI_SWIGLU8, "epi must be 0 (store) or 7 (SwiGLU8)");
        FMCHECK(N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 && K <= 4096, "N in whole 16-row tiles, K in whole 64-k units, at most 4096");
        FMCHECK(ldy >= (epi == EPI_SWIGLU8 ? N / 2 : N) && y2_rows >= 2, "output rows too short or too few");
        StreamGuard g(device);
        DevBufs b(g.s);
        bf16_t* dw = b.upload<bf16_t>(w, (size_t)N * K);
        int8_t* dq = (int8_t*)b.alloc((size_t)N * K);
        bf16_t* ds = (bf16_t*)b.alloc((size_t)N * 2);
        launch_quant_rows<bf16_t>(g.s, dw, N, K, dq, ds);
        int8_t* pq = (int8_t*)b.alloc((size_t)N * K);
        launch_pack_q8(g.s, dq, N, K, pq);
        HIPCHK(hipGetLastError());
        if (q_out) {
            HIPCHK(hipMemcpyAsync(q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
            HIPCHK(hipStreamSynchronize(g.s));
        }
        if (scale_out) download<bf16_t>(ds, (size_t)N, scale_out, g.s);
        GemvArgs<bf16_t> a{};
        a.Wq = (const unsigned char*)pq;
        a.wscale = ds;
        a.nw = b.upload<bf16_t>(nw, (size_t)K);
        a.eps = eps;
        const bf16_t* X = b.upload<bf16_t>(x, (size_t)2 * K);
        a.ldx = K;
        a.N = N;
        a.K = K;
        a.ldy = ldy;
        a.ss_in = (float*)b.alloc((size_t)(K / 16) * 2 * 4);  // (set, never read under ss_gran 1)
        a.ss_gran = 1;
        a.tickets = (int*)b.alloc((size_t)(N / 16 + 16) * 4);
        InOut<bf16_t> o2(b, y2, (size_t)y2_rows * ldy), o1(b, y1, (size_t)2 * ldy);
        {
            GemvArgs<bf16_t> t = a;
            t.X = X;
            t.R = 2;
            t.Y = o2.d;
            launch_gemv<bf16_t>(g.s, t, PRO_PRENORM, epi, 1);
            HIPCHK(hipGetLastError());
        }
        for (int r = 0; r < 2; ++r) {
            GemvArgs<bf16_t> t = a;
            t.X = X + (size_t)r * K;
            t.R = 1;
            t.Y = o1.d + (size_t)r * ldy;
            launch_gemv<bf16_t>(g.s, t, PRO_PRENORM, epi, 1);
            HIPCHK(hipGetLastError());
        }
        o2.get(g.s);
        o1.get(g.s);
    });
}

int fm_op_bstream(int device, int precision, int pro, int epi, const float* w, const float* bias, const float* nw,
                  float eps, const float* x, int ldx, const float* res, int ldr, int R, int N, int K, float* y, int ldy,
                  int y_rows, float* ss_out, int reps, int* plan, int* dirty) {
    return fm_guard([&] {
        FMCHECK(w && x && y && plan && dirty, "null argument");
        FMCHECK(epi == EPI_STORE || epi == EPI_F32 || epi == EPI_SLAB || epi == EPI_SWIGLU8 || epi == EPI_SLABFIN,
                "epi must be 0 (store), 3 (fp32), 4 (slabs), 5 (slabs + finalise) or 7 (SwiGLU8)");
        FMCHECK(pro == PRO_PLAIN || (pro == PRO_PRENORM && nw && precision == FM_PREC_BF16 && K <= 3072 && K >= 256 &&
                                     (epi == EPI_STORE || epi == EPI_SWIGLU8)),
                "pro must be 0, or 3 (PRO_PRENORM: bf16, norm weight, 256 <= K <= 3072, STORE / SWIGLU8)");
        FMCHECK(R > 8 && R <= 32 && N >= 1 && K >= 32 && K % 32 == 0, "need 8 < R <= 32, N >= 1, K a multiple of 32");
        FMCHECK(epi != EPI_SWIGLU8 || N % 16 == 0, "SwiGLU8 needs whole interleaved tiles");
        FMCHECK(epi != EPI_SLABFIN || (res && ss_out && ldr >= N && precision == FM_PREC_BF16), "EPI_SLABFIN: bf16, res and ss_out");
        FMCHECK(ldx >= K && ldx % 8 == 0 && ldy >= (epi == EPI_SWIGLU8 ? N / 2 : N) && y_rows >= R, "bad row strides / output rows");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        BstreamOp o{pro, epi, w, bias, nw, eps, x, ldx, res, ldr, R, N, K, y, ldy, y_rows, ss_out, reps, plan, dirty};
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) bstream_op_t<bf16_t>(g.s, o);
        else bstream_op_t<float>(g.s, o);
    });
}

int fm_op_finalize_norm(int device, int precision, const float* slab, int kparts, int lds, const float* bias,
                        const float* res, int ldr, const float* nw, const float* wscale, float eps, int d, int R,
                        float* x_out, int ldx, int x_rows, float* xn_out, int ldxn, int xn_rows, int reps, int* split,
                        int* err, int* dirty) {
    return fm_guard([&] {
        FMCHECK(slab && res && x_out && split && err && dirty, "null argument");
        FMCHECK(kparts >= 1 && kparts <= 64 && R >= 1 && R <= 1024, "need 1 <= kparts <= 64, 1 <= R <= 1024");
        FMCHECK(d >= 8 && d % 8 == 0 && d <= 8192 && lds >= d && lds % 4 == 0, "d a multiple of 8 up to 8192, slab rows of lds >= d floats, lds % 4 == 0");
        FMCHECK(ldr >= d && ldr % 8 == 0 && ldx >= d && x_rows >= R, "bad row strides / output rows");
        FMCHECK(!nw || (xn_out && ldxn >= d && xn_rows >= R), "the norm needs its output");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        FinalizeOp o{slab, kparts, lds, bias, res, ldr, nw, wscale, eps, d, R, x_out, ldx, x_rows, xn_out, ldxn, xn_rows,
                     reps, split, err, dirty};
        StreamGuard g(device);
        if (precision == FM_PREC_BF16) finalize_op_t<bf16_t>(g.s, o);
        else finalize_op_t<float>(g.s, o);
    });
}

int fm_op_prompt_skinny(int device, const float* w, const float* x, int ldx, int R, int N, int K, int target, int act,
                        float* out, int out_rows, int ldo, int reps, int* ks) {
    return fm_guard([&] {
        FMCHECK(ks && N >= 16 && N % 16 == 0 && K >= 32 && K % 32 == 0 && target >= 1, "bad shape");
        *ks = prompt_skinny_ks(N, K, target);
        if (!out) return;  // the slice count alone (it sizes the caller's slab)
        FMCHECK(w && x, "null argument");
        FMCHECK(*ks >= 1, "K is too short for a slice of 8 k-steps");
        FMCHECK(R >= 1 && R <= 64 && ldx >= K && ldx % 8 == 0, "need 1 <= R <= 64 and 16-byte rows of ldx >= K");
        FMCHECK(act ? (*ks == 1 && ldo >= N / 2 && out_rows >= R) : (ldo == N && out_rows >= *ks * R),
                "direct SwiGLU: one slice, act [>= R][ldo >= N / 2]; else slabs [>= ks * R][N]");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        StreamGuard g(device);
        prompt_skinny_op(g.s, w, x, ldx, R, N, K, *ks, act, out, out_rows, ldo, reps);
    });
}

// weight-only int8 / int4 on launch_prompt_skinny: the model's own device quantizer and pack launchers, then the
// same launch on the packed bf16 fragments of the quantised weights (y_bf16) and on the kernel's code-reading
// form -- the step-granular codes alone (y_q).  Outputs in/out like fm_op_prompt_skinny's; with act the int8
// row scales apply in the SwiGLU (int4 has none: its fragments hold the dequantised values).
int fm_op_prompt_skinny_q(int device, int quant, int gs, const float* w, const float* x, int ldx, int R, int N, int K,
                          int target, int act, float* y_q, float* y_bf16, int out_rows, int ldo, int reps, int* ks,
                          int8_t* q_out, float* scale_out, float* zero_out) {
    return fm_guard([&] {
        FMCHECK(ks && w && x && y_q && y_bf16, "null argument");
        FMCHECK(quant == FM_QUANT_INT8 || quant == FM_QUANT_INT4, "quant must be int8 or int4");
        FMCHECK(N >= 16 && N % 16 == 0 && K >= 32 && K % 32 == 0 && target >= 1, "bad shape");
        const bool q4 = quant == FM_QUANT_INT4;
        FMCHECK(!q4 || (gs >= 128 && gs % 128 == 0 && K % 128 == 0 && K % gs == 0),
                "the int4 code form needs a group size and K in whole 128-k units, K a multiple of the group size");
        *ks = prompt_skinny_ks(N, K, target);
        FMCHECK(*ks >= 1, "K is too short for a slice of 8 k-steps");
        FMCHECK(R >= 1 && R <= 64 && ldx >= K && ldx % 8 == 0, "need 1 <= R <= 64 and 16-byte rows of ldx >= K");
        FMCHECK(act ? (*ks == 1 && ldo >= N / 2 && out_rows >= R) : (ldo == N && out_rows >= *ks * R),
                "direct SwiGLU: one slice, act [>= R][ldo >= N / 2]; else slabs [>= ks * R][N]");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        StreamGuard g(device);
        DevBufs b(g.s);
        const int ng = q4 ? K / gs : 1;
        bf16_t* dw = b.upload<bf16_t>(w, (size_t)N * K);  // (N is whole tiles: no padding rows)
        uint8_t* dq = (uint8_t*)b.alloc((size_t)N * K);
        PromptSkinnyArgs p{};
        p.x = b.upload<bf16_t>(x, (size_t)R * ldx);
        p.ldx = ldx;
        p.R = R;
        p.N = N;
        p.K = K;
        void* pq = nullptr;       // the step-granular codes
        uint32_t* sz4 = nullptr;  // int4: their (scale, zero) table
        if (q4) {
            uint32_t* dsz = (uint32_t*)b.alloc((size_t)N * ng * 4);
            launch_quant4(g.s, dw, N, K, gs, dq, dsz);  // dw <- bf16(fma(q - 8, scale, zero))
            pq = b.alloc((size_t)N * K / 2);
            launch_pack_q4s(g.s, dq, N, K, (uint32_t*)pq);
            sz4 = (uint32_t*)b.alloc((size_t)(N / 16) * (K / 128) * 16 * 4);
            launch_pack_sz4(g.s, dsz, N, K, gs, sz4);
            HIPCHK(hipGetLastError());
            if (scale_out || zero_out) {
                std::vector<uint32_t> hs((size_t)N * ng);
                HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, g.s));
                HIPCHK(hipStreamSynchronize(g.s));
                for (size_t i = 0; i < hs.size(); ++i) {
                    const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
                    if (scale_out) memcpy(&scale_out[i], &us, 4);
                    if (zero_out) memcpy(&zero_out[i], &uz, 4);
                }
            }
        } else {
            bf16_t* ds = (bf16_t*)b.alloc((size_t)N * 2);
            launch_quant_rows<bf16_t>(g.s, dw, N, K, (int8_t*)dq, ds);  // dw <- bf16(q)
            pq = b.alloc((size_t)N * K);
            launch_pack_q8s(g.s, (const int8_t*)dq, N, K, (int8_t*)pq);
            HIPCHK(hipGetLastError());
            if (act) p.wscale = ds;
            if (scale_out) download<bf16_t>(ds, (size_t)N, scale_out, g.s);
        }
        if (q_out) {
            HIPCHK(hipMemcpyAsync(q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
            HIPCHK(hipStreamSynchronize(g.s));
        }
        bf16_t* pk = (bf16_t*)b.alloc((size_t)N * K * 2);
        launch_pack<bf16_t>(g.s, dw, N, K, pk);
        HIPCHK(hipGetLastError());
        for (int form = 0; form < 2; ++form) {
            float* out = form ? y_q : y_bf16;
            InOut<float> slab(b, out, act ? 1 : (size_t)out_rows * N);
            InOut<bf16_t> av(b, out, act ? (size_t)out_rows * ldo : 1);
            PromptSkinnyArgs l = p;
            l.slab = slab.d;  // (the launcher wants it set in the direct form too; the kernel does not write it then)
            if (act) {
                l.act = av.d;
                l.lda = ldo;
            }
            if (!form) {
                l.w = pk;
            } else if (q4) {
                l.q4s = (const uint32_t*)pq;
                l.sz = sz4;
            } else {
                l.q8s = (const unsigned char*)pq;
            }
            for (int i = 0; i < reps; ++i) launch_prompt_skinny(g.s, l, *ks);
            HIPCHK(hipGetLastError());
            if (act) av.get(g.s);
            else slab.get(g.s);
        }
    });
}

// weight-only int8 / int4 on the tiled prompt GEMMs (launch_conv_gemm as Run::prompt_gemm calls it for a linear of
// more than 64 rows): the model's device quantizer and pack launchers, then the same call once on the packed bf16
// fragments of the quantised weights (y_bf16; int8: the row scales as ConvArgs::rscale) and once on the step-granular
// codes alone (y_q).  plan: what conv_plan picked for the call.
int fm_op_prompt_gemm_q(int device, int quant, int gs, const float* w, const float* bias, const float* x, int ldx, int R,
                        int N, int K, const float* res, int ldr, int ksplit, float* y_q, float* y_bf16, int out_rows,
                        int ldo, int reps, int* plan, int8_t* q_out, float* scale_out, float* zero_out) {
    return fm_guard([&] {
        FMCHECK(plan && w && x && y_q && y_bf16, "null argument");
        FMCHECK(quant == FM_QUANT_INT8 || quant == FM_QUANT_INT4, "quant must be int8 or int4");
        FMCHECK(N >= 16 && N % 16 == 0 && K >= 32 && K % 32 == 0, "bad shape");
        const bool q4 = quant == FM_QUANT_INT4;
        FMCHECK(!q4 || (gs >= 128 && gs % 128 == 0 && K % 128 == 0 && K % gs == 0),
                "the int4 code form needs a group size and K in whole 128-k units, K a multiple of the group size");
        FMCHECK(R >= 1 && R <= 4096 && ldx >= K && ldx % 8 == 0, "need 1 <= R <= 4096 and 16-byte rows of ldx >= K");
        FMCHECK(ldo >= N && out_rows >= R && (!res || ldr >= N), "output [>= R][ldo >= N], residual rows of ldr >= N");
        FMCHECK(ksplit >= 1 && ksplit <= 64 && K / 32 >= ksplit, "ksplit 1..64, at least one k-step per slice");
        FMCHECK(reps >= 1 && reps <= 8, "reps 1..8");
        StreamGuard g(device);
        DevBufs b(g.s);
        const int ng = q4 ? K / gs : 1;
        bf16_t* dw = b.upload<bf16_t>(w, (size_t)N * K);  // (N is whole tiles: no padding rows)
        uint8_t* dq = (uint8_t*)b.alloc((size_t)N * K);
        ConvArgs<bf16_t> c{};
        c.x = b.upload<bf16_t>(x, (size_t)R * ldx);
        c.ldx = ldx;
        c.Ci = K;
        c.Lq = R;
        c.Lx = R;
        c.Co = N;
        c.ntaps = 1;
        c.stride = 1;
        c.nphase = 1;
        c.bias = bias ? b.upload<bf16_t>(bias, (size_t)N) : nullptr;
        c.res = res ? b.upload<bf16_t>(res, (size_t)R * ldr) : nullptr;
        c.ldr = ldr;
        c.ldo = ldo;
        c.flags = CE_STORE | (bias ? CE_BIAS : 0) | (res ? CE_RES : 0);
        if (ksplit > 1) {  // rows in whole 64-row blocks, so the call is one segment
            c.ksplit = ksplit;
            c.slab_cap = (size_t)ksplit * FM_CEIL(R, 64) * 64 * N;
            c.slab = (float*)b.alloc(c.slab_cap * 4);
        }
        void* pq = nullptr;       // the step-granular codes
        uint32_t* sz4 = nullptr;  // int4: their (scale, zero) table
        if (q4) {
            uint32_t* dsz = (uint32_t*)b.alloc((size_t)N * ng * 4);
            launch_quant4(g.s, dw, N, K, gs, dq, dsz);  // dw <- bf16(fma(q - 8, scale, zero))
            pq = b.alloc((size_t)N * K / 2);
            launch_pack_q4s(g.s, dq, N, K, (uint32_t*)pq);
            sz4 = (uint32_t*)b.alloc((size_t)(N / 16) * (K / 128) * 16 * 4);
            launch_pack_sz4(g.s, dsz, N, K, gs, sz4);
            HIPCHK(hipGetLastError());
            if (scale_out || zero_out) {
                std::vector<uint32_t> hs((size_t)N * ng);
                HIPCHK(hipMemcpyAsync(hs.data(), dsz, hs.size() * 4, hipMemcpyDeviceToHost, g.s));
                HIPCHK(hipStreamSynchronize(g.s));
                for (size_t i = 0; i < hs.size(); ++i) {
                    const uint32_t us = hs[i] << 16, uz = hs[i] & 0xffff0000u;
                    if (scale_out) memcpy(&scale_out[i], &us, 4);
                    if (zero_out) memcpy(&zero_out[i], &uz, 4);
                }
            }
        } else {
            bf16_t* ds = (bf16_t*)b.alloc((size_t)N * 2);
            launch_quant_rows<bf16_t>(g.s, dw, N, K, (int8_t*)dq, ds);  // dw <- bf16(q)
            pq = b.alloc((size_t)N * K);
            launch_pack_q8s(g.s, (const int8_t*)dq, N, K, (int8_t*)pq);
            HIPCHK(hipGetLastError());
            c.rscale = ds;
            if (scale_out) download<bf16_t>(ds, (size_t)N, scale_out, g.s);
        }
        if (q_out) {
            HIPCHK(hipMemcpyAsync(q_out, dq, (size_t)N * K, hipMemcpyDeviceToHost, g.s));
            HIPCHK(hipStreamSynchronize(g.s));
        }
        bf16_t* pk = (bf16_t*)b.alloc((size_t)N * K * 2);
        launch_pack<bf16_t>(g.s, dw, N, K, pk);
        HIPCHK(hipGetLastError());
        for (int form = 0; form < 2; ++form) {
            InOut<bf16_t> out(b, form ? y_q : y_bf16, (size_t)out_rows * ldo);
            ConvArgs<bf16_t> l = c;
            l.out = out.d;
            if (!form) {
                l.w = pk;
            } else if (q4) {
                l.q4s = (const uint32_t*)pq;
                l.sz = sz4;
            } else {
                l.q8s = (const unsigned char*)pq;
            }
            const ConvPlan p = conv_plan(l);  // (a function of the shape, the flags and the alignment: the same for both forms)
            const int pv[6] = {p.kernel, p.ksplit, p.nseg, p.epi, p.seg_rows, p.kernel_last};
            FMCHECK(!form || memcmp(pv, plan, sizeof(pv)) == 0, "prompt GEMM: the code form planned another launch");
            memcpy(plan, pv, sizeof(pv));
            for (int i = 0; i < reps; ++i) launch_conv_gemm<bf16_t>(g.s, l);
            HIPCHK(hipGetLastError());
            out.get(g.s);
        }
    });
}

int fm_op_sample(int device, int precision, int slow, const float* logits, int R, int ldl, int Nl,
                 const int32_t* row_slot, int slots, const float* temperature, const float* top_p, const int32_t* top_k,
                 const int32_t* mask_im_end, const uint64_t* seed, const int32_t* step, const int32_t* force, int sb,
                 int se, int im_end, int cb, int draw, int col_idx, const int32_t* ras, int ras_enable,
                 const int32_t* force_cols, int32_t* cols, int ldc, float* tap, int tap_ld, int* kernel) {
    return fm_guard([&] {
        FMCHECK(logits && row_slot && temperature && top_p && top_k && mask_im_end && seed && step && force && ras &&
                    force_cols && cols && tap && kernel,
                "null argument");
        FMCHECK(R >= 1 && R <= 64 && slots >= 1 && slots <= 64 && Nl >= 1 && ldl >= Nl && tap_ld >= Nl,
                "need 1 <= R, slots <= 64 and rows of ldl, tap_ld >= Nl >= 1");
        // launch_sample_radix's own LDS condition, refused here before anything is allocated
        size_t P = 1;  // the wide path's sort length
        while (P < (size_t)Nl) P <<= 1;
        FMCHECK(std::max(sizeof(float) * (size_t)Nl, sizeof(uint64_t) * P) + 8 * 1024 <= 160 * 1024,
                "sampler: vocabulary too wide for the LDS row");
        FMCHECK(cb >= 1 && draw >= 0 && draw < 64 && (slow ? ldc >= 2 : (col_idx >= 0 && col_idx < ldc)),
                "cols rows hold [0], [1] (slow) or [col_idx] (fast)");
        for (int r = 0; r < R; ++r) FMCHECK(row_slot[r] >= 0 && row_slot[r] < slots, "row_slot outside the slot table");
        for (int i = 0; i < slots; ++i) FMCHECK(step[i] >= 0, "negative step");
        StreamGuard g(device);
        DevBufs b(g.s);
        sample_init();
        std::vector<SlotParams> sp((size_t)slots);
        for (int i = 0; i < slots; ++i) {
            sp[i] = SlotParams{};
            sp[i].temperature = temperature[i];
            sp[i].top_p = top_p[i];
            sp[i].top_k = top_k[i];
            sp[i].mask_im_end = mask_im_end[i];
            sp[i].seed = seed[i];
            sp[i].step = step[i];
            sp[i].force = force[i];
        }
        auto dev = [&](const void* h, size_t bytes) {
            void* d = b.alloc(bytes);
            b.put(d, h, bytes);
            return d;
        };
        SampleArgs a{};
        a.logits = (const float*)dev(logits, (size_t)R * ldl * 4);
        a.ldl = ldl;
        a.Nl = Nl;
        a.row_slot = (const int*)dev(row_slot, (size_t)R * 4);
        a.sp = (const SlotParams*)dev(sp.data(), sizeof(SlotParams) * slots);
        a.ras = (const int32_t*)dev(ras, (size_t)slots * 10 * 4);
        a.ras_stride = 10;
        a.ras_enable = ras_enable;
        a.slow = slow != 0;
        a.sb = sb;
        a.se = se;
        a.im_end = im_end;
        a.cb = cb;
        a.draw = draw;
        a.col_idx = col_idx;
        a.dbg = nullptr;
        a.cols = (int32_t*)dev(cols, (size_t)R * ldc * 4);
        a.ldc = ldc;
        a.force_cols = (const int32_t*)dev(force_cols, (size_t)slots * ldc * 4);
        a.tap = (float*)dev(tap, (size_t)slots * tap_ld * 4);
        a.tap_ld = tap_ld;
        *kernel = (Nl <= sample_fast_max_row() && fm_tuning().sampler_fast) ? 1 : 0;  // the launcher's own choice
        if (precision == FM_PREC_BF16) launch_sample_radix<bf16_t>(g.s, a, R);
        else launch_sample_radix<float>(g.s, a, R);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(cols, a.cols, (size_t)R * ldc * 4, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipMemcpyAsync(tap, a.tap, (size_t)slots * tap_ld * 4, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
    });
}

int fm_rope_table(int seq_len, int head_dim, float base, float* out) {
    return fm_guard([&] {
        FMCHECK(out && seq_len >= 1 && head_dim >= 2 && head_dim % 2 == 0, "bad arguments");
        auto t = rope_table_host(seq_len, head_dim, base);
        memcpy(out, t.data(), t.size() * 4);
    });
}

}  // extern "C"
