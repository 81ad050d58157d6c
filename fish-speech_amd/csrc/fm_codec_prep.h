// fm_codec_prep.h -- how the codec prepares a conv / linear layer for conv_gemm: the packed weight
// record, its split-K factor, the weight re-layouts and the ConvArgs of a call site.  The model
// (fm_codec.cpp) and the per-op hooks (fm_codec_ops.cpp) call the same functions.
#pragma once
#include <functional>
#include <vector>

#include "fm_codec.h"
#include "fm_runtime.h"

struct PackedW {
    void* w = nullptr;
    size_t wphase = 0;
    int Co = 0, Ci = 0, ntaps = 1, nphase = 1, stride = 1;
    int shift[8] = {0};
    void* bias = nullptr;
    int ks = 1;  // split-K factor (small-M layers; a property of the layer, so every chunking of a
                 // streamed decode sums in the same order as the one-shot decode)
};

// split-K factor of a layer that runs at a few hundred rows: K steps of 32 per slice >= 8, <= 8 slices
inline void small_m(PackedW& W) {
    const int S = (W.ntaps * W.Ci + 31) / 32;
    int ks = 1;
    while (ks < 8 && S / (2 * ks) >= 8) ks *= 2;
    W.ks = W.Co % 8 == 0 ? ks : 1;
}

// A GEMM weight from the fp32 device tensor `w` (kind per conv_weight_kernel: 0 Conv1d [Co][Ci][k],
// 1 ConvTranspose1d [Ci][Co][2s], 2 ConvTranspose1d [Ci][Co][s], 3 Linear [Co][Ci]): the taps, their
// shifts and the phases packed for the MFMA GEMMs into memory from `alloc` (bias left null).
// Synchronises the stream before returning.
inline PackedW pack_conv_weight(hipStream_t s, int prec, const float* w, int kind, int Ci, int Co, int k, int st,
                                int dil, const std::function<void*(size_t)>& alloc) {
    PackedW p;
    p.Co = Co;
    p.Ci = Ci;
    p.ntaps = kind == 0 ? k : (kind == 1 ? 2 : 1);
    p.nphase = (kind == 1 || kind == 2) ? st : 1;
    p.stride = (kind == 1 || kind == 2) ? st : 1;
    FMCHECK(p.ntaps >= 1 && p.ntaps <= 8, "too many taps");
    FMCHECK(Ci >= 8 && Ci % 8 == 0, "codec channel counts must be multiples of 8");
    for (int j = 0; j < p.ntaps; ++j) p.shift[j] = kind == 0 ? (k - 1 - j) * dil : j;
    const int Kt = (p.ntaps * Ci + 31) / 32 * 32;  // padded
    const size_t rm = (size_t)p.nphase * Co * Kt, esz = prec == FM_PREC_BF16 ? 2 : 4;
    p.wphase = (size_t)(Co + 15) / 16 * 16 * Kt;
    void* tmp = nullptr;
    HIPCHK(hipMalloc(&tmp, rm * esz));
    try {
        p.w = alloc(p.wphase * p.nphase * esz);
        if (prec == FM_PREC_BF16) {
            launch_conv_weight<bf16_t>(s, w, kind, Ci, Co, k, st, (bf16_t*)tmp);
            for (int ph = 0; ph < p.nphase; ++ph)
                launch_pack<bf16_t>(s, (const bf16_t*)tmp + (size_t)ph * Co * Kt, Co, Kt, (bf16_t*)p.w + ph * p.wphase);
        } else {
            launch_conv_weight<float>(s, w, kind, Ci, Co, k, st, (float*)tmp);
            for (int ph = 0; ph < p.nphase; ++ph)
                launch_pack<float>(s, (const float*)tmp + (size_t)ph * Co * Kt, Co, Kt, (float*)p.w + ph * p.wphase);
        }
        HIPCHK(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipFree(tmp);
        throw;
    }
    HIPCHK(hipFree(tmp));
    return p;
}

// causal conv k = 2s, stride s (CausalConvNet, modded_dac.py:59-90; left pad k - s, no right pad
// when L % s == 0): out[t] = sum_j W[j] x[ts + j - s] = tap0 . x'[t-1] + tap1 . x'[t] over the
// contiguous view x'[L/s][s*Ci] of a time-major x, with x'[t][jj*Ci + ci] = x[ts + jj][ci].
// w [Co][Ci][2s] (host) -> the kind-0 weight [Co][s*Ci][2] of that two-tap conv
inline std::vector<float> strided_as_two_taps(const std::vector<float>& w, int Ci, int Co, int s) {
    std::vector<float> o((size_t)Co * s * Ci * 2);
    for (int co = 0; co < Co; ++co)
        for (int ci = 0; ci < Ci; ++ci)
            for (int jj = 0; jj < s; ++jj)
                for (int tap = 0; tap < 2; ++tap)
                    o[(((size_t)co * s + jj) * Ci + ci) * 2 + tap] = w[((size_t)co * Ci + ci) * 2 * s + tap * s + jj];
    return o;
}

// The ConvArgs of one call site of layer W, as every codec GEMM fills them: bias when the layer has
// one, the Snake to out2 when out2 is given (CE_NORM: out2 is the norm's output instead).  The
// caller adds the split-K workspace and factor and the CE_ROPE / CE_NORM operands.
template <typename T>
ConvArgs<T> conv_site_args(const PackedW& W, const void* x, int ldx, int Lq, int Lx, void* out, int ldo, int flags,
                           const void* res, int ldr, const void* gamma, const void* alpha2, const float* ialpha2,
                           void* out2, int ldo2, int lo) {
    ConvArgs<T> a{};
    a.x = (const T*)x;
    a.ldx = ldx;
    a.Ci = W.Ci;
    a.Lq = Lq;
    a.Lx = Lx;
    a.w = (const T*)W.w;
    a.wphase = W.wphase;
    a.Co = W.Co;
    a.ntaps = W.ntaps;
    a.stride = W.stride;
    a.nphase = W.nphase;
    for (int j = 0; j < 8; ++j) a.shift[j] = W.shift[j];
    a.bias = (const T*)W.bias;
    a.gamma = (const T*)gamma;
    a.res = (const T*)res;
    a.ldr = ldr;
    a.alpha2 = (const T*)alpha2;
    a.ialpha2 = ialpha2;
    a.out = out;
    a.ldo = ldo;
    a.out2 = (T*)out2;
    a.ldo2 = ldo2;
    a.flags = flags | (W.bias ? CE_BIAS : 0) | ((out2 && !(flags & CE_NORM)) ? CE_SNAKE : 0);
    a.lo = lo;
    return a;
}
