// fm_prefix.hip -- the voice prefix cache's copy kernel (fm_llm_prefix_save / fm_llm_prefix_load).
//
// A prefix of npos positions is, per slot, n_layer * 2 * nkv runs: rows [0, npos) of one
// (layer, K | V, kv head) are npos * hd contiguous elements of the slot cache
// [slot][layer][kv head][S][hd], and run r = (layer * 2 + K|V) * nkv + head of the compact store
// [layer][K|V][kv head][npos][hd] is the same npos * hd elements.  One launch moves every run of
// every slot of the call: blockIdx.y = run, blockIdx.z = index into the slot list, blockIdx.x and a
// grid-stride loop along the run.  to_store = 1 reads the slot and writes the store (save, one
// slot), 0 reads the store and writes each listed slot (load).  A pure stream: 16 bytes per lane,
// U accesses in flight per lane before the first store, consecutive lanes on consecutive 16 bytes.
#include "fm_common.h"
#include "fm_kernels.h"

namespace {
typedef __attribute__((ext_vector_type(4))) uint32_t pfx_u4_t;

// V: the access unit (16-byte vector, or a 2-byte scalar where a run or a base is not 16-byte
// aligned); run_units = run bytes / sizeof(V)
template <typename V, int U>
__global__ __launch_bounds__(256) void kv_prefix_copy_kernel(KvPrefixArgs a) {
    const int run = blockIdx.y;
    const int head = run % a.nkv, kv = (run / a.nkv) & 1, layer = run / (2 * a.nkv);
    const int slot = a.slots[blockIdx.z];
    char* cache = (kv ? a.vc : a.kc) + (size_t)slot * a.slot_stride_b + (size_t)layer * a.layer_stride_b +
                  (size_t)head * a.head_stride_b;
    char* store = a.store + (size_t)run * a.run_bytes;
    const V* __restrict__ src = reinterpret_cast<const V*>(a.to_store ? cache : store);
    V* __restrict__ dst = reinterpret_cast<V*>(a.to_store ? store : cache);
    const int64_t n = a.run_units, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + (U - 1) * stride < n; i += U * stride) {
        V v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[i + u * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) dst[i + u * stride] = v[u];
    }
    for (; i < n; i += stride) dst[i] = src[i];
}
}  // namespace

void launch_kv_prefix_copy(hipStream_t s, const KvPrefixArgs& a0, int n_layer, int nslots) {
    KvPrefixArgs a = a0;
    const auto al16 = [](size_t v) { return v % 16 == 0; };
    const bool vec = fm_tuning().prefix_vec && al16(a.run_bytes) && al16(a.slot_stride_b) && al16(a.layer_stride_b) &&
                     al16(a.head_stride_b) && al16((size_t)a.kc) && al16((size_t)a.vc) && al16((size_t)a.store);
    const int runs = n_layer * 2 * a.nkv;
    if (vec) {
        constexpr int U = 4;
        a.run_units = (int64_t)(a.run_bytes / 16);
        // blocks along a run: each moves U * 4 KiB per step; enough of them that a one-slot copy of a
        // short prefix still covers the chip, at most 8 (a 700-position S2-Pro run is 175 KiB)
        const int gx = (int)std::min<int64_t>(8, std::max<int64_t>(1, FM_CEIL(a.run_units, (int64_t)256 * U)));
        kv_prefix_copy_kernel<pfx_u4_t, U><<<dim3(gx, runs, nslots), 256, 0, s>>>(a);
    } else {
        constexpr int U = 4;
        a.run_units = (int64_t)(a.run_bytes / 2);
        const int gx = (int)std::min<int64_t>(8, std::max<int64_t>(1, FM_CEIL(a.run_units, (int64_t)256 * U)));
        kv_prefix_copy_kernel<uint16_t, U><<<dim3(gx, runs, nslots), 256, 0, s>>>(a);
    }
}
