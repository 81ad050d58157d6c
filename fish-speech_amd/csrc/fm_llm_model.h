// fm_llm_model.h -- the Dual-AR handle (struct fm_llm), its constants, and the functions the
// fm_llm*.cpp files share.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fm_kernels.h"
#include "fm_runtime.h"

static constexpr int PREFILL_CHUNK = 1024;  // prompt rows per slow-stack pass (GEMM M)
static constexpr int ATTN_PIECE = 256;      // prompt rows per attention launch (bounds the split partials)
static constexpr int ATTN_SPLIT = 64;
static constexpr int GEMV_MAX_ROWS = 8;  // frames with <= 8 streams take the fused GEMV path
static constexpr int KSB_MAX = 8;

// attn_decode2's rows per block in a frame: the LDS budget (attn2_cap), capped by the attn_cap knob of the
// small-batch frame or attn_cap_batched of the batched one (the frames and fm_op_decode_attn_ex's frame mode)
inline int attn2_frame_cap(int hd, int g, size_t esz, bool batched) {
    const int cap = attn2_cap(hd, g, esz), knob = batched ? fm_tuning().attn_cap_batched : fm_tuning().attn_cap;
    return knob ? std::min(cap, knob) : cap;
}
// Which slow decode attention a frame of R rows launches, and with what geometry (the frame's
// attn_slow_on and the per-op hook fm_op_decode_attn_ex both ask here).  kernel as fm_op_decode_attn
// numbers them: 3 attn_fd, 2 attn_dec3, 0 attn_decode2.  attn_fd: nwb waves per block and splits of
// at least cap positions, hpb q heads of a kv head per block, from the fd_* knobs; the other two keep
// the caller's cap (cap0).
struct AttnSlowPlan {
    int kernel, nwb, cap;
    int hpb = 4;
};
// attn_fd's q heads per block on R rows: fm_tune fd_hpb up to 8 rows, every head of the kv head past them
inline int fd_hpb_rows(int R) { return R <= GEMV_MAX_ROWS ? fm_tuning().fd_hpb : 4; }
inline AttnSlowPlan attn_slow_plan(int R, int hd, int g, int cap0) {
    const FmTuning& tu = fm_tuning();
    if (tu.attn_fd && attn_fd_ok(hd, g)) {
        AttnSlowPlan p{3, 4, std::max(16, R > GEMV_MAX_ROWS ? tu.fd_min_batched : tu.fd_min), fd_hpb_rows(R)};
        if (R <= GEMV_MAX_ROWS && tu.fd_nw > 4) {
            p.nwb = tu.fd_nw;
            p.cap = std::max(16, tu.fd_min16);
        } else if (R > GEMV_MAX_ROWS && tu.fd_nw_batched > 4) {
            p.nwb = tu.fd_nw_batched;
        }
        return p;
    }
    if (tu.attn3 && R > GEMV_MAX_ROWS && hd % 32 == 0 && hd <= 128 && g <= 6) return {2, 4, cap0};
    return {0, 4, cap0};
}
static constexpr int BS_KPARTS = 8;  // most K parts of a bstream slab (fm_bstream.hip)

// split-K factor across blocks for a GEMV with N output rows: >= ~512 blocks when possible,
// K/(32*ksb) integral, LDS staging within budget.
inline int pick_ksb(int N, int K, int R, size_t esz) {
    const int nb = (N + 15) / 16;
    const FmTuning& tu = fm_tuning();
    int ksb = 1;
    while (ksb < KSB_MAX && nb * ksb < tu.ksb_blocks && K % (32 * ksb * 2) == 0) ksb *= 2;
    if (tu.ksb_balance) {
        // among the admissible split factors pick the one whose grid wastes the least of its
        // last round of 256 CUs (ties: the smaller split)
        double best = 1e9;
        int bk = ksb;
        for (int k = 1; k <= KSB_MAX && K % (32 * k) == 0; k *= 2) {
            const int b = nb * k;
            if (b < 256) continue;
            const double rounds = (double)((b + 255) / 256), waste = rounds * 256.0 / b;
            if (waste < best - 1e-3) {
                best = waste;
                bk = k;
            }
        }
        ksb = bk;
    }
    while (gemv_lds_bytes(R, K / ksb, esz) > 96 * 1024 && ksb < KSB_MAX && K % (32 * ksb * 2) == 0) ksb *= 2;
    while (K / ksb > 4096 && K % (32 * ksb * 2) == 0) ksb *= 2;  // one 8-element chunk per thread
    return ksb;
}

// One nn.Linear [N][K] on the device, in every layout a kernel reads.  finalize() fills it once; the launches only
// read it, and a pointer that is null means the linear has no such layout.  Every pointer is a device address.
// Ownership: each buffer below is in fm_llm::allocs (freed once, at close), never in the DTensor map -- except an
// int8 checkpoint's row scales (scale / rm_scale), which stay the "<name>.scales" DTensor's.
struct Linear {
    int N = 0, K = 0;
    // packed bf16 / fp32 MFMA fragments (fm_kernels.h); null: a compact handle's quantised linear (fm_llm_set_quant_compact
    // keeps only the codes), which every launcher serves from the code layouts below
    const void* frag = nullptr;
    // weight-only int8 / int4, decode-GEMV units: the packed codes (int4: 4-bit) with the int8 row scales [rows padded
    // to 16] or the int4 packed (scale, zero) per (tile, 128-k unit, row)
    const unsigned char* q8 = nullptr;
    const void* scale = nullptr;
    const uint32_t* sz = nullptr;
    // bf16: the step-granular copy of the same codes the batched linears stream (max_slots > 8) and the tile kernel's
    // code form reads (compact), with scale / sz above (launch_pack_q8s / launch_pack_q4s)
    const unsigned char* q8s = nullptr;
    const uint32_t* q4s = nullptr;
    // the row-block GEMV's row-major copy (fm_rowgemv.hip): bf16 rows, int8 codes with their row scales (w1 || w3: in
    // its row-block interleaved order), or int4 code words with their (scale, zero) rows
    const void* rm = nullptr;
    const void* rm_scale = nullptr;
    const uint32_t* rm_sz = nullptr;
    explicit operator bool() const { return frag || q8; }
};

// Weight bytes one launch streams (bench.py's roofline and fm_llm_profile_read report them), one formula per layout;
// form: 0 the T weight (E bytes per element), 1 int8 codes, 2 int4 codes.  N: the rows the launch covers.
// decode-GEMV units: int8 books no scales, int4 its (scale, zero) words of rows padded to 16
inline int64_t gemv_wbytes(int form, int64_t N, int64_t K, int64_t E) {
    return form == 2 ? N * K / 2 + (N + 15) / 16 * 16 * (K / 128) * 4 : (form == 1 ? N * K : N * K * E);
}
// the tile kernel's and bstream's step-granular codes: + a 2-byte scale per row, or a (scale, zero) word per 128-k unit
inline int64_t step_wbytes(int form, int64_t N, int64_t K, int64_t E) {
    return form == 2 ? N * K / 2 + N * (K / 128) * 4 : (form == 1 ? N * K + N * 2 : N * K * E);
}
// the row-major copy (bf16): + a 2-byte scale per row, or a (scale, zero) word per group of gs
inline int64_t row_wbytes(int form, int64_t N, int64_t K, int gs) {
    return form == 2 ? N * K / 2 + N * (K / gs) * 4 : (form == 1 ? N * K + N * 2 : N * K * 2);
}

struct LayerW {
    Linear wqkv, wo, w13, w2;  // w13: row-interleaved W1||W3
    void *bqkv = nullptr, *bo = nullptr, *qn = nullptr, *kn = nullptr, *an = nullptr, *fn = nullptr;
};

struct StackDims {
    int n_layer, dim, nh, nkv, hd, inter, qkv_bias, o_bias, qk_norm;
    int nq() const { return nh * hd; }
    int nqkv() const { return (nh + 2 * nkv) * hd; }
};

struct fm_llm {
    fm_model_config c{};
    int device = 0, prec = FM_PREC_BF16, max_slots = 1;
    size_t esz = 2;
    hipStream_t stream = nullptr;
    std::map<std::string, DTensor> w;
    bool finalized = false;
    StackDims sd{}, fdm{};
    int S = 0, C = 0, C1 = 0, cb = 0, nsem = 0, Nhead = 0, maxsplit = 0, Rmax = 0;
    std::vector<LayerW> slow, fast;
    void *emb = nullptr, *cbemb = nullptr, *norm = nullptr, *fproj_b = nullptr, *femb = nullptr, *fnorm = nullptr;
    // the constrained slow head; fast_project_in (unset when dim == fast_dim); the codebook head
    Linear head_c, fproj_w, fout;
    // caches
    void *kc = nullptr, *vc = nullptr, *fkc = nullptr, *fvc = nullptr;
    size_t slot_stride = 0, layer_stride = 0, fslot_stride = 0, flayer_stride = 0;
    float *rope = nullptr, *frope = nullptr;
    // activations
    void *x = nullptr, *h = nullptr, *xn = nullptr, *qkv = nullptr, *q = nullptr, *att = nullptr,
         *act = nullptr;
    void *xl = nullptr, *xnl = nullptr, *fx = nullptr, *fh = nullptr, *fxn = nullptr;
    // batch-1 GEMV chain (fm_tune gemv_chain): layer outputs alternate between x / x2 (fx / fx2), so no
    // launch re-reads a residual row it has already read and a later stage rewrites
    void *x2 = nullptr, *fx2 = nullptr;
    unsigned* chain_cnt = nullptr;  // [GEMV_CHAIN_WORDS] arrival counters (zeroed; each launch re-zeroes them)
    int* chain_err = nullptr;       // a chain wait timed out
    int* h_chain_err = nullptr;     // pinned copy, read after the host's stream sync
    void* plast = nullptr;  // batched prefill: the last prompt row of each request [max_slots][dim]
    float *part = nullptr, *logits = nullptr, *flogits = nullptr;
    void* act2 = nullptr;  // batched path: [R][2 * inter] output of the interleaved W1||W3
    int* attn_cnt = nullptr;
    float *ssX = nullptr, *ssH = nullptr;  // per-16-column tile sums of squares of the residual rows
    int* tickets = nullptr;               // EPI_SLABFIN / linear split-K arrival counters (zero between launches)
    float* skpart = nullptr;              // linear_kernel split-K partial tiles
    long long skpart_cap = 0;             //   floats
    float *slabA = nullptr, *slabB = nullptr;  // split-K partials of wo / w2 (small-batch path)
    float *bsA = nullptr, *bsB = nullptr;      // bstream K-part slabs of wo / w2 (batched path)
    float* bsQ = nullptr;                      // K-part slabs of the batched QKV (fm_tune bs_qkv_slab)
    // rows / slots
    int *frame_slot = nullptr, *frame_pos = nullptr, *prow_slot = nullptr, *prow_pos = nullptr;
    int32_t *tok_in = nullptr, *cols = nullptr, *ptok = nullptr, *ras = nullptr;
    SlotParams* sp = nullptr;
    // teacher forcing on the production graph (fm_llm_force / fm_llm_read_logits)
    int32_t* force_cols = nullptr;              // [max_slots][C1]
    float *tap_slow = nullptr, *tap_fast = nullptr;  // [max_slots][Nhead], [max_slots][C-1][cb]
    std::vector<int> host_force;
    int32_t* h_cols = nullptr;  // pinned [2][max_slots][C1]
    int32_t* h_hist = nullptr;  // pinned, grown on demand: [frames][n][C1] of fm_llm_decode_frames
    size_t h_hist_n = 0;
    std::vector<int> host_pos, host_step;
    std::vector<int> uploaded_slots;
    // graphs
    bool use_graph = true;
    std::map<int, hipGraphExec_t> graphs;
    Profiler prof;
    std::vector<void*> allocs;
    // weight-only int8 / int4 (fm_llm_set_quant, fm_llm_set_quant_int4): the linears' code layouts are in their Linear
    int quant = FM_QUANT_NONE;
    int q4_gs = 0;  // int4: group size along K
    int qmode() const { return quant == FM_QUANT_INT8 ? 1 : (quant == FM_QUANT_INT4 ? 2 : 0); }  // the kernels' QM
    int* fin_cnt = nullptr;   // split finalize_norm: [max rows][2] counters (zero between launches)
    float* fin_ss = nullptr;  //                      [max rows][16] chunk sums of squares
    // compact weight-only handles (fm_llm_set_quant_compact): finalize keeps the codes of every quantised
    // linear and frees (int8 checkpoints: never makes) its bf16 copy: Linear::frag is null
    bool compact = false;
    // whether the <= 8-row launches stream the linears' codes: an int4 handle under fm_tune int4_stream 0 runs on its
    // dequantised bf16 weights instead, unless it is compact and has none
    bool streams_codes() const { return quant != FM_QUANT_INT4 || fm_tuning().int4_stream || compact; }
    // fm_llm_memory_info: steady-state device bytes, booked where they are allocated
    // (finalize; ensure_qkv0's table): [0] fragment copies of quantised linears, [1] decode-GEMV code units
    // and their scale tables, [2] step-granular codes, [3] row-major copies and their tables, [4] every
    // other weight, [5] KV caches, [6] activations and scratch
    int64_t mem[7] = {0, 0, 0, 0, 0, 0, 0};
    int mem_cat = 6;  // the class dalloc books under
    bool row_ok = false;                    // every layer of both stacks has wo / w2 row-major (Linear::rm)
    bool row_qkv_ok = false;                //                         ... and wqkv
    bool row_w13_ok = false;                //                         ... and w1 || w3
    uint32_t* fxt = nullptr;                // fused fast attention + wo: tagged attention words [nh * hd]
    uint32_t* sxt = nullptr;                // fused slow attention + wo: tagged attention words [nh * hd] (its own buffer)
    int32_t* fiota = nullptr;              // [16]: fiota[c] = c - 1 (the fast KV prefetch's last cached row)
    // fm_tune rowgemv bit 5: the first fast layer's raw q|k|v row of every code [cb][fast nqkv] (bf16, unquantised
    // models; ensure_qkv0), valid while qkv0_epoch is the tuning epoch it was built under
    void* qkv0 = nullptr;
    int32_t* qkv0_iota = nullptr;           // [cb]: 0, 1, ...: the build's gather index
    unsigned qkv0_epoch = 0;
    bool qkv0_built = false;
    // voice prefix cache (fm_llm_prefix_*): id -> a compact snapshot [layer][K|V][kv head][npos][hd] of
    // the slow-stack rows [0, npos) some slot held, one device buffer each (freed at drop / close)
    struct Prefix {
        void* buf = nullptr;
        int npos = 0;
        size_t bytes = 0;
    };
    std::map<int, Prefix> prefixes;
    int next_prefix_id = 1;
    int* pfx_slots = nullptr;  // device [max_slots]: the slot list of one prefix copy launch

    ~fm_llm() {
        if (device >= 0) (void)hipSetDevice(device);
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
        for (auto& kv : w) {  // the tensors as uploaded (finalize hands the linears' buffers over to allocs)
            if (kv.second.p) (void)hipFree(kv.second.p);
            if (kv.second.q) (void)hipFree(kv.second.q);
        }
        for (void* p : allocs) (void)hipFree(p);
        for (auto& kv : prefixes) (void)hipFree(kv.second.buf);
        if (h_cols) (void)hipHostFree(h_cols);
        if (h_hist) (void)hipHostFree(h_hist);
        if (h_chain_err) (void)hipHostFree(h_chain_err);
        if (stream) (void)hipStreamDestroy(stream);
    }
    void* dalloc(size_t bytes, bool zero = true) {
        void* p = nullptr;
        if (bytes == 0) bytes = 16;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess)
            throw FmError{FM_ERR_OOM, "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e)};
        if (zero) HIPCHK(hipMemsetAsync(p, 0, bytes, stream));
        allocs.push_back(p);
        mem[mem_cat] += (int64_t)bytes;
        return p;
    }
};

// fm_llm_weights.cpp
void add_t(fm_llm* m, const std::string& n, int64_t rows, int64_t cols);
void build_inventory(fm_llm* m);
DTensor& tensor_for(fm_llm* m, const char* name, int64_t numel);
bool is_quant_linear(const std::string& n);
std::string base_of(const std::string& n);
void finalize(fm_llm* m);
// fm_llm_frame.cpp: the only translation unit that instantiates Run<T>
void ensure_qkv0(fm_llm* m);
void launch_frame(fm_llm* m, int n);        // one decode frame for the uploaded rows (graph replay when enabled), async
void decode_frame_eager(fm_llm* m, int n);  // the same frame launched eagerly (fm_llm_kernel_bench records it)
// prompt(s) through the slow stack, then the first frame's head + fast model + samplers (the caller finishes it)
void prefill_frame(fm_llm* m, int slot, const int32_t* tokens, int T, int pos0);
void prefill_batch_frame(fm_llm* m, int n, const int32_t* slots, const int32_t* const* toks, const int32_t* T,
                         const int32_t* pos0);
// fm_llm_teacher_step's launches and copies: lg receives the Nhead slow logits once the stream is synchronised
void teacher_frame(fm_llm* m, int slot, const int32_t* x, int S, int pos0, const int32_t* next_col, float* lg,
                   float* hidden, float* fast_logits);
