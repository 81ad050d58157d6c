// fm_llm_weights.cpp -- the Dual-AR weights: tensor inventory, quantisation, packing, finalize.
#include "fm_llm_model.h"

// ------------------------------------------------------------------------------------------
// tensor inventory (names = reference state_dict keys after remap; llama.py module tree)
// ------------------------------------------------------------------------------------------
void add_t(fm_llm* m, const std::string& n, int64_t rows, int64_t cols) {
    DTensor t;
    t.rows = rows;
    t.cols = cols;
    t.numel = rows * cols;
    m->w[n] = t;
}
static void add_stack(fm_llm* m, const std::string& pre, const StackDims& s) {
    for (int i = 0; i < s.n_layer; ++i) {
        std::string p = pre + std::to_string(i) + ".";
        add_t(m, p + "attention.wqkv.weight", s.nqkv(), s.dim);
        if (s.qkv_bias) add_t(m, p + "attention.wqkv.bias", 1, s.nqkv());
        add_t(m, p + "attention.wo.weight", s.dim, s.nq());
        if (s.o_bias) add_t(m, p + "attention.wo.bias", 1, s.dim);
        if (s.qk_norm) {
            add_t(m, p + "attention.q_norm.weight", 1, s.hd);
            add_t(m, p + "attention.k_norm.weight", 1, s.hd);
        }
        add_t(m, p + "feed_forward.w1.weight", s.inter, s.dim);
        add_t(m, p + "feed_forward.w3.weight", s.inter, s.dim);
        add_t(m, p + "feed_forward.w2.weight", s.dim, s.inter);
        add_t(m, p + "ffn_norm.weight", 1, s.dim);
        add_t(m, p + "attention_norm.weight", 1, s.dim);
    }
}

void build_inventory(fm_llm* m) {
    const fm_model_config& c = m->c;
    m->sd = StackDims{c.n_layer, c.dim, c.n_head, c.n_local_heads, c.head_dim, c.intermediate_size,
                      c.qkv_bias, c.o_bias, c.qk_norm};
    m->fdm = StackDims{c.n_fast_layer, c.fast_dim, c.fast_n_head, c.fast_n_local_heads, c.fast_head_dim,
                       c.fast_intermediate_size, c.fast_qkv_bias, c.fast_o_bias, c.fast_qk_norm};
    add_t(m, "embeddings.weight", c.vocab_size, c.dim);
    add_t(m, "codebook_embeddings.weight", (int64_t)c.codebook_size * c.num_codebooks, c.dim);
    add_stack(m, "layers.", m->sd);
    add_t(m, "norm.weight", 1, c.dim);
    if (!c.tie_word_embeddings) add_t(m, "output.weight", c.vocab_size, c.dim);
    if (c.fast_dim != c.dim) {
        add_t(m, "fast_project_in.weight", c.fast_dim, c.dim);
        add_t(m, "fast_project_in.bias", 1, c.fast_dim);
    }
    add_t(m, "fast_embeddings.weight", c.codebook_size, c.fast_dim);
    add_stack(m, "fast_layers.", m->fdm);
    add_t(m, "fast_norm.weight", 1, c.fast_dim);
    add_t(m, "fast_output.weight", c.codebook_size, c.fast_dim);
}

DTensor& tensor_for(fm_llm* m, const char* name, int64_t numel) {
    auto it = m->w.find(name);
    FMCHECK(it != m->w.end(), std::string("unknown tensor: ") + name);
    FMCHECK(it->second.numel == numel, std::string("wrong numel for ") + name + ": got " +
                                           std::to_string(numel) + ", want " + std::to_string(it->second.numel));
    DTensor& t = it->second;
    if (!t.p) {
        const int64_t rows = t.rows > 1 ? (t.rows + 15) / 16 * 16 : 1;
        const size_t bytes = (size_t)rows * t.cols * m->esz;
        HIPCHK(hipMalloc(&t.p, bytes));
        HIPCHK(hipMemsetAsync(t.p, 0, bytes, m->stream));
    }
    return t;
}

// ------------------------------------------------------------------------------------------
// finalize: validate weights, derive pointers, allocate caches / buffers
// ------------------------------------------------------------------------------------------
static void* W(fm_llm* m, const std::string& n) {
    auto it = m->w.find(n);
    FMCHECK(it != m->w.end() && it->second.set, "tensor not set: " + n);
    return it->second.p;
}
static void* Wopt(fm_llm* m, const std::string& n) {
    auto it = m->w.find(n);
    return (it != m->w.end() && it->second.set) ? it->second.p : nullptr;
}

static bool is_linear_weight(const std::string& n) {
    auto ends = [&](const char* suf) {
        const size_t L = strlen(suf);
        return n.size() >= L && n.compare(n.size() - L, L, suf) == 0;
    };
    return ends("attention.wqkv.weight") || ends("attention.wo.weight") || ends("feed_forward.w1.weight") ||
           ends("feed_forward.w2.weight") || ends("feed_forward.w3.weight") || n == "fast_output.weight" ||
           n == "fast_project_in.weight";
}

// every nn.Linear of the model (WeightOnlyInt8QuantHandler quantizes them all, quantize.py:190-206);
// the tied head is F.linear on the embedding table, not a module, and stays in T
bool is_quant_linear(const std::string& n) { return is_linear_weight(n) || n == "output.weight"; }
std::string base_of(const std::string& n) { return n.substr(0, n.size() - strlen(".weight")); }

// int8 row-major [rows][cols] (rows padded to 16) -> packed int8 decode-GEMV layout
static void* pack_q8_dev(fm_llm* m, const void* q, int rows, int cols) {
    FMCHECK(cols % 64 == 0, "int8 weights need in_features % 64 == 0");
    void* dst = nullptr;
    HIPCHK(hipMalloc(&dst, (size_t)(rows + 15) / 16 * 16 * cols));
    launch_pack_q8(m->stream, (const int8_t*)q, rows, cols, (int8_t*)dst);
    HIPCHK(hipGetLastError());
    m->allocs.push_back(dst);
    m->mem[1] += (int64_t)(rows + 15) / 16 * 16 * cols;
    return dst;
}

// the batched linears' step-granular copy of the same codes: only where bsacc_kernel can take it (int8,
// bf16, a handle with more than GEMV_MAX_ROWS slots); a max_slots <= 8 handle allocates nothing here -- unless it is
// compact: there the copy is what linear_kernel's code form reads, whatever max_slots is
static const unsigned char* pack_q8s_dev(fm_llm* m, const void* q, int rows, int cols) {
    if (m->quant != FM_QUANT_INT8 || m->prec != FM_PREC_BF16 || (m->max_slots <= GEMV_MAX_ROWS && !m->compact) || cols % 32)
        return nullptr;
    void* dst = nullptr;
    HIPCHK(hipMalloc(&dst, (size_t)(rows + 15) / 16 * 16 * cols));
    launch_pack_q8s(m->stream, (const int8_t*)q, rows, cols, (int8_t*)dst);
    HIPCHK(hipGetLastError());
    m->allocs.push_back(dst);
    m->mem[2] += (int64_t)(rows + 15) / 16 * 16 * cols;
    return (const unsigned char*)dst;
}

// int4: codes row-major [rows][cols] + sz [rows][cols / gs] -> the packed GEMV stream and its
// (scale, zero) table; none (the bf16 dequantised copy serves every kernel) unless the group size
// and K are whole 128-k units
static fm_llm::QInfo pack_q4_dev(fm_llm* m, const void* q, const void* sz, int rows, int cols) {
    if (m->q4_gs % 128 || cols % 128) return fm_llm::QInfo{};
    const size_t tiles = (size_t)(rows + 15) / 16;
    void* dq = nullptr;
    void* ds = nullptr;
    HIPCHK(hipMalloc(&dq, tiles * 16 * cols / 2));
    HIPCHK(hipMalloc(&ds, tiles * (cols / 128) * 16 * 4));
    launch_pack_q4(m->stream, (const uint8_t*)q, rows, cols, (uint8_t*)dq);
    launch_pack_sz4(m->stream, (const uint32_t*)sz, rows, cols, m->q4_gs, (uint32_t*)ds);
    HIPCHK(hipGetLastError());
    m->allocs.push_back(dq);
    m->allocs.push_back(ds);
    m->mem[1] += (int64_t)(tiles * 16 * cols / 2 + tiles * (cols / 128) * 16 * 4);
    // the batched linears' step-granular copy of the same codes (they stream it with ds): only where
    // bsacc_kernel can take it -- bf16, a handle with more than GEMV_MAX_ROWS slots; a max_slots <= 8
    // handle allocates nothing here (a compact one does: linear_kernel's code form reads it).  Its own allocation:
    // row_copies 0 frees none of it.
    void* d4 = nullptr;
    if (m->prec == FM_PREC_BF16 && (m->max_slots > GEMV_MAX_ROWS || m->compact)) {
        HIPCHK(hipMalloc(&d4, tiles * 16 * cols / 2));
        launch_pack_q4s(m->stream, (const uint8_t*)q, rows, cols, (uint32_t*)d4);
        HIPCHK(hipGetLastError());
        m->allocs.push_back(d4);
        m->mem[2] += (int64_t)(tiles * 16 * cols / 2);
    }
    return fm_llm::QInfo{(const unsigned char*)dq, nullptr, (const uint32_t*)ds, nullptr, (const uint32_t*)d4};
}

// int8 mode, before packing: every quantized linear ends with t.p = T(q) row-major (what the
// T-fragment kernels read), t.q = int8 row-major, t.s = row scales.  int8 checkpoints supply q and
// "<name>.scales"; float weights are quantized here with quantize.py's per-channel rule.
static void quantize_linears(fm_llm* m) {
    m->mem_cat = 1;  // (the int8 row scales allocated below belong to the decode-GEMV units)
    if (m->quant == FM_QUANT_INT4) {  // every linear: codes, group (scale, zero), dequantised bf16 in place
        for (auto& kv : m->w) {
            if (!is_quant_linear(kv.first)) continue;
            DTensor& t = kv.second;
            const size_t rp = (size_t)(t.rows + 15) / 16 * 16;
            HIPCHK(hipMalloc(&t.q, rp * t.cols));
            HIPCHK(hipMemsetAsync(t.q, 8, rp * t.cols, m->stream));
            void* sz = nullptr;
            HIPCHK(hipMalloc(&sz, rp * (t.cols / m->q4_gs) * 4));
            HIPCHK(hipMemsetAsync(sz, 0, rp * (t.cols / m->q4_gs) * 4, m->stream));
            t.s = sz;
            launch_quant4(m->stream, (bf16_t*)t.p, (int)t.rows, (int)t.cols, m->q4_gs, (uint8_t*)t.q, (uint32_t*)sz);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(m->stream));
        m->mem_cat = 6;
        return;
    }
    for (auto& kv : m->w) {
        if (!is_quant_linear(kv.first)) continue;
        DTensor& t = kv.second;
        const size_t rp = (size_t)(t.rows + 15) / 16 * 16;
        DTensor& sc = m->w.at(base_of(kv.first) + ".scales");
        if (t.q) {
            FMCHECK(sc.set, "int8 weight without scales: " + kv.first);
            FMCHECK(!t.p, "tensor set twice: " + kv.first);
            if (!m->compact) {  // (a compact handle serves the linear from its codes: no T expansion at all)
                HIPCHK(hipMalloc(&t.p, rp * t.cols * m->esz));
                if (m->prec == FM_PREC_BF16)
                    launch_i8_to<bf16_t>(m->stream, (const int8_t*)t.q, (int64_t)rp * t.cols, (bf16_t*)t.p);
                else
                    launch_i8_to<float>(m->stream, (const int8_t*)t.q, (int64_t)rp * t.cols, (float*)t.p);
            }
            t.s = sc.p;
        } else {
            FMCHECK(!sc.set, "scales given with a float weight: " + kv.first);
            HIPCHK(hipMalloc(&t.q, rp * t.cols));
            HIPCHK(hipMemsetAsync(t.q, 0, rp * t.cols, m->stream));
            t.s = m->dalloc(rp * m->esz);
            if (m->prec == FM_PREC_BF16)
                launch_quant_rows<bf16_t>(m->stream, (bf16_t*)t.p, (int)t.rows, (int)t.cols, (int8_t*)t.q, (bf16_t*)t.s);
            else
                launch_quant_rows<float>(m->stream, (float*)t.p, (int)t.rows, (int)t.cols, (int8_t*)t.q, (float*)t.s);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    m->mem_cat = 6;
}

// row-major [rows][cols] device tensor -> packed fragment layout (fm_kernels.h)
// (booked as the fragment copy of a quantised linear, qlin, or as any other weight)
static void* pack_dev(fm_llm* m, const void* src, int rows, int cols, bool qlin) {
    const size_t n = (size_t)(rows + 15) / 16 * 16 * cols;
    void* dst = nullptr;
    HIPCHK(hipMalloc(&dst, n * m->esz));
    m->mem[qlin ? 0 : 4] += (int64_t)(n * m->esz);
    if (m->prec == FM_PREC_BF16)
        launch_pack<bf16_t>(m->stream, (const bf16_t*)src, rows, cols, (bf16_t*)dst);
    else
        launch_pack<float>(m->stream, (const float*)src, rows, cols, (float*)dst);
    HIPCHK(hipGetLastError());
    return dst;
}

// bf16 wo / w2 / wqkv whose shapes the row-block GEMV takes keep their row-major copy
// (fm_rowgemv.hip; ~3.7 GB at S2-Pro beside the packed tiles the batched paths read)
// fm_tune row_copies 0: a row-major copy only where the rowgemv bits in force at finalize use it
static bool row_bits(fm_llm* m, int bits) {
    const FmTuning& t = fm_tuning();
    return t.row_copies || ((m->quant == FM_QUANT_INT4 ? t.rowgemv_q4 : t.rowgemv) & bits) != 0;
}
static bool row_keep(fm_llm* m, const std::string& n, int rows, int cols) {
    auto ends = [&](const char* suf) {
        const size_t L = strlen(suf);
        return n.size() >= L && n.compare(n.size() - L, L, suf) == 0;
    };
    // bf16: the T row-major weight; weight-only int8: the int8 row-major codes (rowgemv QM 1)
    const int qm = m->quant == FM_QUANT_INT8 ? 1 : (m->quant == FM_QUANT_INT4 ? 2 : 0);
    if (m->prec != FM_PREC_BF16 || rowgemv_u(cols, qm) == 0) return false;
    if (qm == 2 && (m->q4_gs % 8 || cols % m->q4_gs)) return false;
    if (ends("attention.wo.weight") || ends("feed_forward.w2.weight")) return rows % 2 == 0 && row_bits(m, 1);
    if (n == "fast_output.weight") return rows % 8 == 0 && rowgemv_u(cols, qm) <= 8 && row_bits(m, 8);
    return ends("attention.wqkv.weight") && rows % 8 == 0 && rowgemv_u(cols, qm) <= 8 && row_bits(m, 2 | 16);
}

static bool is_ffn_w13(const std::string& n) {
    auto ends = [&](const char* suf) {
        const size_t L = strlen(suf);
        return n.size() >= L && n.compare(n.size() - L, L, suf) == 0;
    };
    return ends("feed_forward.w1.weight") || ends("feed_forward.w3.weight");
}

// W1 [inter][dim] and W3 -> one packed [2*inter][dim] matrix whose 16-row tiles hold 8 rows of W1
// then the same 8 rows of W3, so one GEMV tile (EPI_SWIGLU8) has both halves of 8 SwiGLU outputs and
// the decode grid is 2*inter/16 single-matrix blocks.  The row-major W1/W3 are freed; their map
// entries keep the shapes (the packed matrix hangs off the w1 entry).
static void* pack_w13(fm_llm* m, const std::string& p, int inter, int dim) {
    FMCHECK(inter % 8 == 0, "intermediate_size must be a multiple of 8");
    DTensor& t1 = m->w.at(p + "feed_forward.w1.weight");
    DTensor& t3 = m->w.at(p + "feed_forward.w3.weight");
    const size_t E = m->esz, rb = (size_t)dim * E;
    void* tmp = nullptr;
    void* pk = nullptr;
    if (m->compact) {  // no T tiles: the key of the codes packed below
        pk = const_cast<void*>(m->compact_key());
    } else {
        HIPCHK(hipMalloc(&tmp, 2 * (size_t)inter * rb));
        HIPCHK(hipMemcpy2DAsync(tmp, 16 * rb, t1.p, 8 * rb, 8 * rb, inter / 8, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)tmp + 8 * rb, 16 * rb, t3.p, 8 * rb, 8 * rb, inter / 8, hipMemcpyDeviceToDevice,
                                m->stream));
        pk = pack_dev(m, tmp, 2 * inter, dim, m->quant != FM_QUANT_NONE);
    }
    m->mem_cat = 3;  // the row-block GEMV's copies and their tables
    // the row-block GEMV's copy (fm_rowgemv.hip ROWGEMV_NORM_SWIGLU): row-major, rows 4b .. 4b+3 of W1
    // then the same rows of W3, per 8-row block (bf16 rows, or int8 codes + scales, or int4 packed
    // code words + (scale, zero) rows)
    const int qm = m->quant == FM_QUANT_INT8 ? 1 : (m->quant == FM_QUANT_INT4 ? 2 : 0);
    const bool rk = m->prec == FM_PREC_BF16 && inter % 4 == 0 && rowgemv_u(dim, qm) > 0 && rowgemv_u(dim, qm) <= 8 &&
                    (qm != 2 || (m->q4_gs % 8 == 0 && dim % m->q4_gs == 0)) && row_bits(m, 4);
    auto il4 = [&](const void* a1, const void* a3, size_t rb4) -> void* {  // rb4: bytes per row
        void* d = m->dalloc(2 * (size_t)inter * rb4, false);
        HIPCHK(hipMemcpy2DAsync(d, 8 * rb4, a1, 4 * rb4, 4 * rb4, inter / 4, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)d + 4 * rb4, 8 * rb4, a3, 4 * rb4, 4 * rb4, inter / 4, hipMemcpyDeviceToDevice,
                                m->stream));
        return d;
    };
    if (rk && qm == 0) m->rowmajor[pk] = il4(t1.p, t3.p, rb);
    if (rk && qm == 1) {
        m->rowmajor[pk] = il4(t1.q, t3.q, (size_t)dim);
        m->rowscale[pk] = il4(t1.s, t3.s, E);
    }
    if (rk && qm == 2) {
        void* codes = nullptr;  // one byte per code, interleaved, then packed to row words
        HIPCHK(hipMalloc(&codes, 2 * (size_t)inter * dim));
        HIPCHK(hipMemcpy2DAsync(codes, 8 * (size_t)dim, t1.q, 4 * (size_t)dim, 4 * (size_t)dim, inter / 4,
                                hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)codes + 4 * (size_t)dim, 8 * (size_t)dim, t3.q, 4 * (size_t)dim, 4 * (size_t)dim,
                                inter / 4, hipMemcpyDeviceToDevice, m->stream));
        void* words = m->dalloc((size_t)inter * dim, false);
        launch_pack_q4_rows(m->stream, (const uint8_t*)codes, 2 * inter, dim, (uint32_t*)words);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipFree(codes));
        m->rowmajor[pk] = words;
        m->rowsz[pk] = il4(t1.s, t3.s, (size_t)(dim / m->q4_gs) * 4);
    }
    if (m->quant == FM_QUANT_INT4) {  // the same interleave of the code rows and of the (scale, zero) rows
        const size_t gb = (size_t)(dim / m->q4_gs) * 4;
        void* qt = nullptr;
        void* st = nullptr;
        HIPCHK(hipMalloc(&qt, 2 * (size_t)inter * dim));
        HIPCHK(hipMalloc(&st, 2 * (size_t)inter * gb));
        HIPCHK(hipMemcpy2DAsync(qt, 16 * (size_t)dim, t1.q, 8 * (size_t)dim, 8 * (size_t)dim, inter / 8,
                                hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)qt + 8 * (size_t)dim, 16 * (size_t)dim, t3.q, 8 * (size_t)dim,
                                8 * (size_t)dim, inter / 8, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync(st, 16 * gb, t1.s, 8 * gb, 8 * gb, inter / 8, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)st + 8 * gb, 16 * gb, t3.s, 8 * gb, 8 * gb, inter / 8, hipMemcpyDeviceToDevice,
                                m->stream));
        fm_llm::QInfo qi = pack_q4_dev(m, qt, st, 2 * inter, dim);
        qi.compact = m->compact;
        FMCHECK(qi.q8 || !m->compact, "compact: no int4 code layout for " + p + "feed_forward.w1.weight");
        if (qi.q8) m->qmap[pk] = qi;
        HIPCHK(hipStreamSynchronize(m->stream));
        for (void* p : {qt, st, t1.q, t3.q, t1.s, t3.s}) HIPCHK(hipFree(p));
        t1.q = t3.q = nullptr;
        t1.s = t3.s = nullptr;
    } else if (m->quant) {  // the same interleave of the int8 rows and of the row scales
        void* qt = nullptr;
        HIPCHK(hipMalloc(&qt, 2 * (size_t)inter * dim));
        HIPCHK(hipMemcpy2DAsync(qt, 16 * (size_t)dim, t1.q, 8 * (size_t)dim, 8 * (size_t)dim, inter / 8,
                                hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)qt + 8 * (size_t)dim, 16 * (size_t)dim, t3.q, 8 * (size_t)dim,
                                8 * (size_t)dim, inter / 8, hipMemcpyDeviceToDevice, m->stream));
        m->mem_cat = 1;
        void* s13 = m->dalloc(2 * (size_t)inter * E);
        m->mem_cat = 3;
        HIPCHK(hipMemcpy2DAsync(s13, 16 * E, t1.s, 8 * E, 8 * E, inter / 8, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpy2DAsync((char*)s13 + 8 * E, 16 * E, t3.s, 8 * E, 8 * E, inter / 8, hipMemcpyDeviceToDevice,
                                m->stream));
        m->qmap[pk] = fm_llm::QInfo{(const unsigned char*)pack_q8_dev(m, qt, 2 * inter, dim), s13, nullptr,
                                    pack_q8s_dev(m, qt, 2 * inter, dim), nullptr, m->compact};
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipFree(qt));
        HIPCHK(hipFree(t1.q));
        HIPCHK(hipFree(t3.q));
        t1.q = t3.q = nullptr;
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    m->mem_cat = 6;
    if (tmp) HIPCHK(hipFree(tmp));
    if (t1.p) HIPCHK(hipFree(t1.p));  // (null: a compact handle's int8 checkpoint tensor was never expanded)
    if (t3.p) HIPCHK(hipFree(t3.p));
    t1.p = pk;
    t3.p = nullptr;
    return pk;
}

void finalize(fm_llm* m) {
    if (m->finalized) return;
    const fm_model_config& c = m->c;
    bsacc_init();
    sample_init();
    for (auto& kv : m->w) FMCHECK(kv.second.set || kv.second.optional, "tensor not set: " + kv.first);
    if (m->compact) {
        // before anything is freed or packed: every quantised linear must have a code layout all its kernels read
        // (int8: whole 64-k units; int4: pack_q4_dev's condition -- group size and K whole 128-k units, K whole groups)
        FMCHECK(m->quant && m->prec == FM_PREC_BF16, "compact: a weight-only bf16 handle only");
        for (auto& kv : m->w) {
            if (!is_quant_linear(kv.first)) continue;
            const int64_t K = kv.second.cols;
            if (m->quant == FM_QUANT_INT4)
                FMCHECK(m->q4_gs % 128 == 0 && K % 128 == 0 && K % m->q4_gs == 0,
                        "compact int4 needs a group size and in_features that are multiples of 128: " + kv.first +
                            " (group size " + std::to_string(m->q4_gs) + ", in_features " + std::to_string(K) + ")");
            else
                FMCHECK(K % 64 == 0, "compact int8 needs in_features % 64 == 0: " + kv.first);
        }
    }
    if (m->quant) quantize_linears(m);
    for (auto& kv : m->w) {
        if (!is_linear_weight(kv.first) || is_ffn_w13(kv.first)) continue;  // W1/W3: pack_w13 below
        DTensor& t = kv.second;
        // (a compact handle packs no T tiles: the linear's key stands where the packed pointer would)
        void* pk = m->compact ? const_cast<void*>(m->compact_key())
                              : pack_dev(m, t.p, (int)t.rows, (int)t.cols, m->quant != FM_QUANT_NONE);
        if (m->quant == FM_QUANT_INT4) {
            fm_llm::QInfo qi = pack_q4_dev(m, t.q, t.s, (int)t.rows, (int)t.cols);
            qi.compact = m->compact;
            FMCHECK(qi.q8 || !m->compact, "compact: no int4 code layout for " + kv.first);
            if (qi.q8) m->qmap[pk] = qi;
            const bool keep = row_keep(m, kv.first, (int)t.rows, (int)t.cols);
            if (keep) {  // the codes as packed row-major words + the row-major (scale, zero) table
                m->mem_cat = 3;
                void* rw = m->dalloc((size_t)t.rows * t.cols / 2, false);
                m->mem_cat = 6;
                launch_pack_q4_rows(m->stream, (const uint8_t*)t.q, (int)t.rows, (int)t.cols, (uint32_t*)rw);
                HIPCHK(hipGetLastError());
                m->rowmajor[pk] = rw;
                m->rowsz[pk] = t.s;
                m->allocs.push_back(const_cast<void*>(t.s));
                m->mem[3] += (int64_t)((t.rows + 15) / 16 * 16 * (t.cols / m->q4_gs) * 4);
            }
            HIPCHK(hipStreamSynchronize(m->stream));
            HIPCHK(hipFree(t.q));
            if (!keep) HIPCHK(hipFree(const_cast<void*>(t.s)));
            t.q = nullptr;
            t.s = nullptr;
        } else if (m->quant) {
            m->qmap[pk] = fm_llm::QInfo{(const unsigned char*)pack_q8_dev(m, t.q, (int)t.rows, (int)t.cols), t.s, nullptr,
                                        pack_q8s_dev(m, t.q, (int)t.rows, (int)t.cols), nullptr, m->compact};
            HIPCHK(hipStreamSynchronize(m->stream));
            if (row_keep(m, kv.first, (int)t.rows, (int)t.cols)) {
                m->rowmajor[pk] = t.q;  // the int8 codes, row-major, for the row-block GEMV
                m->allocs.push_back(t.q);
                m->mem[3] += (int64_t)((t.rows + 15) / 16 * 16 * t.cols);
            } else {
                HIPCHK(hipFree(t.q));
            }
            t.q = nullptr;
        }
        HIPCHK(hipStreamSynchronize(m->stream));
        if (!m->quant && row_keep(m, kv.first, (int)t.rows, (int)t.cols)) {
            m->rowmajor[pk] = t.p;  // kept for the batch-1 row-pair GEMV
            m->allocs.push_back(t.p);
            m->mem[3] += (int64_t)((t.rows + 15) / 16 * 16 * t.cols * m->esz);
        } else if (t.p) {  // (null: a compact handle's int8 checkpoint tensor was never expanded)
            HIPCHK(hipFree(t.p));
        }
        t.p = pk;
    }
    auto stack = [&](const std::string& pre, const StackDims& d, std::vector<LayerW>& out) {
        out.resize(d.n_layer);
        for (int i = 0; i < d.n_layer; ++i) {
            std::string p = pre + std::to_string(i) + ".";
            LayerW& L = out[i];
            L.wqkv = W(m, p + "attention.wqkv.weight");
            L.bqkv = Wopt(m, p + "attention.wqkv.bias");
            L.wo = W(m, p + "attention.wo.weight");
            L.bo = Wopt(m, p + "attention.wo.bias");
            L.qn = Wopt(m, p + "attention.q_norm.weight");
            L.kn = Wopt(m, p + "attention.k_norm.weight");
            L.w13 = pack_w13(m, p, d.inter, d.dim);
            L.w2 = W(m, p + "feed_forward.w2.weight");
            L.an = W(m, p + "attention_norm.weight");
            L.fn = W(m, p + "ffn_norm.weight");
            auto rm = [&](const void* pk) -> void* {
                auto it = m->rowmajor.find(pk);
                return it == m->rowmajor.end() ? nullptr : it->second;
            };
            L.wo_rm = rm(L.wo);
            L.w2_rm = rm(L.w2);
            L.wqkv_rm = rm(L.wqkv);
            L.w13_rm = rm(L.w13);
        }
    };
    stack("layers.", m->sd, m->slow);
    stack("fast_layers.", m->fdm, m->fast);
    {
        int32_t io[16];
        for (int c = 0; c < 16; ++c) io[c] = c - 1;
        m->fiota = (int32_t*)m->dalloc(sizeof(io), false);
        HIPCHK(hipMemcpy(m->fiota, io, sizeof(io), hipMemcpyHostToDevice));
    }
    if (m->prec == FM_PREC_BF16)
        // (two rows: fm_tune fast_pair publishes codebook positions 0 and 1 in one launch)
        m->fxt = (uint32_t*)m->dalloc(2 * (size_t)m->fdm.nh * m->fdm.hd * sizeof(uint32_t));  // tags 0: never current
    m->row_ok = m->row_qkv_ok = m->row_w13_ok = true;
    for (auto* st : {&m->slow, &m->fast})
        for (const LayerW& L : *st) {
            m->row_ok = m->row_ok && L.wo_rm && L.w2_rm;
            m->row_qkv_ok = m->row_qkv_ok && L.wqkv_rm;
            m->row_w13_ok = m->row_w13_ok && L.w13_rm;
        }
    if (m->quant) {  // WeightOnlyInt8Linear has no bias (quantize.py:206-229): the checkpoint's are unused
        for (auto* st : {&m->slow, &m->fast})
            for (LayerW& L : *st) L.bqkv = L.bo = nullptr;
    }
    m->emb = W(m, "embeddings.weight");
    m->cbemb = W(m, "codebook_embeddings.weight");
    m->norm = W(m, "norm.weight");
    m->fproj_w = Wopt(m, "fast_project_in.weight");
    m->fproj_b = m->quant ? nullptr : Wopt(m, "fast_project_in.bias");
    m->femb = W(m, "fast_embeddings.weight");
    m->fnorm = W(m, "fast_norm.weight");
    m->fout = W(m, "fast_output.weight");
    {
        auto it = m->rowmajor.find(m->fout);
        m->fout_rm = it == m->rowmajor.end() ? nullptr : it->second;
    }
    // constrained head (inference.py:308-320): only the semantic rows + <|im_end|> can be
    // finite after the bias, so the LM head streams exactly those rows.
    const void* outw = c.tie_word_embeddings ? m->emb : W(m, "output.weight");
    m->nsem = c.semantic_end_id - c.semantic_begin_id + 1;
    m->Nhead = m->nsem + 1;
    FMCHECK(m->Nhead <= 8192, "constrained head wider than 8192 rows is not supported");
    const size_t rowb = (size_t)c.dim * m->esz;
    const bool head_q = m->quant && !c.tie_word_embeddings;  // output.weight is a quantised linear; a tied head is not
    if (m->compact && head_q) {
        m->head_c = const_cast<void*>(m->compact_key());  // served from the compact rows of the codes packed below
    } else {
        m->mem_cat = 4;
        void* head_rm = m->dalloc((size_t)(m->Nhead + 15) / 16 * 16 * rowb);
        m->mem_cat = 6;
        HIPCHK(hipMemcpyAsync(head_rm, (const char*)outw + (size_t)c.semantic_begin_id * rowb,
                              (size_t)m->nsem * rowb, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpyAsync((char*)head_rm + (size_t)m->nsem * rowb,
                              (const char*)outw + (size_t)c.im_end_id * rowb, rowb, hipMemcpyDeviceToDevice,
                              m->stream));
        m->head_c = pack_dev(m, head_rm, m->Nhead, c.dim, head_q);
        m->allocs.push_back(m->head_c);
    }
    if (m->quant == FM_QUANT_INT4 && !c.tie_word_embeddings) {  // the compact rows of the codes and groups
        DTensor& o = m->w.at("output.weight");
        const size_t gb = (size_t)(c.dim / m->q4_gs) * 4;
        void* hq = nullptr;
        void* hs = nullptr;
        HIPCHK(hipMalloc(&hq, (size_t)(m->Nhead + 15) / 16 * 16 * c.dim));
        HIPCHK(hipMalloc(&hs, (size_t)(m->Nhead + 15) / 16 * 16 * gb));
        HIPCHK(hipMemcpyAsync(hq, (const char*)o.q + (size_t)c.semantic_begin_id * c.dim, (size_t)m->nsem * c.dim,
                              hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpyAsync((char*)hq + (size_t)m->nsem * c.dim, (const char*)o.q + (size_t)c.im_end_id * c.dim,
                              c.dim, hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(hs, (const char*)o.s + (size_t)c.semantic_begin_id * gb, (size_t)m->nsem * gb,
                              hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpyAsync((char*)hs + (size_t)m->nsem * gb, (const char*)o.s + (size_t)c.im_end_id * gb, gb,
                              hipMemcpyDeviceToDevice, m->stream));
        fm_llm::QInfo qi = pack_q4_dev(m, hq, hs, m->Nhead, c.dim);
        qi.compact = m->compact;
        FMCHECK(qi.q8 || !m->compact, "compact: no int4 code layout for output.weight");
        if (qi.q8) m->qmap[m->head_c] = qi;
        HIPCHK(hipStreamSynchronize(m->stream));
        for (void* p : {hq, hs, o.q, o.s}) HIPCHK(hipFree(p));
        o.q = o.s = nullptr;
    } else if (m->quant && !c.tie_word_embeddings) {  // the same compact rows of the int8 head and its scales
        DTensor& o = m->w.at("output.weight");
        m->mem_cat = 1;
        void* hq = m->dalloc((size_t)(m->Nhead + 15) / 16 * 16 * c.dim);
        HIPCHK(hipMemcpyAsync(hq, (const char*)o.q + (size_t)c.semantic_begin_id * c.dim, (size_t)m->nsem * c.dim,
                              hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpyAsync((char*)hq + (size_t)m->nsem * c.dim, (const char*)o.q + (size_t)c.im_end_id * c.dim,
                              c.dim, hipMemcpyDeviceToDevice, m->stream));
        void* hs = m->dalloc((size_t)(m->Nhead + 15) / 16 * 16 * m->esz);
        HIPCHK(hipMemcpyAsync(hs, (const char*)o.s + (size_t)c.semantic_begin_id * m->esz, (size_t)m->nsem * m->esz,
                              hipMemcpyDeviceToDevice, m->stream));
        HIPCHK(hipMemcpyAsync((char*)hs + (size_t)m->nsem * m->esz, (const char*)o.s + (size_t)c.im_end_id * m->esz,
                              m->esz, hipMemcpyDeviceToDevice, m->stream));
        m->mem_cat = 6;
        m->qmap[m->head_c] = fm_llm::QInfo{(const unsigned char*)pack_q8_dev(m, hq, m->Nhead, c.dim), hs, nullptr,
                                           pack_q8s_dev(m, hq, m->Nhead, c.dim), nullptr, m->compact};
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipFree(o.q));
        o.q = nullptr;
    }
    if (m->compact && head_q) {  // the whole table's T copy served only the head rows above
        DTensor& o = m->w.at("output.weight");
        if (o.p) HIPCHK(hipFree(o.p));
        o.p = nullptr;
    }
    // every tensor still held as uploaded: embeddings, norms, biases, an untied head's table (int8: the row scales)
    for (auto& kv : m->w) {
        const DTensor& t = kv.second;
        if (!t.p || is_linear_weight(kv.first)) continue;
        const int64_t rows = t.rows > 1 ? (t.rows + 15) / 16 * 16 : 1;
        const std::string& n = kv.first;
        const bool scales = n.size() > 7 && n.compare(n.size() - 7, 7, ".scales") == 0;
        m->mem[scales ? 1 : 4] += rows * t.cols * (int64_t)m->esz;
    }
    // caches [slot][layer][kv][S][hd]
    const StackDims& d = m->sd;
    m->layer_stride = (size_t)d.nkv * m->S * d.hd;
    m->slot_stride = m->layer_stride * d.n_layer;
    m->mem_cat = 5;
    m->kc = m->dalloc(m->slot_stride * m->max_slots * m->esz);
    m->vc = m->dalloc(m->slot_stride * m->max_slots * m->esz);
    const StackDims& f = m->fdm;
    m->flayer_stride = (size_t)f.nkv * m->C * f.hd;
    m->fslot_stride = m->flayer_stride * f.n_layer;
    m->fkc = m->dalloc(m->fslot_stride * m->max_slots * m->esz);
    m->fvc = m->dalloc(m->fslot_stride * m->max_slots * m->esz);
    m->mem_cat = 6;
    auto rt = rope_table_host(m->S, d.hd, c.rope_base);
    m->rope = (float*)m->dalloc(rt.size() * 4, false);
    HIPCHK(hipMemcpy(m->rope, rt.data(), rt.size() * 4, hipMemcpyHostToDevice));
    auto frt = rope_table_host(m->C, f.hd, c.rope_base);
    m->frope = (float*)m->dalloc(frt.size() * 4, false);
    HIPCHK(hipMemcpy(m->frope, frt.data(), frt.size() * 4, hipMemcpyHostToDevice));
    // activations
    const int R = m->Rmax = std::max(m->max_slots, PREFILL_CHUNK);
    const int dmax = std::max(c.dim, c.fast_dim);
    const int qkvmax = std::max(d.nqkv(), f.nqkv()), qmax = std::max(d.nq(), f.nq());
    const int imax = std::max(d.inter, f.inter);
    const size_t E = m->esz;
    m->x = m->dalloc((size_t)R * dmax * E);
    m->h = m->dalloc((size_t)R * dmax * E);
    m->xn = m->dalloc((size_t)R * dmax * E);
    m->qkv = m->dalloc((size_t)R * qkvmax * E);
    m->q = m->dalloc((size_t)R * qmax * E);
    m->att = m->dalloc((size_t)R * qmax * E);
    m->act = m->dalloc((size_t)R * imax * E);
    m->act2 = m->dalloc((size_t)R * 2 * imax * E);
    const int n = m->max_slots;
    m->xl = m->dalloc((size_t)n * dmax * E);
    m->plast = m->dalloc((size_t)n * dmax * E);
    m->xnl = m->dalloc((size_t)n * dmax * E);
    // (the fast residual rows hold two rows on a one-slot handle too: fm_tune fast_pair's paired pass)
    m->fx = m->dalloc((size_t)std::max(n, 2) * dmax * E);
    m->fh = m->dalloc((size_t)std::max(n, 2) * dmax * E);
    m->fxn = m->dalloc((size_t)n * dmax * E);
    m->x2 = m->dalloc((size_t)std::min(n, GEMV_MAX_ROWS) * dmax * E);
    m->fx2 = m->dalloc((size_t)std::max(std::min(n, GEMV_MAX_ROWS), 2) * dmax * E);
    m->chain_cnt = (unsigned*)m->dalloc(GEMV_CHAIN_WORDS * sizeof(unsigned));
    m->chain_err = (int*)m->dalloc(16 * sizeof(int));
    HIPCHK(hipHostMalloc((void**)&m->h_chain_err, 16 * sizeof(int), hipHostMallocDefault));
    m->h_chain_err[0] = 0;
    m->maxsplit = FM_CEIL(m->S, ATTN_SPLIT);
    const int Rpart = std::max(m->max_slots, ATTN_PIECE);  // decode rows, or one prompt attention piece
    m->part = (float*)m->dalloc((size_t)Rpart * d.nh * std::max(m->maxsplit, FM_CEIL(m->S, 16)) * (d.hd + 2) * 4, false);
    m->attn_cnt = (int*)m->dalloc((size_t)R * d.nkv * sizeof(int));  // tickets: zeroed
    m->ssX = (float*)m->dalloc((size_t)(dmax / 16) * std::min(n, 32) * 4);  // batched chain: up to 32 rows
    m->ssH = (float*)m->dalloc((size_t)(dmax / 16) * std::min(n, 32) * 4);
    {
        // arrival counters: one per 16-row tile of the largest decode GEMV (the slow head / W13)
        const int maxn = std::max({m->Nhead, 2 * c.intermediate_size, 2 * c.fast_intermediate_size, qkvmax, dmax, m->cb});  // W1||W3 is one 2*I-row linear on the batched path
        m->tickets = (int*)m->dalloc((size_t)(maxn / 16 + 16) * sizeof(int));
        m->fin_cnt = (int*)m->dalloc((size_t)std::max(m->max_slots, 64) * 2 * sizeof(int));
        m->fin_ss = (float*)m->dalloc((size_t)std::max(m->max_slots, 64) * 16 * sizeof(float));
        m->skpart_cap = 16ll << 20;  // 64 MiB of partial tiles (prompt GEMM slabs: 256 rows x 2 x 19456)
        m->skpart = (float*)m->dalloc((size_t)m->skpart_cap * sizeof(float), false);
    }
    HIPCHK(hipMemsetAsync(m->attn_cnt, 0, (size_t)R * d.nkv * sizeof(int), m->stream));
    m->slabA = (float*)m->dalloc((size_t)KSB_MAX * std::min(n, GEMV_MAX_ROWS) * dmax * 4);
    m->slabB = (float*)m->dalloc((size_t)KSB_MAX * std::min(n, GEMV_MAX_ROWS) * dmax * 4);
    if (n > GEMV_MAX_ROWS) {  // [BS_KPARTS][32][dmax] fp32 each
        m->bsA = (float*)m->dalloc((size_t)BS_KPARTS * 32 * dmax * 4, false);
        m->bsB = (float*)m->dalloc((size_t)BS_KPARTS * 32 * dmax * 4, false);
        m->bsQ = (float*)m->dalloc((size_t)BS_KPARTS * 32 * std::max(m->sd.nqkv(), m->fdm.nqkv()) * 4, false);
    }
    m->logits = (float*)m->dalloc((size_t)n * m->Nhead * 4);
    m->flogits = (float*)m->dalloc((size_t)n * m->cb * 4);
    m->frame_slot = (int*)m->dalloc(n * 4);
    m->frame_pos = (int*)m->dalloc(n * 4);
    m->prow_slot = (int*)m->dalloc(PREFILL_CHUNK * 4);
    m->prow_pos = (int*)m->dalloc(PREFILL_CHUNK * 4);
    m->pfx_slots = (int*)m->dalloc((size_t)n * 4);
    m->tok_in = (int32_t*)m->dalloc((size_t)n * m->C1 * 4);
    m->cols = (int32_t*)m->dalloc((size_t)n * m->C1 * 4);
    m->ptok = (int32_t*)m->dalloc((size_t)PREFILL_CHUNK * m->C1 * 4);
    m->ras = (int32_t*)m->dalloc((size_t)n * m->C1 * 10 * 4);
    m->sp = (SlotParams*)m->dalloc(sizeof(SlotParams) * n);
    m->force_cols = (int32_t*)m->dalloc((size_t)n * m->C1 * 4);
    m->tap_slow = (float*)m->dalloc((size_t)n * m->Nhead * 4);
    m->tap_fast = (float*)m->dalloc((size_t)n * std::max(m->C - 1, 1) * m->cb * 4);
    m->host_force.assign(n, 0);
    HIPCHK(hipHostMalloc((void**)&m->h_cols, (size_t)2 * n * m->C1 * 4, hipHostMallocDefault));
    m->host_pos.assign(n, 0);
    m->host_step.assign(n, 0);
    HIPCHK(hipStreamSynchronize(m->stream));
    m->finalized = true;
}
