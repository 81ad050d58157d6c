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

static bool ends(const std::string& n, const char* suf) {
    const size_t L = strlen(suf);
    return n.size() >= L && n.compare(n.size() - L, L, suf) == 0;
}
static bool is_ffn_w13(const std::string& n) { return ends(n, "feed_forward.w1.weight") || ends(n, "feed_forward.w3.weight"); }
static bool is_linear_weight(const std::string& n) {
    return ends(n, "attention.wqkv.weight") || ends(n, "attention.wo.weight") || is_ffn_w13(n) ||
           ends(n, "feed_forward.w2.weight") || n == "fast_output.weight" || n == "fast_project_in.weight";
}

// every nn.Linear of the model (WeightOnlyInt8QuantHandler quantizes them all, quantize.py:190-206);
// the tied head is F.linear on the embedding table, not a module, and stays in T
bool is_quant_linear(const std::string& n) { return is_linear_weight(n) || n == "output.weight"; }
std::string base_of(const std::string& n) { return n.substr(0, n.size() - strlen(".weight")); }

static size_t pad16(int64_t rows) { return (size_t)(rows + 15) / 16 * 16; }

// Every buffer a Linear reads is the handle's until close (fm_llm::allocs) and booked under one class of
// fm_llm_memory_info: a new one ...
static void* keep_alloc(fm_llm* m, size_t bytes, int cat, bool zero = false) {
    m->mem_cat = cat;
    void* p = m->dalloc(bytes, zero);
    m->mem_cat = 6;
    return p;
}
// ... or a tensor's own buffer that its Linear goes on reading
static void keep(fm_llm* m, const void* p, size_t bytes, int cat) {
    m->allocs.push_back(const_cast<void*>(p));
    m->mem[cat] += (int64_t)bytes;
}
// finalize's temporaries: freed (null: none) once the stream's work on them is done
static void* tmp_alloc(std::vector<void*>& tmp, size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    tmp.push_back(p);
    return p;
}
static void free_dev(fm_llm* m, const std::vector<void*>& ps) {
    HIPCHK(hipStreamSynchronize(m->stream));
    for (void* p : ps)
        if (p) HIPCHK(hipFree(p));
}

// int8 row-major [rows][cols] (rows padded to 16) -> packed int8 decode-GEMV layout
static const unsigned char* pack_q8_dev(fm_llm* m, const void* q, int rows, int cols) {
    FMCHECK(cols % 64 == 0, "int8 weights need in_features % 64 == 0");
    void* dst = keep_alloc(m, pad16(rows) * cols, 1);
    launch_pack_q8(m->stream, (const int8_t*)q, rows, cols, (int8_t*)dst);
    HIPCHK(hipGetLastError());
    return (const unsigned char*)dst;
}

// the batched linears' step-granular copy of the same codes: only where bsacc_kernel can take it (int8,
// bf16, a handle with more than GEMV_MAX_ROWS slots); a max_slots <= 8 handle allocates nothing here -- unless it is
// compact: there the copy is what linear_kernel's code form reads, whatever max_slots is
static const unsigned char* pack_q8s_dev(fm_llm* m, const void* q, int rows, int cols) {
    if (m->quant != FM_QUANT_INT8 || m->prec != FM_PREC_BF16 || (m->max_slots <= GEMV_MAX_ROWS && !m->compact) || cols % 32)
        return nullptr;
    void* dst = keep_alloc(m, pad16(rows) * cols, 2);
    launch_pack_q8s(m->stream, (const int8_t*)q, rows, cols, (int8_t*)dst);
    HIPCHK(hipGetLastError());
    return (const unsigned char*)dst;
}

// int4: codes row-major [L.N][L.K] + sz [L.N][L.K / gs] -> the packed GEMV stream and its (scale, zero) table; none
// (the bf16 dequantised copy serves every kernel) unless the group size and K are whole 128-k units
static void pack_q4_dev(fm_llm* m, Linear& L, const void* q, const void* sz) {
    const int rows = L.N, cols = L.K;
    if (m->q4_gs % 128 || cols % 128) return;
    const size_t tiles = pad16(rows) / 16;
    void* dq = keep_alloc(m, tiles * 16 * cols / 2, 1);
    void* ds = keep_alloc(m, tiles * (cols / 128) * 16 * 4, 1);
    launch_pack_q4(m->stream, (const uint8_t*)q, rows, cols, (uint8_t*)dq);
    launch_pack_sz4(m->stream, (const uint32_t*)sz, rows, cols, m->q4_gs, (uint32_t*)ds);
    HIPCHK(hipGetLastError());
    L.q8 = (const unsigned char*)dq;
    L.sz = (const uint32_t*)ds;
    // the batched linears' step-granular copy of the same codes (they stream it with ds): only where
    // bsacc_kernel can take it -- bf16, a handle with more than GEMV_MAX_ROWS slots; a max_slots <= 8
    // handle allocates nothing here (a compact one does: linear_kernel's code form reads it).  Its own allocation:
    // row_copies 0 frees none of it.
    if (m->prec == FM_PREC_BF16 && (m->max_slots > GEMV_MAX_ROWS || m->compact)) {
        void* d4 = keep_alloc(m, tiles * 16 * cols / 2, 2);
        launch_pack_q4s(m->stream, (const uint8_t*)q, rows, cols, (uint32_t*)d4);
        HIPCHK(hipGetLastError());
        L.q4s = (const uint32_t*)d4;
    }
}

// int8 mode, before packing: every quantized linear ends with t.p = T(q) row-major (what the
// T-fragment kernels read), t.q = int8 row-major, t.s = row scales.  int8 checkpoints supply q and
// "<name>.scales"; float weights are quantized here with quantize.py's per-channel rule.
static void quantize_linears(fm_llm* m) {
    if (m->quant == FM_QUANT_INT4) {  // every linear: codes, group (scale, zero), dequantised bf16 in place
        for (auto& kv : m->w) {
            if (!is_quant_linear(kv.first)) continue;
            DTensor& t = kv.second;
            const size_t rp = pad16(t.rows);
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
        return;
    }
    for (auto& kv : m->w) {
        if (!is_quant_linear(kv.first)) continue;
        DTensor& t = kv.second;
        const size_t rp = pad16(t.rows);
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
            t.s = keep_alloc(m, rp * m->esz, 1, true);  // (the int8 row scales belong to the decode-GEMV units)
            if (m->prec == FM_PREC_BF16)
                launch_quant_rows<bf16_t>(m->stream, (bf16_t*)t.p, (int)t.rows, (int)t.cols, (int8_t*)t.q, (bf16_t*)t.s);
            else
                launch_quant_rows<float>(m->stream, (float*)t.p, (int)t.rows, (int)t.cols, (int8_t*)t.q, (float*)t.s);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(m->stream));
}

// row-major [rows][cols] device tensor -> packed fragment layout (fm_kernels.h)
// (booked as the fragment copy of a quantised linear, qlin, or as any other weight)
static void* pack_dev(fm_llm* m, const void* src, int rows, int cols, bool qlin) {
    void* dst = keep_alloc(m, pad16(rows) * cols * m->esz, qlin ? 0 : 4);
    if (m->prec == FM_PREC_BF16)
        launch_pack<bf16_t>(m->stream, (const bf16_t*)src, rows, cols, (bf16_t*)dst);
    else
        launch_pack<float>(m->stream, (const float*)src, rows, cols, (float*)dst);
    HIPCHK(hipGetLastError());
    return dst;
}

// The layouts every linear has, from its row-major forms.  The fragment copy of the T weight p [N][K]; a compact
// handle packs none of a quantised linear, qlin (p null: its int8 checkpoint tensor was never expanded) ...
static Linear frag_linear(fm_llm* m, const void* p, int N, int K, bool qlin) {
    Linear L;
    L.N = N;
    L.K = K;
    if (!(m->compact && qlin)) L.frag = pack_dev(m, p, N, K, qlin);
    return L;
}
// ... and the code layouts of a quantised linear, from its codes q and their row scales / group (scale, zero) rows s
static void pack_codes(fm_llm* m, Linear& L, const std::string& name, const void* q, const void* s) {
    if (m->quant == FM_QUANT_INT4) {
        pack_q4_dev(m, L, q, s);
        FMCHECK(L.q8 || !m->compact, "compact: no int4 code layout for " + name);
    } else {
        L.q8 = pack_q8_dev(m, q, L.N, L.K);
        L.scale = s;
        L.q8s = pack_q8s_dev(m, q, L.N, L.K);
    }
}

// bf16 wo / w2 / wqkv whose shapes the row-block GEMV takes keep their row-major copy
// (fm_rowgemv.hip; ~3.7 GB at S2-Pro beside the packed tiles the batched paths read)
// fm_tune row_copies 0: a row-major copy only where the rowgemv bits in force at finalize use it
static bool row_bits(fm_llm* m, int bits) {
    const FmTuning& t = fm_tuning();
    return t.row_copies || ((m->quant == FM_QUANT_INT4 ? t.rowgemv_q4 : t.rowgemv) & bits) != 0;
}
// (bf16: the T row-major weight; weight-only int8 / int4: the row-major codes, rowgemv QM 1 / 2)
static bool row_shape_ok(fm_llm* m, int cols) {
    const int qm = m->qmode();
    return m->prec == FM_PREC_BF16 && rowgemv_u(cols, qm) > 0 && (qm != 2 || (m->q4_gs % 8 == 0 && cols % m->q4_gs == 0));
}
static bool row_keep(fm_llm* m, const std::string& n, int rows, int cols) {
    if (!row_shape_ok(m, cols)) return false;
    if (ends(n, "attention.wo.weight") || ends(n, "feed_forward.w2.weight")) return rows % 2 == 0 && row_bits(m, 1);
    const bool u8 = rows % 8 == 0 && rowgemv_u(cols, m->qmode()) <= 8;
    if (n == "fast_output.weight") return u8 && row_bits(m, 8);
    return ends(n, "attention.wqkv.weight") && u8 && row_bits(m, 2 | 16);
}

// wqkv, wo, w2, the codebook head, fast_project_in: the tensor's row-major buffers are packed, then handed to the
// row-block GEMV where it takes the shape (row_keep), else freed
static Linear plain_linear(fm_llm* m, const std::string& n) {
    auto it = m->w.find(n);
    FMCHECK(it != m->w.end() && it->second.set, "tensor not set: " + n);
    DTensor& t = it->second;
    const int N = (int)t.rows, K = (int)t.cols;
    Linear L = frag_linear(m, t.p, N, K, m->quant != FM_QUANT_NONE);
    if (m->quant) pack_codes(m, L, n, t.q, t.s);
    const bool rk = row_keep(m, n, N, K);
    if (rk && m->quant == FM_QUANT_INT4) {  // the codes as packed row-major words + the row-major (scale, zero) table
        void* rw = keep_alloc(m, (size_t)N * K / 2, 3);
        launch_pack_q4_rows(m->stream, (const uint8_t*)t.q, N, K, (uint32_t*)rw);
        HIPCHK(hipGetLastError());
        L.rm = rw;
        L.rm_sz = (const uint32_t*)t.s;
        keep(m, t.s, pad16(N) * (K / m->q4_gs) * 4, 3);
    } else if (rk && m->quant) {  // the int8 codes, row-major, and the row scales as they are
        L.rm = t.q;
        L.rm_scale = t.s;
        keep(m, t.q, pad16(N) * K, 3);
    } else if (rk) {
        L.rm = t.p;
        keep(m, t.p, pad16(N) * K * m->esz, 3);
    }
    // (int4's group rows are this tensor's own allocation; int8's row scales are not: quantize_linears)
    std::vector<void*> done{t.q, m->quant == FM_QUANT_INT4 ? t.s : nullptr, t.p};
    for (void*& p : done)
        if (p == L.rm || p == L.rm_sz) p = nullptr;
    free_dev(m, done);
    t.p = t.q = t.s = nullptr;
    return L;
}

// dst [2 * rows] rows of rb bytes: per block, rpb rows of a then the same rpb rows of b
static void* interleave_rows(fm_llm* m, void* dst, const void* a, const void* b, int rows, int rpb, size_t rb) {
    HIPCHK(hipMemcpy2DAsync(dst, 2 * rpb * rb, a, rpb * rb, rpb * rb, rows / rpb, hipMemcpyDeviceToDevice, m->stream));
    HIPCHK(hipMemcpy2DAsync((char*)dst + rpb * rb, 2 * rpb * rb, b, rpb * rb, rpb * rb, rows / rpb, hipMemcpyDeviceToDevice,
                            m->stream));
    return dst;
}

// W1 [inter][dim] and W3 -> one packed [2*inter][dim] matrix whose 16-row tiles hold 8 rows of W1
// then the same 8 rows of W3, so one GEMV tile (EPI_SWIGLU8) has both halves of 8 SwiGLU outputs and
// the decode grid is 2*inter/16 single-matrix blocks.  The row-major W1/W3 are freed; their map
// entries keep the shapes.
static Linear w13_linear(fm_llm* m, const std::string& p, int inter, int dim) {
    FMCHECK(inter % 8 == 0, "intermediate_size must be a multiple of 8");
    DTensor& t1 = m->w.at(p + "feed_forward.w1.weight");
    DTensor& t3 = m->w.at(p + "feed_forward.w3.weight");
    const int qm = m->qmode();
    // bytes per row: the T weight, its codes (one byte each), their row scale or group (scale, zero) words
    const size_t E = m->esz, rb = (size_t)dim * E, qb = (size_t)dim, sb = qm == 2 ? (size_t)(dim / m->q4_gs) * 4 : E;
    const size_t n2 = 2 * (size_t)inter;
    std::vector<void*> tmp, ptmp;
    auto il = [&](void* dst, const void* a1, const void* a3, int rpb, size_t bytes) {
        return interleave_rows(m, dst, a1, a3, inter, rpb, bytes);
    };
    // the tile kernels' 8 + 8 interleave of the rows ...
    const void* pt = m->compact ? nullptr : il(tmp_alloc(ptmp, n2 * rb), t1.p, t3.p, 8, rb);
    Linear L = frag_linear(m, pt, 2 * inter, dim, qm != 0);
    // the row-block GEMV's copy (fm_rowgemv.hip ROWGEMV_NORM_SWIGLU): row-major, rows 4b .. 4b+3 of W1
    // then the same rows of W3, per 8-row block (bf16 rows, or int8 codes + scales, or int4 packed
    // code words + (scale, zero) rows)
    if (inter % 4 == 0 && row_shape_ok(m, dim) && rowgemv_u(dim, qm) <= 8 && row_bits(m, 4)) {
        if (qm == 2) {  // one byte per code, interleaved, then packed to row words
            std::vector<void*> ctmp;
            const void* codes = il(tmp_alloc(ctmp, n2 * qb), t1.q, t3.q, 4, qb);
            void* words = keep_alloc(m, n2 * qb / 2, 3);
            launch_pack_q4_rows(m->stream, (const uint8_t*)codes, 2 * inter, dim, (uint32_t*)words);
            HIPCHK(hipGetLastError());
            free_dev(m, ctmp);
            L.rm = words;
            L.rm_sz = (const uint32_t*)il(keep_alloc(m, n2 * sb, 3), t1.s, t3.s, 4, sb);
        } else {
            L.rm = qm ? il(keep_alloc(m, n2 * qb, 3), t1.q, t3.q, 4, qb) : il(keep_alloc(m, n2 * rb, 3), t1.p, t3.p, 4, rb);
            if (qm) L.rm_scale = il(keep_alloc(m, n2 * sb, 3), t1.s, t3.s, 4, sb);
        }
    }
    if (qm) {  // ... and the same interleave of the code rows and of their scale / (scale, zero) rows
        const void* qt = il(tmp_alloc(tmp, n2 * qb), t1.q, t3.q, 8, qb);
        // (int8: the row scales the code layouts go on reading; int4: pack_q4_dev repacks the group rows)
        const void* st = il(qm == 1 ? keep_alloc(m, n2 * sb, 1) : tmp_alloc(tmp, n2 * sb), t1.s, t3.s, 8, sb);
        pack_codes(m, L, p + "feed_forward.w1.weight", qt, st);
    }
    // (int4's group rows are the tensors' own allocations; int8's row scales are not: quantize_linears)
    // (freed codes first, T rows last: see finalize on the order)
    tmp.insert(tmp.end(), {t1.q, t3.q, qm == 2 ? t1.s : nullptr, qm == 2 ? t3.s : nullptr});
    tmp.insert(tmp.end(), ptmp.begin(), ptmp.end());
    tmp.insert(tmp.end(), {t1.p, t3.p});
    free_dev(m, tmp);
    for (DTensor* t : {&t1, &t3}) t->p = t->q = t->s = nullptr;
    return L;
}

// dst [Nhead padded to 16] rows of rb bytes: the constrained head's rows of the [vocab] table src -- the semantic
// rows, then <|im_end|>
static void* head_rows(fm_llm* m, void* dst, const void* src, size_t rb) {
    const fm_model_config& c = m->c;
    HIPCHK(hipMemcpyAsync(dst, (const char*)src + (size_t)c.semantic_begin_id * rb, (size_t)m->nsem * rb,
                          hipMemcpyDeviceToDevice, m->stream));
    HIPCHK(hipMemcpyAsync((char*)dst + (size_t)m->nsem * rb, (const char*)src + (size_t)c.im_end_id * rb, rb,
                          hipMemcpyDeviceToDevice, m->stream));
    return dst;
}

// constrained head (inference.py:308-320): only the semantic rows + <|im_end|> can be
// finite after the bias, so the LM head streams exactly those rows.
static Linear head_linear(fm_llm* m) {
    const fm_model_config& c = m->c;
    m->nsem = c.semantic_end_id - c.semantic_begin_id + 1;
    m->Nhead = m->nsem + 1;
    FMCHECK(m->Nhead <= 8192, "constrained head wider than 8192 rows is not supported");
    const size_t np = pad16(m->Nhead), rb = (size_t)c.dim * m->esz, qb = (size_t)c.dim;
    if (!m->quant || c.tie_word_embeddings) {  // (a tied head is the embedding table's rows: not a quantised linear)
        const void* table = c.tie_word_embeddings ? W(m, "embeddings.weight") : W(m, "output.weight");
        return frag_linear(m, head_rows(m, keep_alloc(m, np * rb, 4, true), table, rb), m->Nhead, c.dim, false);
    }
    // output.weight is a quantised linear: the same rows of its codes and of their scales / groups
    DTensor& o = m->w.at("output.weight");
    std::vector<void*> tmp;
    const bool q4 = m->quant == FM_QUANT_INT4;
    const size_t sb = q4 ? (size_t)(c.dim / m->q4_gs) * 4 : m->esz;
    const void* hp = m->compact ? nullptr : head_rows(m, keep_alloc(m, np * rb, 4, true), o.p, rb);
    Linear L = frag_linear(m, hp, m->Nhead, c.dim, true);
    const void* hq = head_rows(m, q4 ? tmp_alloc(tmp, np * qb) : keep_alloc(m, np * qb, 1, true), o.q, qb);
    const void* hs = head_rows(m, q4 ? tmp_alloc(tmp, np * sb) : keep_alloc(m, np * sb, 1, true), o.s, sb);
    pack_codes(m, L, "output.weight", hq, hs);
    // the table's codes (int4: and its own group rows) served only these rows; a compact handle's T copy too
    tmp.insert(tmp.end(), {o.q, q4 ? o.s : nullptr, m->compact ? o.p : nullptr});
    o.q = o.s = nullptr;
    if (m->compact) o.p = nullptr;
    free_dev(m, tmp);
    return L;
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
    // wqkv, wo, w2, the codebook head, fast_project_in (W1 / W3: w13_linear below), all before the first W1 || W3
    // and in the tensor map's order: the order of the allocations (and of the frees between them) decides where the
    // weights lie on the device, and the frame times follow it by a few tenths of a percent (profiles/linear_record.md)
    std::map<std::string, Linear> plain;
    for (auto& kv : m->w)
        if (is_linear_weight(kv.first) && !is_ffn_w13(kv.first)) plain[kv.first] = plain_linear(m, kv.first);
    m->row_ok = m->row_qkv_ok = m->row_w13_ok = true;
    auto stack = [&](const std::string& pre, const StackDims& d, std::vector<LayerW>& out) {
        out.resize(d.n_layer);
        for (int i = 0; i < d.n_layer; ++i) {
            std::string p = pre + std::to_string(i) + ".";
            LayerW& L = out[i];
            L.wqkv = plain.at(p + "attention.wqkv.weight");
            L.wo = plain.at(p + "attention.wo.weight");
            L.w13 = w13_linear(m, p, d.inter, d.dim);
            L.w2 = plain.at(p + "feed_forward.w2.weight");
            // WeightOnlyInt8Linear has no bias (quantize.py:206-229): the checkpoint's are unused
            L.bqkv = m->quant ? nullptr : Wopt(m, p + "attention.wqkv.bias");
            L.bo = m->quant ? nullptr : Wopt(m, p + "attention.wo.bias");
            L.qn = Wopt(m, p + "attention.q_norm.weight");
            L.kn = Wopt(m, p + "attention.k_norm.weight");
            L.an = W(m, p + "attention_norm.weight");
            L.fn = W(m, p + "ffn_norm.weight");
            m->row_ok = m->row_ok && L.wo.rm && L.w2.rm;
            m->row_qkv_ok = m->row_qkv_ok && L.wqkv.rm;
            m->row_w13_ok = m->row_w13_ok && L.w13.rm;
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
    // fm_tune slow_attn_wo: the slow layers' tagged attention words, one row (tags 0: never current), on the handles
    // whose batch-1 frame can take the fused launch (weight-only int8 / int4 ones under slow_attn_wo_q: the form of their codes)
    if (m->prec == FM_PREC_BF16 && (!m->quant || m->qmode()) && m->sd.n_layer >= 2 && m->sd.n_layer <= 40 &&
        slow_attn_wo_ok(m->sd.nh, m->sd.nkv, m->sd.hd, m->sd.dim, m->sd.nq(), m->qmode()))
        m->sxt = (uint32_t*)m->dalloc((size_t)m->sd.nq() * sizeof(uint32_t));
    m->emb = W(m, "embeddings.weight");
    m->cbemb = W(m, "codebook_embeddings.weight");
    m->norm = W(m, "norm.weight");
    if (plain.count("fast_project_in.weight")) m->fproj_w = plain.at("fast_project_in.weight");
    m->fproj_b = m->quant ? nullptr : Wopt(m, "fast_project_in.bias");
    m->femb = W(m, "fast_embeddings.weight");
    m->fnorm = W(m, "fast_norm.weight");
    m->fout = plain.at("fast_output.weight");
    m->head_c = head_linear(m);
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
    // tickets, zeroed: [rows][nkv] for attn_decode2 / attn_dec3 (rows of a chunk), [rows][nh] for attn_fd (one per row,
    // kv head and group of fd_hpb q heads; its rows are distinct slots, at most max_slots)
    const size_t ncnt = std::max((size_t)R * d.nkv, (size_t)m->max_slots * d.nh);
    m->attn_cnt = (int*)m->dalloc(ncnt * sizeof(int));
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
    HIPCHK(hipMemsetAsync(m->attn_cnt, 0, ncnt * sizeof(int), m->stream));
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
