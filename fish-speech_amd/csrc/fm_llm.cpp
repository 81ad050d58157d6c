// fm_llm.cpp -- host runtime of the Dual-AR decode path (C ABI in include/fishmi.h).
//
// One handle per GPU owns: the weights (bf16 or fp32), per-slot KV caches, per-slot sampler
// state (temperature/top_p/top_k/seed/step + RAS window), and the activation buffers.  A
// frame (one decode_one_token_ar for n slots, inference.py:96-181) is a fixed kernel sequence
// that reads every dynamic value (tokens, positions, steps) from device memory, so it is
// captured once per batch size into a hipGraph and replayed.
#include <math.h>

#include <memory>

#include "fm_llm_model.h"

static thread_local std::string g_err;
void fm_set_error(const std::string& s) { g_err = s; }
extern "C" const char* fm_last_error(void) { return g_err.c_str(); }
extern "C" int fm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static void check_tokens(fm_llm* m, const int32_t* tok, int T) {
    const fm_model_config& c = m->c;
    for (int t = 0; t < T; ++t) {
        const int t0 = tok[t];
        FMCHECK(t0 >= 0 && t0 < c.vocab_size, "token id out of range: " + std::to_string(t0));
        for (int q = 0; q < m->C; ++q) {
            const int v = tok[(size_t)(q + 1) * T + t];
            FMCHECK(v >= 0 && v < m->cb, "codebook token out of range: " + std::to_string(v));
        }
    }
}

static void reset_slot(fm_llm* m, int slot, const fm_sampling* sp) {
    HIPCHK(hipMemsetAsync((char*)m->ras + (size_t)slot * m->C1 * 10 * 4, 0, (size_t)m->C1 * 10 * 4, m->stream));
    SlotParams p{};
    if (sp) {
        // top_k <= 64: register/wave select; larger (the reference takes any, inference.py:54-77):
        // the whole row sorted in LDS (sample_wide)
        FMCHECK(sp->top_k >= 1, "top_k must be >= 1: got " + std::to_string(sp->top_k));
        p.temperature = sp->temperature;
        p.top_p = sp->top_p;
        p.top_k = sp->top_k;
        p.mask_im_end = sp->mask_im_end;
        p.seed = sp->seed;
    } else {
        p.temperature = 0.7f;
        p.top_p = 0.9f;
        p.top_k = 1;
    }
    p.step = 0;
    p.force = m->host_force[slot];
    HIPCHK(hipMemcpyAsync(m->sp + slot, &p, sizeof p, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->host_step[slot] = 0;
}

static void upload_frame_rows(fm_llm* m, const int32_t* slots, int n) {
    std::vector<int> s(slots, slots + n), p(n);
    if (s == m->uploaded_slots) return;
    for (int i = 0; i < n; ++i) p[i] = m->host_pos[s[i]];
    HIPCHK(hipMemcpyAsync(m->frame_slot, s.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->frame_pos, p.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->uploaded_slots = s;
}

// gemv chain health: the error word travels to pinned memory behind the frames; after the
// host's stream sync, a timed-out hand-off wait (a hang avoided) resets the counters and fails
static void chain_err_async(fm_llm* m) {
    if (fm_tuning().gemv_chain || fm_tuning().fin_split > 1 ||
        (m->fxt && fm_tuning().fattn_wo) || (m->sxt && (m->quant ? fm_tuning().slow_attn_wo_q : fm_tuning().slow_attn_wo)))
        HIPCHK(hipMemcpyAsync(m->h_chain_err, m->chain_err, sizeof(int), hipMemcpyDeviceToHost, m->stream));
}
static void chain_err_check(fm_llm* m) {
    if (!m->h_chain_err || !m->h_chain_err[0]) return;
    m->h_chain_err[0] = 0;
    HIPCHK(hipMemset(m->chain_cnt, 0, GEMV_CHAIN_WORDS * sizeof(unsigned)));
    HIPCHK(hipMemset(m->chain_err, 0, 16 * sizeof(int)));
    if (m->fin_cnt) HIPCHK(hipMemset(m->fin_cnt, 0, (size_t)std::max(m->max_slots, 64) * 2 * sizeof(int)));
    throw FmError{FM_ERR_STATE,
                  "in-launch hand-off wait timed out (gemv chain / split finalize / fused fast or slow "
                  "attention + wo; counters reset)"};
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int fm_llm_open(const fm_model_config* cfg, int device, int precision, int max_slots, fm_llm** out) {
    return fm_guard([&] {
        FMCHECK(cfg && out, "null argument");
        FMCHECK(precision == FM_PREC_BF16 || precision == FM_PREC_FP32, "bad precision");
        FMCHECK(max_slots >= 1 && max_slots <= 4096, "bad max_slots");
        const fm_model_config& c = *cfg;
        FMCHECK(c.dim % 32 == 0 && c.fast_dim % 32 == 0, "dims must be multiples of 32");
        FMCHECK(c.intermediate_size % 32 == 0 && c.fast_intermediate_size % 32 == 0,
                "intermediate sizes must be multiples of 32");
        FMCHECK((c.n_head * c.head_dim) % 32 == 0 && (c.fast_n_head * c.fast_head_dim) % 32 == 0,
                "n_head*head_dim must be a multiple of 32");
        FMCHECK(c.head_dim % 8 == 0 && c.head_dim <= 256 && c.fast_head_dim <= 256, "bad head_dim");
        FMCHECK(c.n_head % c.n_local_heads == 0 && c.fast_n_head % c.fast_n_local_heads == 0, "bad GQA");
        FMCHECK(c.num_codebooks >= 1 && c.num_codebooks <= 63, "bad num_codebooks");
        FMCHECK(c.codebook_size <= 8192, "codebook_size > 8192 unsupported");
        FMCHECK(c.im_end_id >= 0 && c.im_end_id < c.vocab_size, "im_end_id must be set");
        FMCHECK(c.semantic_begin_id >= 0 && c.semantic_end_id < c.vocab_size &&
                    c.semantic_begin_id <= c.semantic_end_id,
                "bad semantic id range");
        int ndev = fm_device_count();
        FMCHECK(ndev > 0, "no HIP device visible");
        FMCHECK(device >= 0 && device < ndev, "bad device index");
        HIPCHK(hipSetDevice(device));
        std::unique_ptr<fm_llm> m(new fm_llm());
        m->c = c;
        m->device = device;
        m->prec = precision;
        m->esz = precision == FM_PREC_BF16 ? 2 : 4;
        m->max_slots = max_slots;
        m->S = (c.max_seq_len + 7) / 8 * 8;
        m->C = c.num_codebooks;
        m->C1 = c.num_codebooks + 1;
        m->cb = c.codebook_size;
        HIPCHK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
        const char* g = getenv("FISHMI_GRAPH");  // FISHMI_GRAPH=0: eager launches (profilers)
        m->use_graph = !(g && g[0] == '0');
        build_inventory(m.get());
        *out = m.release();
    });
}

int fm_llm_set_quant_int4(fm_llm* m, int groupsize) {
    return fm_guard([&] {
        FMCHECK(m && (groupsize == 32 || groupsize == 64 || groupsize == 128 || groupsize == 256),
                "int4: groupsize must be 32, 64, 128 or 256 (WeightOnlyInt4QuantHandler, quantize.py:366)");
        FMCHECK(!m->finalized, "weights are frozen after finalize");
        for (auto& kv : m->w) FMCHECK(!kv.second.set, "set the quantization mode before any tensor");
        FMCHECK(m->quant == FM_QUANT_NONE, "quantization mode already set");
        FMCHECK(m->prec == FM_PREC_BF16, "int4: bf16 precision only (the reference quantizes the bf16 weights)");
        const fm_model_config& c = m->c;
        // create_quantized_state_dict asserts bias-free linears (quantize.py:371)
        FMCHECK(!c.qkv_bias && !c.o_bias && !c.fast_qkv_bias && !c.fast_o_bias,
                "int4: the linears must be bias-free (quantize.py:371)");
        for (auto& kv : m->w) {
            if (!is_quant_linear(kv.first)) continue;
            FMCHECK(kv.second.cols % groupsize == 0, "int4: in_features must be a multiple of the group size: " + kv.first);
            FMCHECK(m->w.find(base_of(kv.first) + ".bias") == m->w.end(),
                    "int4: the linears must be bias-free (quantize.py:371): " + kv.first);
        }
        m->quant = FM_QUANT_INT4;
        m->q4_gs = groupsize;
    });
}

int fm_llm_set_quant(fm_llm* m, int mode) {
    if (mode == FM_QUANT_INT4) return fm_llm_set_quant_int4(m, 128);
    return fm_guard([&] {
        FMCHECK(m && (mode == FM_QUANT_NONE || mode == FM_QUANT_INT8), "bad arguments");
        FMCHECK(!m->finalized, "weights are frozen after finalize");
        for (auto& kv : m->w) FMCHECK(!kv.second.set, "set the quantization mode before any tensor");
        if (mode == m->quant) return;
        FMCHECK(m->quant == FM_QUANT_NONE, "quantization mode already set");
        m->quant = mode;
        std::vector<std::pair<std::string, int64_t>> add;
        for (auto& kv : m->w) {
            if (!is_quant_linear(kv.first)) continue;
            FMCHECK(kv.second.cols % 64 == 0, "int8 weights need in_features % 64 == 0: " + kv.first);
            add.emplace_back(base_of(kv.first) + ".scales", kv.second.rows);
            auto b = m->w.find(base_of(kv.first) + ".bias");
            if (b != m->w.end()) b->second.optional = true;
        }
        for (auto& a : add) {
            add_t(m, a.first, 1, a.second);
            m->w[a.first].optional = true;
        }
    });
}

int fm_llm_set_quant_compact(fm_llm* m, int enable) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        auto state = [](bool ok, const char* msg) {
            if (!ok) throw FmError{FM_ERR_STATE, msg};
        };
        state(!m->finalized, "weights are frozen after finalize");
        FMCHECK(m->prec == FM_PREC_BF16, "compact: bf16 precision only (the code-reading kernel forms are bf16)");
        state(m->quant != FM_QUANT_NONE, "compact: set the quantization mode first (fm_llm_set_quant / fm_llm_set_quant_int4)");
        for (auto& kv : m->w) state(!kv.second.set, "compact: set it before any tensor");
        m->compact = enable != 0;
    });
}

int fm_llm_memory_info(fm_llm* m, int64_t out[8]) {
    return fm_guard([&] {
        FMCHECK(m && out, "null argument");
        if (!m->finalized) throw FmError{FM_ERR_STATE, "memory_info: finalize the handle first"};
        int64_t sum = 0;
        for (int i = 0; i < 7; ++i) sum += out[i] = m->mem[i];
        out[7] = sum;
    });
}

int fm_llm_set_tensor(fm_llm* m, const char* name, const void* data, int dtype, int64_t numel) {
    return fm_guard([&] {
        FMCHECK(m && name && data, "null argument");
        FMCHECK(!m->finalized, "weights are frozen after finalize");
        HIPCHK(hipSetDevice(m->device));
        if (dtype == FM_DT_I8) {  // an int8 checkpoint's weight (WeightOnlyInt8QuantHandler state_dict)
            FMCHECK(m->quant == FM_QUANT_INT8 && is_quant_linear(name), std::string("int8 data for ") + name +
                                                                             " needs fm_llm_set_quant(INT8) and a linear weight");
            auto it = m->w.find(name);
            FMCHECK(it != m->w.end() && it->second.numel == numel, std::string("unknown tensor or wrong numel: ") + name);
            DTensor& t = it->second;
            FMCHECK(!t.set, std::string("tensor set twice: ") + name);
            const size_t bytes = (size_t)(t.rows + 15) / 16 * 16 * t.cols;
            HIPCHK(hipMalloc(&t.q, bytes));
            HIPCHK(hipMemsetAsync(t.q, 0, bytes, m->stream));
            HIPCHK(hipMemcpyAsync(t.q, data, (size_t)numel, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));
            t.set = true;
            return;
        }
        DTensor& t = tensor_for(m, name, numel);
        const size_t sb = dtype == FM_DT_BF16 ? 2 : 4;
        void* tmp = nullptr;
        HIPCHK(hipMalloc(&tmp, (size_t)numel * sb));
        HIPCHK(hipMemcpy(tmp, data, (size_t)numel * sb, hipMemcpyHostToDevice));
        if (m->prec == FM_PREC_BF16)
            launch_convert<bf16_t>(m->stream, tmp, dtype == FM_DT_BF16, numel, (bf16_t*)t.p);
        else
            launch_convert<float>(m->stream, tmp, dtype == FM_DT_BF16, numel, (float*)t.p);
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipFree(tmp));
        t.set = true;
    });
}

int fm_llm_synth_tensor(fm_llm* m, const char* name, int64_t numel, uint64_t seed, float center,
                        int log2_half) {
    return fm_guard([&] {
        FMCHECK(m && name, "null argument");
        FMCHECK(!m->finalized, "weights are frozen after finalize");
        HIPCHK(hipSetDevice(m->device));
        DTensor& t = tensor_for(m, name, numel);
        if (m->prec == FM_PREC_BF16)
            launch_synth<bf16_t>(m->stream, (bf16_t*)t.p, numel, seed, fnv1a32(name), center, log2_half);
        else
            launch_synth<float>(m->stream, (float*)t.p, numel, seed, fnv1a32(name), center, log2_half);
        HIPCHK(hipGetLastError());
        t.set = true;
    });
}

int fm_llm_finalize(fm_llm* m) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        ensure_qkv0(m);
    });
}

// pos0 > 0 continues a slot whose positions [0, pos0) already hold the KV of the same tokens
// (prefix reuse across generate_long batches); the prompt suffix runs at pos0 .. pos0 + T - 1
static void do_prefill(fm_llm* m, int slot, const int32_t* tokens, int T, const fm_sampling* sp,
                       int32_t* first_col, int pos0 = 0) {
    FMCHECK(slot >= 0 && slot < m->max_slots, "bad slot");
    FMCHECK(T >= 1 && pos0 >= 0 && pos0 + T < m->c.max_seq_len, "prompt must end before max_seq_len");
    FMCHECK(pos0 <= m->host_pos[slot], "prefix reuse past the slot's cached positions");
    check_tokens(m, tokens, T);
    reset_slot(m, slot, sp);
    const int32_t one = slot;
    m->uploaded_slots.clear();
    HIPCHK(hipMemcpyAsync(m->frame_slot, &one, 4, hipMemcpyHostToDevice, m->stream));
    prefill_frame(m, slot, tokens, T, pos0);
    int pos = pos0 + T - 1;  // finish() advances it: the first decode frame runs at pos0 + T
    HIPCHK(hipMemcpyAsync(m->frame_pos, &pos, 4, hipMemcpyHostToDevice, m->stream));
    launch_finish(m->stream, 1, m->frame_slot, m->frame_pos, m->cols, m->C1, m->tok_in, m->ras,
                  m->C1 * 10, m->C1, 0, m->sp);
    HIPCHK(hipMemcpyAsync(m->h_cols, m->cols, (size_t)m->C1 * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->prof.collect();
    m->host_pos[slot] = pos0 + T;
    m->host_step[slot] = 1;
    m->uploaded_slots.clear();
    if (first_col) memcpy(first_col, m->h_cols, (size_t)m->C1 * 4);
}

// Several requests prefilled together (each from position 0 of its own slot, or -- pos0 given --
// request i after its slot's cached positions [0, pos0[i])): one pass of the slow stack over all
// their prompt rows, then one batched first frame (head + fast model + samplers) for their last
// rows -- the same columns as n separate do_prefill calls.
static void do_prefill_batch(fm_llm* m, int n, const int32_t* slots, const int32_t* tokens, const int32_t* T,
                             const fm_sampling* sps, int32_t* first_cols, const int32_t* pos0 = nullptr) {
    FMCHECK(n >= 1 && n <= m->max_slots, "bad request count");
    std::vector<const int32_t*> tk(n);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        FMCHECK(slots[i] >= 0 && slots[i] < m->max_slots, "bad slot");
        for (int j = 0; j < i; ++j) FMCHECK(slots[j] != slots[i], "duplicate slot");
        const int p0 = pos0 ? pos0[i] : 0;
        FMCHECK(T[i] >= 1 && p0 >= 0 && (int64_t)p0 + T[i] < m->c.max_seq_len, "prompt must end before max_seq_len");
        FMCHECK(p0 <= m->host_pos[slots[i]], "prefix reuse past the slot's cached positions");
        tk[i] = tokens + off;
        check_tokens(m, tk[i], T[i]);
        off += (size_t)m->C1 * T[i];
    }
    for (int i = 0; i < n; ++i) reset_slot(m, slots[i], sps ? sps + i : nullptr);
    m->uploaded_slots.clear();
    HIPCHK(hipMemcpyAsync(m->frame_slot, slots, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    prefill_batch_frame(m, n, slots, tk.data(), T, pos0);
    std::vector<int> pos(n);
    for (int i = 0; i < n; ++i) pos[i] = (pos0 ? pos0[i] : 0) + T[i] - 1;  // finish() advances it
    HIPCHK(hipMemcpyAsync(m->frame_pos, pos.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    launch_finish(m->stream, n, m->frame_slot, m->frame_pos, m->cols, m->C1, m->tok_in, m->ras, m->C1 * 10,
                  m->C1, 0, m->sp);
    HIPCHK(hipMemcpyAsync(m->h_cols, m->cols, (size_t)n * m->C1 * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->prof.collect();
    for (int i = 0; i < n; ++i) {
        m->host_pos[slots[i]] = (pos0 ? pos0[i] : 0) + T[i];
        m->host_step[slots[i]] = 1;
    }
    m->uploaded_slots.clear();
    if (first_cols) memcpy(first_cols, m->h_cols, (size_t)n * m->C1 * 4);
}

int fm_llm_prefill_batch(fm_llm* m, int n, const int32_t* slots, const int32_t* tokens, const int32_t* T,
                         const fm_sampling* sp, int32_t* first_cols) {
    return fm_guard([&] {
        FMCHECK(m && slots && tokens && T, "null argument");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        do_prefill_batch(m, n, slots, tokens, T, sp, first_cols);
    });
}

int fm_llm_prefill_batch_at(fm_llm* m, int n, const int32_t* slots, const int32_t* tokens, const int32_t* T,
                            const int32_t* pos0, const fm_sampling* sp, int32_t* first_cols) {
    return fm_guard([&] {
        FMCHECK(m && slots && tokens && T && pos0, "null argument");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        do_prefill_batch(m, n, slots, tokens, T, sp, first_cols, pos0);
    });
}

// one launch of the prefix copy kernel between entry `e` and the listed slots (checked by the caller)
static void prefix_copy(fm_llm* m, const fm_llm::Prefix& e, const int32_t* slots, int n, bool to_store) {
    const StackDims& d = m->sd;
    HIPCHK(hipMemcpyAsync(m->pfx_slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    KvPrefixArgs a{};
    a.kc = (char*)m->kc;
    a.vc = (char*)m->vc;
    a.store = (char*)e.buf;
    a.slots = m->pfx_slots;
    a.slot_stride_b = m->slot_stride * m->esz;
    a.layer_stride_b = m->layer_stride * m->esz;
    a.head_stride_b = (size_t)m->S * d.hd * m->esz;
    a.run_bytes = (size_t)e.npos * d.hd * m->esz;
    a.nkv = d.nkv;
    a.to_store = to_store ? 1 : 0;
    launch_kv_prefix_copy(m->stream, a, d.n_layer, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));  // the caller's slot list is free again; a failed copy fails here
}

static fm_llm::Prefix& prefix_of(fm_llm* m, int id) {
    auto it = m->prefixes.find(id);
    FMCHECK(it != m->prefixes.end(), "unknown or dropped prefix id " + std::to_string(id));
    return it->second;
}

int fm_llm_prefix_save(fm_llm* m, int slot, int npos, int* prefix_id) {
    return fm_guard([&] {
        FMCHECK(m && prefix_id, "null argument");
        FMCHECK(m->finalized, "prefix_save before any prefill");
        HIPCHK(hipSetDevice(m->device));
        FMCHECK(slot >= 0 && slot < m->max_slots, "bad slot");
        FMCHECK(npos >= 1 && npos <= m->host_pos[slot],
                "prefix_save: npos " + std::to_string(npos) + " outside [1, " + std::to_string(m->host_pos[slot]) +
                    "], the slot's cached positions");
        fm_llm::Prefix e;
        e.npos = npos;
        e.bytes = (size_t)m->sd.n_layer * 2 * m->sd.nkv * npos * m->sd.hd * m->esz;
        const hipError_t err = hipMalloc(&e.buf, e.bytes);
        if (err != hipSuccess) {
            (void)hipGetLastError();  // the failed allocation is reported here, not by the next launch
            throw FmError{FM_ERR_OOM, "prefix_save: hipMalloc(" + std::to_string(e.bytes) + ") failed: " +
                                          hipGetErrorString(err)};
        }
        try {
            const int32_t one = slot;
            prefix_copy(m, e, &one, 1, true);
        } catch (...) {
            (void)hipFree(e.buf);
            throw;
        }
        const int id = m->next_prefix_id++;
        m->prefixes[id] = e;
        *prefix_id = id;
    });
}

int fm_llm_prefix_load(fm_llm* m, int prefix_id, const int32_t* slots, int n) {
    return fm_guard([&] {
        FMCHECK(m && slots, "null argument");
        FMCHECK(m->finalized, "prefix_load before any prefill");
        HIPCHK(hipSetDevice(m->device));
        const fm_llm::Prefix& e = prefix_of(m, prefix_id);
        FMCHECK(n >= 1 && n <= m->max_slots, "bad slot count");
        for (int i = 0; i < n; ++i) {
            FMCHECK(slots[i] >= 0 && slots[i] < m->max_slots, "bad slot");
            for (int j = 0; j < i; ++j) FMCHECK(slots[j] != slots[i], "duplicate slot");
        }
        FMCHECK(e.npos <= m->S, "prefix longer than the slot cache");
        prefix_copy(m, e, slots, n, false);
        // the slots now hold the prefix as if they had just run those positions; their sampling records
        // and RAS windows stay as they are (the prefill that follows resets them)
        for (int i = 0; i < n; ++i) {
            m->host_pos[slots[i]] = e.npos;
            m->host_step[slots[i]] = 0;
        }
        m->uploaded_slots.clear();  // the frame rows on the device still carry the old positions
    });
}

int fm_llm_prefix_drop(fm_llm* m, int prefix_id) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        HIPCHK(hipSetDevice(m->device));
        const fm_llm::Prefix e = prefix_of(m, prefix_id);
        HIPCHK(hipStreamSynchronize(m->stream));
        m->prefixes.erase(prefix_id);
        HIPCHK(hipFree(e.buf));
    });
}

int fm_llm_prefix_info(fm_llm* m, int prefix_id, int* npos, int64_t* bytes) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        const fm_llm::Prefix& e = prefix_of(m, prefix_id);
        if (npos) *npos = e.npos;
        if (bytes) *bytes = (int64_t)e.bytes;
    });
}

int fm_llm_prefill(fm_llm* m, int slot, const int32_t* tokens, int T, const fm_sampling* sp,
                   int32_t* first_col) {
    return fm_guard([&] {
        FMCHECK(m && tokens, "null argument");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        do_prefill(m, slot, tokens, T, sp, first_col);
    });
}

int fm_llm_prefill_at(fm_llm* m, int slot, const int32_t* suffix, int T, int pos0, const fm_sampling* sp,
                      int32_t* first_col) {
    return fm_guard([&] {
        FMCHECK(m && suffix, "null argument");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        do_prefill(m, slot, suffix, T, sp, first_col, pos0);
    });
}

int fm_llm_decode(fm_llm* m, const int32_t* slots, int n, int32_t* cols) {
    return fm_guard([&] {
        FMCHECK(m && slots && n >= 1 && n <= m->max_slots, "bad arguments");
        FMCHECK(m->finalized, "call fm_llm_prefill first");
        HIPCHK(hipSetDevice(m->device));
        for (int i = 0; i < n; ++i) {
            FMCHECK(slots[i] >= 0 && slots[i] < m->max_slots, "bad slot");
            FMCHECK(m->host_pos[slots[i]] < m->c.max_seq_len, "slot reached max_seq_len");
        }
        upload_frame_rows(m, slots, n);
        launch_frame(m, n);
        HIPCHK(hipMemcpyAsync(m->h_cols, m->cols, (size_t)n * m->C1 * 4, hipMemcpyDeviceToHost, m->stream));
        chain_err_async(m);
        HIPCHK(hipStreamSynchronize(m->stream));
        chain_err_check(m);
        m->prof.collect();
        for (int i = 0; i < n; ++i) {
            m->host_pos[slots[i]]++;
            m->host_step[slots[i]]++;
        }
        if (cols) memcpy(cols, m->h_cols, (size_t)n * m->C1 * 4);
    });
}

int fm_llm_decode_frames(fm_llm* m, const int32_t* slots, int n, int nframes, int32_t* cols) {
    return fm_guard([&] {
        FMCHECK(m && slots && cols && n >= 1 && n <= m->max_slots && nframes >= 0, "bad arguments");
        FMCHECK(m->finalized, "call fm_llm_prefill first");
        HIPCHK(hipSetDevice(m->device));
        for (int i = 0; i < n; ++i) {
            FMCHECK(slots[i] >= 0 && slots[i] < m->max_slots, "bad slot");
            for (int j = 0; j < i; ++j) FMCHECK(slots[j] != slots[i], "duplicate slot");
            FMCHECK(m->host_pos[slots[i]] + nframes <= m->c.max_seq_len, "slot would pass max_seq_len");
        }
        if (nframes == 0) return;
        const size_t per = (size_t)n * m->C1;
        if (m->h_hist_n < per * nframes) {
            if (m->h_hist) HIPCHK(hipHostFree(m->h_hist));
            m->h_hist = nullptr;
            m->h_hist_n = 0;
            HIPCHK(hipHostMalloc((void**)&m->h_hist, per * nframes * 4, hipHostMallocDefault));
            m->h_hist_n = per * nframes;
        }
        upload_frame_rows(m, slots, n);
        // every frame is queued back to back; the columns stream to pinned memory behind them
        for (int k = 0; k < nframes; ++k) {
            launch_frame(m, n);
            HIPCHK(hipMemcpyAsync(m->h_hist + per * k, m->cols, per * 4, hipMemcpyDeviceToHost, m->stream));
        }
        chain_err_async(m);
        HIPCHK(hipStreamSynchronize(m->stream));
        chain_err_check(m);
        m->prof.collect();
        for (int i = 0; i < n; ++i) {
            m->host_pos[slots[i]] += nframes;
            m->host_step[slots[i]] += nframes;
        }
        memcpy(cols, m->h_hist, per * nframes * 4);
    });
}

static void do_generate(fm_llm* m, int slot, const int32_t* prompt, int T, int pos0, int max_new,
                        const fm_sampling* sp, int32_t* out, int* n_out) {
        FMCHECK(m && prompt && out && n_out, "null argument");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        const fm_model_config& c = m->c;
        if (max_new <= 0 || pos0 + T + max_new > c.max_seq_len) max_new = c.max_seq_len - pos0 - T;
        FMCHECK(max_new >= 1, "prompt leaves no room to generate");
        const int C1 = m->C1;
        int32_t col[64];
        do_prefill(m, slot, prompt, T, sp, col, pos0);
        for (int q = 0; q < C1; ++q) out[(size_t)q * max_new] = col[q];
        int n = 1;
        upload_frame_rows(m, &slot, 1);
        // pipelined: frame k+1 is queued before frame k's column is inspected on the host
        hipEvent_t ev[2];
        HIPCHK(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
        auto issue = [&](int k) {
            launch_frame(m, 1);
            HIPCHK(hipMemcpyAsync(m->h_cols + (size_t)(k & 1) * m->max_slots * C1, m->cols, (size_t)C1 * 4,
                                  hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipEventRecord(ev[k & 1], m->stream));
        };
        const int steps = max_new - 1;
        int issued = 0;
        if (steps > 0) issue(issued++);
        for (int k = 0; k < steps; ++k) {
            if (issued < steps && issued <= k + 1) issue(issued++);
            HIPCHK(hipEventSynchronize(ev[k & 1]));
            const int32_t* hc = m->h_cols + (size_t)(k & 1) * m->max_slots * C1;
            for (int q = 0; q < C1; ++q) out[(size_t)q * max_new + n] = hc[q];
            n++;
            if (hc[0] == c.im_end_id) break;
        }
        chain_err_async(m);
        HIPCHK(hipStreamSynchronize(m->stream));
        chain_err_check(m);
        m->prof.collect();
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
        m->host_pos[slot] = pos0 + T + issued;  // device advanced once per issued frame
        m->host_step[slot] = 1 + issued;
        m->uploaded_slots.clear();
        *n_out = n;
}

int fm_llm_generate(fm_llm* m, int slot, const int32_t* prompt, int T, int max_new, const fm_sampling* sp,
                    int32_t* out, int* n_out) {
    return fm_guard([&] { do_generate(m, slot, prompt, T, 0, max_new, sp, out, n_out); });
}

int fm_llm_generate_at(fm_llm* m, int slot, const int32_t* suffix, int T, int pos0, int max_new,
                       const fm_sampling* sp, int32_t* out, int* n_out) {
    return fm_guard([&] { do_generate(m, slot, suffix, T, pos0, max_new, sp, out, n_out); });
}

int fm_llm_slot_pos(fm_llm* m, int slot, int* pos) {
    return fm_guard([&] {
        FMCHECK(m && pos && slot >= 0 && slot < m->max_slots, "bad arguments");
        *pos = m->host_pos[slot];
    });
}

int fm_llm_teacher_step(fm_llm* m, int slot, const int32_t* x, int S, int pos0, const int32_t* next_col,
                        float* slow_logits, float* hidden, float* fast_logits) {
    return fm_guard([&] {
        FMCHECK(m && x && S >= 1, "bad arguments");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        FMCHECK(slot >= 0 && slot < m->max_slots, "bad slot");
        FMCHECK(pos0 + S <= m->c.max_seq_len, "beyond max_seq_len");
        check_tokens(m, x, S);
        if (next_col)
            for (int q = 1; q < m->C1; ++q)
                FMCHECK(next_col[q] >= 0 && next_col[q] < m->cb, "next_col codebook token out of range");
        if (pos0 == 0) reset_slot(m, slot, nullptr);
        const fm_model_config& c = m->c;
        const int32_t one = slot;
        HIPCHK(hipMemcpyAsync(m->frame_slot, &one, 4, hipMemcpyHostToDevice, m->stream));
        m->uploaded_slots.clear();
        std::vector<float> lg(m->Nhead);
        teacher_frame(m, slot, x, S, pos0, next_col, lg.data(), hidden, fast_logits);
        HIPCHK(hipStreamSynchronize(m->stream));
        m->prof.collect();
        m->host_pos[slot] = pos0 + S;
        if (slow_logits) {
            for (int i = 0; i < c.vocab_size; ++i) slow_logits[i] = -INFINITY;
            for (int i = 0; i < m->nsem; ++i) slow_logits[c.semantic_begin_id + i] = lg[i];
            slow_logits[c.im_end_id] = lg[m->nsem];
        }
    });
}

int64_t fm_llm_frame_bytes(fm_llm* m, int n, int pos) {
    if (!m) return -1;
    const fm_model_config& c = m->c;
    const int64_t E = (int64_t)m->esz;
    // weight-only int8: one byte per linear weight plus one T scale per output row; int4 (streamed
    // form): half a byte per weight plus one (scale, zero) word per row and 128-k unit
    const bool q4 = m->quant == FM_QUANT_INT4 && m->q4_gs % 128 == 0;
    auto lin = [&](int64_t N, int64_t K) -> int64_t {
        if (q4 && K % 128 == 0) return N * K / 2 + N * (K / 128) * 4;
        if (m->quant == FM_QUANT_INT8) return N * K + N * E;
        return N * K * E;
    };
    auto stack_bytes = [&](const StackDims& d) {
        int64_t per = lin(d.nqkv(), d.dim) + lin(d.dim, d.nq()) + lin(2LL * d.inter, d.dim) + lin(d.dim, d.inter) +
                      2LL * d.dim * E;
        if (d.qk_norm) per += 2LL * d.hd * E;
        return per * d.n_layer;
    };
    int64_t b = stack_bytes(m->sd) + (c.tie_word_embeddings ? (int64_t)m->Nhead * c.dim * E : lin(m->Nhead, c.dim)) +
                (int64_t)c.dim * E;
    b += (int64_t)m->C * stack_bytes(m->fdm) + (int64_t)(m->C - 1) * (lin(m->cb, c.fast_dim) + (int64_t)c.fast_dim * E);
    if (m->fproj_w) b += lin(c.fast_dim, c.dim);
    // per-stream: KV reads (+ the row written), embeddings
    int64_t per_stream = 2LL * m->sd.n_layer * m->sd.nkv * m->sd.hd * E * (pos + 1);
    for (int cc = 0; cc < m->C; ++cc) per_stream += 2LL * m->fdm.n_layer * m->fdm.nkv * m->fdm.hd * E * (cc + 1);
    per_stream += (int64_t)(m->C + 1) * c.dim * E + (int64_t)(m->C - 1) * c.fast_dim * E;
    return b + per_stream * n;
}

int fm_llm_use_graph(fm_llm* m, int enable) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        m->use_graph = enable != 0;
        // captured frames are dropped so that the next ones pick up any fm_tune change
        for (auto& g : m->graphs) (void)hipGraphExecDestroy(g.second);
        m->graphs.clear();
    });
}

int fm_llm_close(fm_llm* m) {
    return fm_guard([&] { delete m; });
}

}  // extern "C"
