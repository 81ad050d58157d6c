// fm_llm_dev.cpp -- developer hooks of libfishmi: tuning knobs, timestamps, profiler, kernel bench,
// teacher forcing taps, buffer reads, the host-fault stack trace.
#include <dlfcn.h>
#include <execinfo.h>
#include <math.h>
#include <signal.h>

#include <algorithm>

#include "fm_llm_model.h"

// developer: FISHMI_SEGV_TRACE=1 prints the native stack (module + offset per frame) of a host
// fault before the default action (the rocprofv3 fault investigation)
namespace {
void segv_trace(int sig, siginfo_t* si, void*) {
    void* fr[64];
    const int n = backtrace(fr, 64);
    fprintf(stderr, "fishmi: signal %d at address %p, %d frames\n", sig, si ? si->si_addr : nullptr, n);
    for (int i = 0; i < n; ++i) {
        Dl_info d{};
        if (dladdr(fr[i], &d) && d.dli_fname)
            fprintf(stderr, "  #%d %s +0x%lx (%s)\n", i, d.dli_fname,
                    (unsigned long)((const char*)fr[i] - (const char*)d.dli_fbase), d.dli_sname ? d.dli_sname : "?");
        else
            fprintf(stderr, "  #%d %p\n", i, fr[i]);
    }
    fflush(stderr);
    signal(sig, SIG_DFL);
    raise(sig);
}
struct SegvTraceInstaller {
    SegvTraceInstaller() {
        const char* e = getenv("FISHMI_SEGV_TRACE");
        if (!e || e[0] != '1') return;
        struct sigaction sa {};
        sa.sa_sigaction = segv_trace;
        sa.sa_flags = SA_SIGINFO;
        sigaction(SIGSEGV, &sa, nullptr);
        sigaction(SIGBUS, &sa, nullptr);
    }
} g_segv_trace;
}  // namespace

FmTuning& fm_tuning() {
    static FmTuning t;
    return t;
}

// the knobs of fm_tune_table.h, by name
namespace {
struct Knob {
    const char* name;
    int FmTuning::*field;
    int rule, a, b;
};
const Knob KNOBS[] = {
#define FM_KNOB(name, def, ...) {#name, &FmTuning::name, __VA_ARGS__},
#include "fm_tune_table.h"
#undef FM_KNOB
};
static_assert(KSB_MAX == 8 && GEMV_CHAIN_MAX == 4, "fm_tune_table.h: the ranges of fin_ksb / chain_max");
const Knob& knob_of(const std::string& key) {
    for (const Knob& k : KNOBS)
        if (key == k.name) return k;
    throw FmError{FM_ERR_ARG, "unknown tuning key: " + key};
}
bool knob_accepts(const Knob& k, int v) {
    switch (k.rule) {
        case FM_RULE_SET: return v >= 0 && v <= 30 && ((k.a >> v) & 1);
        case FM_RULE_RANGE: return v >= k.a && v <= k.b;
        case FM_RULE_MULT16: return (k.a && v == 0) || (v >= 16 && v % 16 == 0);
        default: return true;  // FM_RULE_BOOL, FM_RULE_ANY
    }
}
}  // namespace

extern "C" {

int fm_llm_profile(fm_llm* m, int enable) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        m->prof.on = enable != 0;
        if (enable) m->prof.acc.clear();
    });
}

int fm_llm_profile_read(fm_llm* m, const char* cls, double* ms, int64_t* launches, int64_t* bytes) {
    return fm_guard([&] {
        FMCHECK(m && cls, "null argument");
        auto it = m->prof.acc.find(cls);
        Profiler::Acc a = it == m->prof.acc.end() ? Profiler::Acc{} : it->second;
        if (ms) *ms = a.ms;
        if (launches) *launches = a.n;
        if (bytes) *bytes = a.bytes;
    });
}

int fm_tune(const char* key, int value) {
    return fm_guard([&] {
        FMCHECK(key, "null key");
        FmTuning& t = fm_tuning();
        const std::string k = key;
        if (k == "debug_ts") {  // (re)arm the per-block timestamp buffer; 0 frees it (no kernel choice changes: no epoch)
            if (t.dbg) HIPCHK(hipFree(t.dbg));
            t.dbg = nullptr;
            if (value) {
                HIPCHK(hipMalloc(&t.dbg, (8 + 8 * (1 << 20)) * sizeof(unsigned long long)));
                HIPCHK(hipMemset(t.dbg, 0, 8 * sizeof(unsigned long long)));
            }
            return;
        }
        ++t.epoch;
        const Knob& kn = knob_of(k);
        FMCHECK(knob_accepts(kn, value), k + ": value " + std::to_string(value) + " is outside the knob's accepted values (fm_tune_table.h)");
        t.*kn.field = kn.rule == FM_RULE_BOOL ? value != 0 : value;
    });
}

int fm_tune_get(const char* key, int* value) {
    return fm_guard([&] {
        FMCHECK(key && value, "null argument");
        const FmTuning& t = fm_tuning();
        *value = std::string(key) == "debug_ts" ? t.dbg != nullptr : t.*knob_of(key).field;
    });
}

int fm_debug_ts_read(unsigned long long* out, int64_t max_records, int64_t* n_records) {
    return fm_guard([&] {
        FMCHECK(out && n_records, "null argument");
        const FmTuning& t = fm_tuning();
        FMCHECK(t.dbg, "debug_ts is not armed");
        HIPCHK(hipDeviceSynchronize());
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, t.dbg, sizeof n, hipMemcpyDeviceToHost));
        n = std::min<unsigned long long>(n, 1ull << 20);
        n = std::min<unsigned long long>(n, (unsigned long long)max_records);
        HIPCHK(hipMemcpy(out, t.dbg + 8, n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        *n_records = (int64_t)n;
    });
}

int fm_llm_kernel_bench(fm_llm* m, const char* cls, int reps, double* avg_us, int64_t* launches,
                        int64_t* bytes) {
    return fm_guard([&] {
        FMCHECK(m && cls && reps >= 1, "bad arguments");
        FMCHECK(m->finalized && !m->uploaded_slots.empty(), "decode a frame first");
        HIPCHK(hipSetDevice(m->device));
        const int n = (int)m->uploaded_slots.size();
        const bool was_on = m->prof.on;
        ensure_qkv0(m);
        // record the class's launches of one eager frame (the frame itself runs normally)
        m->prof.on = false;
        m->prof.rec.clear();
        m->prof.rec_bytes.clear();
        m->prof.rec_cls = cls;
        decode_frame_eager(m, n);
        m->prof.rec_cls.clear();
        m->prof.on = was_on;
        HIPCHK(hipStreamSynchronize(m->stream));
        for (int s : m->uploaded_slots) {  // that frame advanced the slots on the device
            m->host_pos[s]++;
            m->host_step[s]++;
        }
        std::vector<std::function<void()>> rec;
        rec.swap(m->prof.rec);
        FMCHECK(!rec.empty(), std::string("no launches of class ") + cls + " in a decode frame");
        int64_t b = 0;
        for (int64_t x : m->prof.rec_bytes) b += x;
        // replay them back to back as one graph, timed by two events on the compute stream
        hipGraph_t g;
        HIPCHK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
        for (auto& f : rec) f();
        HIPCHK(hipStreamEndCapture(m->stream, &g));
        hipGraphExec_t ge;
        HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        HIPCHK(hipGraphDestroy(g));
        hipEvent_t ea, eb;
        HIPCHK(hipEventCreate(&ea));
        HIPCHK(hipEventCreate(&eb));
        HIPCHK(hipGraphLaunch(ge, m->stream));
        HIPCHK(hipEventRecord(ea, m->stream));
        for (int i = 0; i < reps; ++i) HIPCHK(hipGraphLaunch(ge, m->stream));
        HIPCHK(hipEventRecord(eb, m->stream));
        HIPCHK(hipEventSynchronize(eb));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ea, eb));
        (void)hipEventDestroy(ea);
        (void)hipEventDestroy(eb);
        (void)hipGraphExecDestroy(ge);
        if (avg_us) *avg_us = (double)ms * 1e3 / ((double)reps * rec.size());
        if (launches) *launches = (int64_t)rec.size();
        if (bytes) *bytes = b;
    });
}

int fm_llm_force(fm_llm* m, int slot, const int32_t* col) {
    return fm_guard([&] {
        FMCHECK(m, "null handle");
        HIPCHK(hipSetDevice(m->device));
        finalize(m);
        FMCHECK(slot >= 0 && slot < m->max_slots, "bad slot");
        const int on = col != nullptr;
        if (on) {
            const fm_model_config& c = m->c;
            // any vocabulary id: the reference's bf16 multinomial draw can emit ids outside the
            // semantic support (torch.rand_like in bf16 yields 0 or 1, and argmax over an all-zero
            // or NaN row is id 0: inference.py:43-46), and teacher forcing replays its streams
            FMCHECK(col[0] >= 0 && col[0] < c.vocab_size, "forced token outside the vocabulary");
            for (int q = 1; q < m->C1; ++q)
                FMCHECK(col[q] >= 0 && col[q] < m->cb, "forced codebook token out of range");
            HIPCHK(hipMemcpyAsync(m->force_cols + (size_t)slot * m->C1, col, (size_t)m->C1 * 4,
                                  hipMemcpyHostToDevice, m->stream));
        }
        m->host_force[slot] = on;
        HIPCHK(hipMemcpyAsync(&m->sp[slot].force, &m->host_force[slot], sizeof(int), hipMemcpyHostToDevice,
                              m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    });
}

int fm_llm_read_logits(fm_llm* m, int slot, float* slow_logits, float* fast_logits) {
    return fm_guard([&] {
        FMCHECK(m && m->finalized, "null or unfinalized handle");
        FMCHECK(slot >= 0 && slot < m->max_slots, "bad slot");
        HIPCHK(hipSetDevice(m->device));
        const fm_model_config& c = m->c;
        std::vector<float> lg(m->Nhead);
        HIPCHK(hipMemcpyAsync(lg.data(), m->tap_slow + (size_t)slot * m->Nhead, (size_t)m->Nhead * 4,
                              hipMemcpyDeviceToHost, m->stream));
        if (fast_logits && m->C > 1)
            HIPCHK(hipMemcpyAsync(fast_logits, m->tap_fast + (size_t)slot * (m->C - 1) * m->cb,
                                  (size_t)(m->C - 1) * m->cb * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        if (slow_logits) {
            for (int i = 0; i < c.vocab_size; ++i) slow_logits[i] = -INFINITY;
            for (int i = 0; i < m->nsem; ++i) slow_logits[c.semantic_begin_id + i] = lg[i];
            slow_logits[c.im_end_id] = lg[m->nsem];
        }
    });
}

int fm_llm_debug_vec(fm_llm* m, const char* name, int index, float* out, int64_t n) {
    return fm_guard([&] {
        FMCHECK(m && m->finalized && name && out && n > 0, "bad arguments");
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipStreamSynchronize(m->stream));
        const std::string k = name;
        void* p = k == "qkv" ? m->qkv : k == "att" ? m->att : k == "fh" ? m->fh : k == "act" ? m->act
                : k == "fx" ? m->fx : k == "fx2" ? m->fx2 : k == "xl" ? m->xl : k == "xnl" ? m->xnl : nullptr;
        if (k == "kc" || k == "vc") {  // slot 0's slow-layer `index` cache: [nkv][S][hd]
            FMCHECK(index >= 0 && index < m->sd.n_layer, "layer out of range");
            FMCHECK(n <= (int64_t)m->layer_stride, "n past the layer's cache");
            p = (char*)(k == "kc" ? m->kc : m->vc) + (size_t)index * m->layer_stride * m->esz;
        }
        FMCHECK(p, "unknown buffer: " + k);
        if (m->esz == 4) {
            HIPCHK(hipMemcpy(out, p, (size_t)n * 4, hipMemcpyDeviceToHost));
        } else {
            std::vector<uint16_t> v((size_t)n);
            HIPCHK(hipMemcpy(v.data(), p, (size_t)n * 2, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n; ++i) {
                const uint32_t u = (uint32_t)v[(size_t)i] << 16;
                memcpy(out + i, &u, 4);
            }
        }
    });
}

}  // extern "C"
