// fm_codec_batch.h -- host arithmetic of the batched streamed decode (fm_codec_stream_decode_batch):
// the gap between segments, the argument checks, the staged codes and the device descriptor table.
// Plain C++ with no HIP in it, so the same code compiles into the library and into the stand-alone
// host check (tests/native/codec_batch_host_check.cpp, built with the address and UB sanitizers).
//
// Layout of a batched pass.  Segment i (the next T[i] frames of one stream context) sits at frame
// offset off[i] of the work buffers, off[0] = 0 and off[i + 1] = off[i] + T[i] + gap, so the pass
// spans sum(T) + gap * (n - 1) frames.  At a level with `scale` rows per frame a causal reader that
// carries `rows` rows finds segment i's carried rows in the rows right in front of the segment:
// the buffer prefix for segment 0, the gap for the others -- hence gap * scale >= rows at every site.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

// one causal conv site: the rows it carries and the rows per code frame of the buffer it reads
struct CodecSite {
    int rows, scale;
};

// smallest frame count whose scaled size covers the carried rows of every site
inline int codec_batch_gap(const CodecSite* sites, int nsites) {
    int gap = 0;
    for (int i = 0; i < nsites; ++i) {
        const int g = (sites[i].rows + sites[i].scale - 1) / sites[i].scale;
        if (g > gap) gap = g;
    }
    return gap;
}

// frames a batch of n segments spans (64-bit: T comes from the caller)
inline int64_t codec_batch_span(int n, const int32_t* T, int gap) {
    int64_t s = (int64_t)gap * (n - 1);
    for (int i = 0; i < n; ++i) s += T[i];
    return s;
}

// most segments a pass over max_frames frames can hold (every segment is at least one frame)
inline int codec_batch_max_segments(int max_frames, int gap) { return (max_frames + gap) / (1 + gap); }

// The argument checks of fm_codec_stream_decode_batch, all of them before the first launch.
// pos_of(sid): the context's position, or -1 when no such context is open.  Null: the batch is
// valid; else what is wrong with it (nothing has been touched).
template <typename PosOf>
const char* codec_batch_check(int n, const int32_t* sids, const int32_t* codes, const int32_t* T, const float* pcm,
                              int nq1, int gap, int max_frames, int stream_max, PosOf&& pos_of) {
    if (n < 1) return "batch: at least one segment";
    if (!sids || !codes || !T || !pcm) return "null argument";
    if (n > codec_batch_max_segments(max_frames, gap)) return "batch: more segments than max_frames holds";
    for (int i = 0; i < n; ++i) {
        if (T[i] < 1) return "batch: every segment needs T >= 1";
        for (int j = 0; j < i; ++j)
            if (sids[j] == sids[i]) return "batch: a stream id appears twice";
        const int pos = pos_of((int)sids[i]);
        if (pos < 0) return "batch: unknown codec stream id";
        if ((int64_t)pos + T[i] > stream_max) return "stream longer than the RoPE table: reset it";
    }
    const int64_t span = codec_batch_span(n, T, gap);
    if (span > max_frames) return "batch: sum(T) + gap * (n - 1) exceeds max_frames";
    const int64_t total = (span - (int64_t)gap * (n - 1)) * nq1;
    for (int64_t i = 0; i < total; ++i)
        if (codes[i] < 0) return "negative code";
    return nullptr;
}

// per-segment record of the device table (16 bytes)
struct CodecSeg {
    int32_t off;   // first frame of the segment in the pass
    int32_t T;     // its frames
    int32_t pos0;  // the stream's position at its first frame (RoPE)
    int32_t npre;  // carried key / value rows in use: min(pos0, window - 1)
};

// The table as one blob, uploaded once per call: CodecSeg seg[n], then int32 rowseg[span] (the
// segment a frame belongs to, -1 in a gap), then (8-byte aligned) void* st[n][nsites], the state
// buffers of every segment's stream context in site order.
struct CodecBatchLayout {
    size_t seg_off, rowseg_off, st_off, bytes;
};
inline CodecBatchLayout codec_batch_layout(int n, int span, int nsites) {
    CodecBatchLayout l;
    l.seg_off = 0;
    l.rowseg_off = (size_t)n * sizeof(CodecSeg);
    l.st_off = (l.rowseg_off + (size_t)span * 4 + 7) / 8 * 8;
    l.bytes = l.st_off + (size_t)n * nsites * sizeof(void*);
    return l;
}
// bufs[i]: the nsites state pointers of segment i's context.  Returns the span.
inline int codec_batch_fill(std::vector<uint8_t>& blob, CodecBatchLayout& l, int n, const int32_t* T, const int32_t* pos,
                            int gap, int w1, int nsites, void* const* const* bufs) {
    const int span = (int)codec_batch_span(n, T, gap);
    l = codec_batch_layout(n, span, nsites);
    blob.assign(l.bytes, 0);
    std::vector<int32_t> rowseg((size_t)span, -1);
    int off = 0;
    for (int i = 0; i < n; ++i) {
        CodecSeg s;
        s.off = off;
        s.T = T[i];
        s.pos0 = pos[i];
        s.npre = pos[i] < w1 ? pos[i] : w1;
        memcpy(blob.data() + l.seg_off + (size_t)i * sizeof(CodecSeg), &s, sizeof(CodecSeg));
        for (int t = 0; t < T[i]; ++t) rowseg[(size_t)off + t] = i;
        if (nsites) memcpy(blob.data() + l.st_off + (size_t)i * nsites * sizeof(void*), bufs[i], (size_t)nsites * sizeof(void*));
        off += T[i] + gap;
    }
    if (span) memcpy(blob.data() + l.rowseg_off, rowseg.data(), (size_t)span * 4);
    return span;
}

// the caller's codes (segments back to back, each (nq1, T[i]) row-major) as one (nq1, span)
// row-major array, zeros in the gaps (code 0 is valid in every codebook: the gap rows stay finite)
inline void codec_batch_codes(std::vector<int32_t>& out, int n, const int32_t* T, const int32_t* codes, int nq1, int gap) {
    const int span = (int)codec_batch_span(n, T, gap);
    out.assign((size_t)nq1 * span, 0);
    size_t src = 0;
    int off = 0;
    for (int i = 0; i < n; ++i) {
        for (int q = 0; q < nq1; ++q) memcpy(out.data() + (size_t)q * span + off, codes + src + (size_t)q * T[i], (size_t)T[i] * 4);
        src += (size_t)nq1 * T[i];
        off += T[i] + gap;
    }
}
