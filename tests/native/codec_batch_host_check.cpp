// Stand-alone host check of the batched streamed decode's host arithmetic (csrc/fm_codec_batch.h):
// the gap, the capacity rule, the argument checks, the staged codes and the descriptor table, over the
// shapes the GPU tests use (tests/test_gpu_codec_batch.py), the rejected ones included.  No HIP, no
// Python: build with the host compiler and -fsanitize=address,undefined (make -C fish-speech_amd
// batch-host-check) and run; exit status 0 and "ok" mean every check held and no sanitizer fired.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "fm_codec_batch.h"

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++failures;                                               \
        }                                                             \
    } while (0)

// the shipped decoder's conv sites: two depthwise convs, conv0, then per stage the transposed conv
// and the three k7 units (dilations 1, 3, 9), then the output conv
static std::vector<CodecSite> shipped_sites() {
    std::vector<CodecSite> s = {{6, 2}, {6, 4}, {6, 4}};
    const int rates[4] = {8, 8, 4, 2}, dl[3] = {1, 3, 9};
    int L = 4;
    for (int b = 0; b < 4; ++b) {
        s.push_back({1, L});
        L *= rates[b];
        for (int r = 0; r < 3; ++r) s.push_back({6 * dl[r], L});
    }
    s.push_back({6, L});
    return s;
}

struct Ctxs {
    std::map<int, int> pos;
    int operator()(int sid) const {
        auto it = pos.find(sid);
        return it == pos.end() ? -1 : it->second;
    }
};

static const int NQ1 = 10, MAXF = 320, STREAM_MAX = 1 << 15, W1 = 127, NSITES = 24;

// one valid batch, end to end: check, codes, table -- every byte of the results is read back
static void run_batch(const std::vector<int32_t>& sids, const std::vector<int32_t>& T, const Ctxs& cx, int gap) {
    const int n = (int)sids.size();
    int64_t tot = 0;
    for (int t : T) tot += t;
    std::vector<int32_t> codes((size_t)tot * NQ1);
    for (size_t i = 0; i < codes.size(); ++i) codes[i] = (int32_t)(i % 1000) + 1;
    std::vector<float> pcm((size_t)tot * 2048);
    const char* bad = codec_batch_check(n, sids.data(), codes.data(), T.data(), pcm.data(), NQ1, gap, MAXF, STREAM_MAX, cx);
    EXPECT(bad == nullptr);
    if (bad) return;
    std::vector<int32_t> staged;
    codec_batch_codes(staged, n, T.data(), codes.data(), NQ1, gap);
    const int span = (int)codec_batch_span(n, T.data(), gap);
    EXPECT((int)staged.size() == NQ1 * span);
    // every segment's rows land at its offset, the gaps hold code 0
    size_t src = 0;
    int off = 0;
    for (int i = 0; i < n; ++i) {
        for (int q = 0; q < NQ1; ++q)
            for (int t = 0; t < T[i]; ++t) EXPECT(staged[(size_t)q * span + off + t] == codes[src + (size_t)q * T[i] + t]);
        if (i + 1 < n)
            for (int q = 0; q < NQ1; ++q)
                for (int t = 0; t < gap; ++t) EXPECT(staged[(size_t)q * span + off + T[i] + t] == 0);
        src += (size_t)NQ1 * T[i];
        off += T[i] + gap;
    }
    // the table: fake state pointers that name (segment, site)
    std::vector<std::vector<void*>> ptrs(n, std::vector<void*>(NSITES));
    std::vector<void* const*> bufs(n);
    std::vector<int32_t> pos(n);
    for (int i = 0; i < n; ++i) {
        for (int s = 0; s < NSITES; ++s) ptrs[i][s] = (void*)(uintptr_t)(0x1000 * (sids[i] + 1) + s);
        bufs[i] = ptrs[i].data();
        pos[i] = cx(sids[i]);
    }
    std::vector<uint8_t> blob;
    CodecBatchLayout lay;
    EXPECT(codec_batch_fill(blob, lay, n, T.data(), pos.data(), gap, W1, NSITES, bufs.data()) == span);
    EXPECT(blob.size() == lay.bytes && lay.st_off % 8 == 0);
    const CodecBatchLayout cap = codec_batch_layout(codec_batch_max_segments(MAXF, gap), MAXF, NSITES);
    EXPECT(lay.bytes <= cap.bytes);  // the device table allocated at finalize holds it
    off = 0;
    int covered = 0;
    for (int i = 0; i < n; ++i) {
        CodecSeg sg;
        memcpy(&sg, blob.data() + lay.seg_off + (size_t)i * sizeof(CodecSeg), sizeof sg);
        EXPECT(sg.off == off && sg.T == T[i] && sg.pos0 == pos[i] && sg.npre == (pos[i] < W1 ? pos[i] : W1));
        for (int s = 0; s < NSITES; ++s) {
            void* p;
            memcpy(&p, blob.data() + lay.st_off + ((size_t)i * NSITES + s) * sizeof(void*), sizeof p);
            EXPECT(p == ptrs[i][s]);
        }
        off += T[i] + gap;
    }
    for (int t = 0; t < span; ++t) {
        int32_t r;
        memcpy(&r, blob.data() + lay.rowseg_off + (size_t)t * 4, 4);
        EXPECT(r >= -1 && r < n);
        if (r >= 0) {
            CodecSeg sg;
            memcpy(&sg, blob.data() + lay.seg_off + (size_t)r * sizeof(CodecSeg), sizeof sg);
            EXPECT(t >= sg.off && t < sg.off + sg.T);
            ++covered;
        }
    }
    EXPECT(covered == tot);
}

int main() {
    const std::vector<CodecSite> sites = shipped_sites();
    EXPECT((int)sites.size() == 20);
    const int gap = codec_batch_gap(sites.data(), (int)sites.size());
    EXPECT(gap == 3);  // the first depthwise conv: 6 rows at 2 rows per frame
    for (const CodecSite& s : sites) EXPECT(gap * s.scale >= s.rows);
    bool tight = false;
    for (const CodecSite& s : sites) tight = tight || (gap - 1) * s.scale < s.rows;
    EXPECT(tight);  // and no smaller gap would do
    EXPECT(codec_batch_gap(nullptr, 0) == 0);
    EXPECT(codec_batch_max_segments(MAXF, gap) == 80 && codec_batch_max_segments(1, gap) == 1);

    Ctxs cx;
    cx.pos = {{0, 135}, {1, 0}, {2, 143}, {3, 5}, {4, STREAM_MAX - 10}};
    // the ragged schedules' steps, a batch of one, the handle's own stream beside late starters
    const int ragged[3][4] = {{1, 7, 22, 120}, {22, 22, 22, 84}, {3, 127, 19, 1}};
    for (int k = 0; k < 4; ++k) run_batch({1, 2, 3}, {ragged[0][k], ragged[1][k], ragged[2][k]}, cx, gap);
    run_batch({2}, {90}, cx, gap);
    run_batch({3, 0, 2, 1}, {5, 15, 15, 7}, cx, gap);
    run_batch({4}, {10}, cx, gap);                          // ends exactly at the RoPE table's last position
    run_batch({1, 2, 3}, {10, 10, MAXF - 2 * gap - 20}, cx, gap);  // exactly at capacity
    {
        std::vector<int32_t> ids, T;  // as many one-frame segments as max_frames holds
        Ctxs many;
        for (int i = 0; i < codec_batch_max_segments(MAXF, gap); ++i) {
            ids.push_back(i);
            T.push_back(1);
            many.pos[i] = i;
        }
        run_batch(ids, T, many, gap);
    }

    // the refused ones: nothing is read past what the checks before allow
    std::vector<int32_t> codes((size_t)NQ1 * 400, 1);
    std::vector<float> pcm(16);
    auto check = [&](std::vector<int32_t> sids, std::vector<int32_t> T, const int32_t* c) {
        return codec_batch_check((int)sids.size(), sids.data(), c, T.data(), pcm.data(), NQ1, gap, MAXF, STREAM_MAX, cx);
    };
    EXPECT(check({1, 1}, {10, 10}, codes.data()) != nullptr);                           // duplicate id
    EXPECT(check({1, 99}, {10, 10}, codes.data()) != nullptr);                          // unknown id
    EXPECT(check({1, 2}, {10, 0}, codes.data()) != nullptr);                            // T = 0
    EXPECT(check({1, 2}, {10, -5}, codes.data()) != nullptr);                           // T < 0
    EXPECT(check({1, 2, 3}, {10, 10, MAXF - 2 * gap - 20 + 1}, codes.data()) != nullptr);  // one frame over
    EXPECT(check({1, 2}, {0x7fffffff, 0x7fffffff}, codes.data()) != nullptr);           // the sum does not wrap
    EXPECT(check({4}, {11}, codes.data()) != nullptr);                                  // past the RoPE table
    EXPECT(check({}, {}, codes.data()) != nullptr);                                     // n = 0
    EXPECT(codec_batch_check(2, nullptr, codes.data(), nullptr, pcm.data(), NQ1, gap, MAXF, STREAM_MAX, cx) != nullptr);
    {
        std::vector<int32_t> ids(81), T(81, 1);  // more segments than max_frames holds
        Ctxs many;
        for (int i = 0; i < 81; ++i) many.pos[ids[i] = i] = 0;
        EXPECT(codec_batch_check(81, ids.data(), codes.data(), T.data(), pcm.data(), NQ1, gap, MAXF, STREAM_MAX, many) != nullptr);
    }
    {
        std::vector<int32_t> neg((size_t)NQ1 * 20, 3);  // exactly the batch's codes, the last one negative
        neg.back() = -1;
        EXPECT(check({1, 2}, {10, 10}, neg.data()) != nullptr);
        neg.back() = 0;
        EXPECT(check({1, 2}, {10, 10}, neg.data()) == nullptr);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
