// The two rules of SeqGenerator's negative sampler that the host sampler (host/fdr.cpp, host/neg_sampler.h) and the host side
// of the device sampler (csrc/negs.cpp) must share to the letter: which negatives are kept and where they go, and the set's
// conditionals and bars from its k-mer totals.  The tests compare the two samplers' negatives base for base.  No HIP here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bamm {

// keep_stride > 1: only the negatives idx = 0, stride, 2 stride, ... with idx + stride <= total are generated (the others still
// consume their draws): --FDR scores nothing else (FDR.cpp:58-60).  The third place that states this rule is k_neg_sample's `mine` (negs.hip).
inline bool neg_kept(uint64_t idx, uint64_t keep_stride, uint64_t total_neg) {
    return keep_stride <= 1 || (idx % keep_stride == 0 && idx + keep_stride <= total_neg);
}

// Every negative consumes exactly L draws of the one rand() stream, in order: positive i's negatives are i m_fold + f,
// its draws start at draw0[i], and its kept negatives are first_kept[i] .. first_kept[i + 1] - 1 of the output.
struct NegLayout {
    uint64_t m_fold, keep_stride, total_neg;
    std::vector<uint64_t> draw0, first_kept;                 // [n + 1]
    NegLayout() : m_fold(0), keep_stride(0), total_neg(0), draw0(1, 0), first_kept(1, 0) {}   // of no positives
    bool kept(uint64_t i, uint64_t f) const { return neg_kept(i * m_fold + f, keep_stride, total_neg); }
    uint64_t n_kept(uint64_t i) const { return first_kept[i + 1] - first_kept[i]; }
    uint64_t n_neg() const { return first_kept.back(); }

    template <class LenOf>                                   // len_of(i): positions of positive i
    NegLayout(uint64_t n, LenOf&& len_of, uint64_t m_fold_, uint64_t keep_stride_)
        : m_fold(m_fold_), keep_stride(keep_stride_), total_neg(n * m_fold_), draw0(n + 1, 0), first_kept(n + 1, 0) {
        for (uint64_t i = 0; i < n; i++) {
            uint64_t nk = 0;
            if (keep_stride <= 1) nk = m_fold;
            else for (uint64_t f = 0; f < m_fold; f++) nk += kept(i, f);
            draw0[i + 1] = draw0[i] + (uint64_t)len_of(i) * m_fold;
            first_kept[i + 1] = first_kept[i] + nk;
        }
    }
};

// The set's conditionals v and their cumulative bars, orders 0..s, from the (k+1)-mer totals `cnt` and the pseudo-counts A
// (SeqGenerator.cpp:86-110; the fp32 expression order is the reference's).  Count: size_t on the host, unsigned long long
// where the totals come from the device.  off(k): first cell of order k in the flat [k][y] tables -- each library's own
// (common.h: bg_offset, host_util.h: bgoff; neither header can be included from the other library).
template <class Count, class Off>
void neg_set_tables(const Count* cnt, uint32_t s, const float* A, float* v, float* bar, Off&& off) {
    Count norm = 0;
    for (size_t y = 0; y < 4; y++) norm += cnt[y];
    float sum = 0.0f;
    for (size_t y = 0; y < 4; y++) {
        v[y] = ((float)cnt[y] + A[0] * 0.25f) / ((float)norm + A[0]);
        sum += v[y];
        bar[y] = sum;
    }
    for (uint32_t k = 1; k <= s; k++) {
        const size_t ok = off(k), ok1 = off(k - 1), Yk = size_t(1) << (2 * k);
        sum = 0.f;
        for (size_t y = 0; y < 4 * Yk; y++) {
            const size_t yk = y / 4, y2 = y % Yk;
            v[ok + y] = ((float)cnt[ok + y] + A[k] * v[ok1 + y2]) / ((float)cnt[ok1 + yk] + A[k]);
            if (y % 4 == 0) sum = 0.f;
            sum += v[ok + y];
            bar[ok + y] = sum;
        }
    }
}

}  // namespace bamm
