// ScoreSeqSet::calcPvalues (seq_scoring/ScoreSeqSet.cpp:70-126), the part that runs once per window and the scalars in
// front of it.  Host code, shared by the host path (host/fdr.cpp: mops_pvalues) and the device path (occurrences.cpp:
// bamm_occurrences, which hands it the candidates the rank kernel left): ONE body, so that the two cannot drift.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace bamm {

constexpr float kOccEps = 1.0e-5;                          // ScoreSeqSet.cpp:76

// nTop, S_ntop and lambda from the LOWEST nTop + 1 negative scores (the reference sorts ascending, :81-93).
struct OccScalars {
    size_t negN = 0, nTop = 0;
    float S_ntop = 0.f, lambda = 0.f;
};
inline size_t occ_ntop(size_t negN) { return std::min(100, (int)negN / 10); }
inline OccScalars occ_scalars(const float* lowest, size_t negN) {   // lowest[0 .. nTop] of the ascending negatives
    OccScalars s;
    s.negN = negN;
    s.nTop = occ_ntop(negN);
    s.S_ntop = lowest[s.nTop];
    float lambda = 0.f;
    for (size_t n = 0; n < s.nTop; n++) lambda += (lowest[n] - s.S_ntop);
    s.lambda = lambda / (float)s.nTop;
    return s;
}

// the branch that reads the two negative scores next to Sl (:118-124); the others never look at them
inline bool occ_uses_neighbours(size_t FPl, const OccScalars& s) {
    return FPl != s.negN && !(FPl < 10 && fabs(s.lambda) > kOccEps);
}

// p-value of one window (:97-125).  FPl = negatives scoring above Sl; SlHigher = neg[negN - FPl - 1], SlLower =
// neg[negN - FPl] of the ascending negatives (read only where occ_uses_neighbours()).
inline float occ_window_pvalue(float Sl, size_t FPl, float SlHigher, float SlLower, const OccScalars& s) {
    const float eps = kOccEps;
    const size_t negN = s.negN, nTop = s.nTop;
    float p;
    if (FPl == negN) {
        p = 1.f;
    } else if (FPl < 10 && fabs(s.lambda) > eps) {
        p = float(nTop) / (float)negN * expf(-(Sl - s.S_ntop) / s.lambda);
    } else {
        p = ((float)FPl + (SlHigher - Sl + eps) / (SlHigher - SlLower + eps)) / (float)negN;
    }
    return p;
}

}  // namespace bamm
