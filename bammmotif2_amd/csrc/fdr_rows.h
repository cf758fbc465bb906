// FDR::calculatePR's MOPS rows and FDR::calculatePvalues' p-value (FDR.cpp:156-196, :278-333): the expressions that
// turn the ranking walk's counts into numbers.  ONE body for the host path (host/fdr.cpp: fdr_statistics) and the device
// path (fdr.hip), so that the two cannot drift.  Only conversions, +, - and /: with IEEE division, fp32 denormals kept and
// no contraction (build.py: TU_FLAGS of fdr.hip) the device's bits are the host's.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BAMM_FDR_HD __host__ __device__ inline
#else
#define BAMM_FDR_HD inline
#endif

namespace bamm {

// negatives per positive as the reference counts them (sequences, not windows; FDR.cpp:152)
BAMM_FDR_HD float fdr_mfold(uint64_t posN, uint64_t negN) { return (float)negN / (float)posN; }

// after a step of the walk: ip positive and in negative scores taken so far (FDR.cpp:178-179)
BAMM_FDR_HD float fdr_fp(uint64_t in, float mFold) { return (float)in / mFold; }
BAMM_FDR_HD float fdr_tp(uint64_t ip, uint64_t in, float mFold) { return (float)ip - (float)in / mFold; }
// FDR.cpp:192-193
BAMM_FDR_HD float fdr_fdr(float tp, float fp) { return fp / (tp + fp); }
BAMM_FDR_HD float fdr_rec(float tp, float e_tp) { return tp / e_tp; }

// the peak (FDR.cpp:181-186), one step: idx_max is the LAST step whose tp equals the running maximum in front of it
struct FdrPeakStep {
    float e_tp;
    bool equal;
};
BAMM_FDR_HD FdrPeakStep fdr_peak_step(float e_tp, float tp) {
    FdrPeakStep s;
    s.equal = e_tp == tp;
    s.e_tp = e_tp < tp ? tp : e_tp;
    return s;
}

// FDR.cpp:296-304 / :318-326: low / up = lower and upper bound of a positive score in the ascending negatives
BAMM_FDR_HD float fdr_pvalue(uint64_t low, uint64_t up, uint64_t n_neg) {
    float p = 1.0f - (float)(up + low) / (2.0f * (float)n_neg);
    if (p < 1.e-6) p = 1.e-6;                                // compared in double, as the reference's literal makes it
    if (p > 1.0f) p = 1.0f;
    return p;
}

}  // namespace bamm
