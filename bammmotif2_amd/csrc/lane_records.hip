// The builder of the mixed-row kernel's lane records (lane_records.h): one wavefront per launch slot of a bucket reads the
// packed words, the length and the sequence record exactly as k_em_mix used to in every pass, and stores what the lanes
// derived from them.  Runs once per handle and bucket, from plan_launches, on the handle's stream.
#include <algorithm>

#include "lane_records.h"

namespace bamm {
namespace {

constexpr uint32_t kRecThreads = 256u, kRecWaves = kRecThreads / 64u;

template <int M>
__global__ void __launch_bounds__(kRecThreads) k_mix_records(SeqView sv, const uint4* xrec, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c, int frame,
                                                             uint2* out) {
    const int lane = threadIdx.x & 63;
    const uint32_t total_waves = gridDim.x * kRecWaves;
    for (uint32_t t = blockIdx.x * kRecWaves + (threadIdx.x >> 6); t < sv.count; t += total_waves) {
        const uint32_t seq = pick_sequence(sv, t);
        out[(size_t)t * 64u + (uint32_t)lane] =
            mix_lane_record<M>(sv.words + sv.word_off[seq], sv.len[seq], xrec[seq], lane, W, T, B, n1c, frame);
    }
}

template <int M>
int launch_records(const SeqView& sv, const uint4* xrec, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c, int frame, uint2* out, uint32_t blocks,
                   hipStream_t st) {
    return launch_kernel(&k_mix_records<M>, blocks, kRecThreads, 0, st, sv, xrec, W, T, B, n1c, frame, out);
}

}  // namespace

int launch_mix_records(int mclass, const SeqView& sv, const uint4* xrec, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c, int frame, uint2* out,
                       uint32_t num_cus, hipStream_t st) {
    if (sv.count == 0u && num_cus != kPrimeOnly) return BAMM_OK;
    const uint32_t blocks = num_cus == kPrimeOnly ? kPrimeOnly
                                                  : std::min((sv.count + kRecWaves - 1u) / kRecWaves, std::max(1u, num_cus) * 8u);
    int rc = BAMM_ERR_UNSUPPORTED;
    switch (mclass) {                                        // the length classes k_em_mix is built for (launch_mix)
        case 3: rc = launch_records<4>(sv, xrec, W, T, B, n1c, frame, out, blocks, st); break;
        case 4: rc = launch_records<5>(sv, xrec, W, T, B, n1c, frame, out, blocks, st); break;
        case 5: rc = launch_records<6>(sv, xrec, W, T, B, n1c, frame, out, blocks, st); break;
        case 6: rc = launch_records<7>(sv, xrec, W, T, B, n1c, frame, out, blocks, st); break;
        case 7: rc = launch_records<8>(sv, xrec, W, T, B, n1c, frame, out, blocks, st); break;
        case 8: rc = launch_records<10>(sv, xrec, W, T, B, n1c, frame, out, blocks, st); break;
        default: set_error("no mixed-row kernel for M class %d", mclass);
    }
    if (rc) return rc;
    if (blocks != kPrimeOnly) BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm

// the mixed rows' layout for (W, M) at K = 2: out[4] = T, B, A, resident columns of the accumulating pass
extern "C" int bamm_mix_layout(uint32_t W, int M, uint32_t* out) {
    bamm::GrpGeom g{};
    if (!out) { bamm::set_error("bamm_mix_layout: bad argument"); return BAMM_ERR_ARG; }
    if (M < 1 || !bamm::mix_geometry(2u, W, M, bamm::grp_max_threads(M) / 64u, true, &g)) {
        bamm::set_error("no mixed rows for W=%u at %d positions per lane", W, M);
        return BAMM_ERR_UNSUPPORTED;
    }
    out[0] = g.T; out[1] = g.mixB; out[2] = g.mixA; out[3] = bamm::mix_resident_cols(g);
    return BAMM_OK;
}

// the fix-lane word of one lane record on the host (lane_records.h: mix_fix_word, the function k_mix_records runs):
// out[0] = word y, out[1] = the lane is a fix lane of the sequence.  No device needed.
extern "C" int bamm_mix_fix_word(uint32_t lane, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c, uint32_t L, uint32_t xw, uint32_t xfields,
                                 uint32_t sE, uint32_t* out) {
    if (!out || lane >= 64u || !T || B > T || W > L) { bamm::set_error("bamm_mix_fix_word: bad argument"); return BAMM_ERR_ARG; }
    bool fix = false;
    out[0] = bamm::mix_fix_word(lane, W, T, B, n1c, L, xw, xfields, sE, &fix);
    out[1] = fix ? 1u : 0u;
    return BAMM_OK;
}
