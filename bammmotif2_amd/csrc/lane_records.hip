// The builder of the mixed-row kernel's lane records (lane_records.h): one wavefront per launch slot of a bucket reads the
// packed words, the length and the sequence record exactly as k_em_mix used to in every pass, and stores what the lanes
// derived from them.  Runs once per handle and bucket, from plan_launches, on the handle's stream.
#include <algorithm>

#include "lane_records.h"

namespace bamm {
namespace {

constexpr uint32_t kRecThreads = 256u, kRecWaves = kRecThreads / 64u;

template <int M>
__global__ void __launch_bounds__(kRecThreads) k_mix_records(SeqView sv, const uint4* xrec, uint32_t W, uint32_t T, uint32_t B, uint2* out) {
    const int lane = threadIdx.x & 63;
    const uint32_t total_waves = gridDim.x * kRecWaves;
    for (uint32_t t = blockIdx.x * kRecWaves + (threadIdx.x >> 6); t < sv.count; t += total_waves) {
        const RawSeqG<M> cur = fetch_seq_g<M>(sv, xrec, t, lane);
        out[(size_t)t * 64u + (uint32_t)lane] = mix_lane_record<M>(cur, lane, W, T, B);
    }
}

template <int M>
int launch_records(const SeqView& sv, const uint4* xrec, uint32_t W, uint32_t T, uint32_t B, uint2* out, uint32_t blocks, hipStream_t st) {
    return launch_kernel(&k_mix_records<M>, blocks, kRecThreads, 0, st, sv, xrec, W, T, B, out);
}

}  // namespace

int launch_mix_records(int mclass, const SeqView& sv, const uint4* xrec, uint32_t W, uint32_t T, uint32_t B, uint2* out,
                       uint32_t num_cus, hipStream_t st) {
    if (sv.count == 0u && num_cus != kPrimeOnly) return BAMM_OK;
    const uint32_t blocks = num_cus == kPrimeOnly ? kPrimeOnly
                                                  : std::min((sv.count + kRecWaves - 1u) / kRecWaves, std::max(1u, num_cus) * 8u);
    int rc = BAMM_ERR_UNSUPPORTED;
    switch (mclass) {                                        // the length classes k_em_mix is built for (launch_mix)
        case 3: rc = launch_records<4>(sv, xrec, W, T, B, out, blocks, st); break;
        case 4: rc = launch_records<5>(sv, xrec, W, T, B, out, blocks, st); break;
        case 5: rc = launch_records<6>(sv, xrec, W, T, B, out, blocks, st); break;
        case 6: rc = launch_records<7>(sv, xrec, W, T, B, out, blocks, st); break;
        case 7: rc = launch_records<8>(sv, xrec, W, T, B, out, blocks, st); break;
        case 8: rc = launch_records<10>(sv, xrec, W, T, B, out, blocks, st); break;
        default: set_error("no mixed-row kernel for M class %d", mclass);
    }
    if (rc) return rc;
    if (blocks != kPrimeOnly) BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm
