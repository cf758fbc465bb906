// The device half of ScoreSeqSet::calcPvalues (seq_scoring/ScoreSeqSet.cpp:70-126) behind the scorer: the negative
// windows' scores sorted ascending where k_score left them (keys-only radix sort), and one kernel over the positive
// windows' scores that ranks each against the sorted negatives and appends the windows the host has to look at -- a
// few thousand of some 10^8 -- to a list.  Nothing window-sized leaves the device (occurrences.cpp: bamm_occurrences).
//
// Sort: least-significant-digit first, four passes of 8 bits over order-preserving unsigned keys.  A pass is a
// per-block digit histogram (LDS), one scan of the [digit][block] table, and a STABLE scatter: a block walks its
// contiguous share in order, 256 keys at a time; a key's slot is the block's running offset of its digit, plus the
// keys of that digit in the waves in front of its own, plus its rank among the equal digits of its wave (ballots).
//
// Floating point: the rank kernel evaluates the reference's interpolation branch with the host's operations.  The
// build compiles every unit with -ffp-contract=off (no fused multiply-add in place of a separate add) and this one
// with -fhip-fp32-correctly-rounded-divide-sqrt spelled out (the IEEE division sequence v_div_scale / v_div_fmas /
// v_div_fixup, never a bare v_rcp_f32 times the numerator) and -fno-gpu-flush-denormals-to-zero (fp32 denormals kept,
// as on the host).

#include <algorithm>

#include "common.h"
#include "sort_key.h"

namespace bamm {
namespace {

constexpr uint32_t kSortThreads = 256, kSortWaves = kSortThreads / 64;

// the keys are sort_key.h's; pass 0 reads the scores themselves, pass 3 writes floats back into the array it started from
template <int PASS>
__device__ __forceinline__ uint32_t load_key(const uint32_t* src, uint64_t i) {
    return PASS == 0 ? key_of(__uint_as_float(src[i])) : src[i];
}

// the keys of block b: [begin, end), a multiple of 256 per block
__device__ __forceinline__ void block_range(uint32_t n, uint32_t per_block, uint64_t* begin, uint64_t* end) {
    *begin = (uint64_t)blockIdx.x * per_block;
    *end = *begin + per_block < (uint64_t)n ? *begin + per_block : (uint64_t)n;
    if (*begin > *end) *begin = *end;
}

template <int PASS>
__global__ __launch_bounds__(kSortThreads) void k_occ_hist(const uint32_t* __restrict__ src, uint32_t n, uint32_t per_block,
                                                           uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    uint64_t begin, end;
    block_range(n, per_block, &begin, &end);
    for (uint64_t i = begin + threadIdx.x; i < end; i += kSortThreads)
        atomicAdd(&h[(load_key<PASS>(src, i) >> (8 * PASS)) & 255u], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of the [digit][block] table in place: one block, every thread a contiguous run
__global__ __launch_bounds__(1024) void k_occ_scan(uint32_t* __restrict__ hist, uint32_t total) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (total + 1023u) / 1024u;
    const uint32_t b = min(threadIdx.x * per, total), e = min(b + per, total);
    uint32_t sum = 0u;
    for (uint32_t i = b; i < e; i++) sum += hist[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t i = b; i < e; i++) {
        const uint32_t c = hist[i];
        hist[i] = run;
        run += c;
    }
}

template <int PASS>
__global__ __launch_bounds__(kSortThreads) void k_occ_scatter(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                              uint32_t n, uint32_t per_block, const uint32_t* __restrict__ hist) {
    __shared__ uint32_t base[256];                           // where the block's next key of each digit goes
    __shared__ uint32_t cnt[kSortWaves][256], off[kSortWaves][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    base[tid] = hist[(size_t)tid * gridDim.x + blockIdx.x];
    for (uint32_t w = 0; w < kSortWaves; w++) cnt[w][tid] = 0u;
    __syncthreads();
    uint64_t begin, end;
    block_range(n, per_block, &begin, &end);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint64_t at = begin; at < end; at += kSortThreads) {     // block-uniform trip count
        const uint64_t i = at + tid;
        const bool valid = i < end;
        const uint32_t key = valid ? load_key<PASS>(src, i) : 0u;
        const uint32_t digit = (key >> (8 * PASS)) & 255u;
        unsigned long long peers = __ballot(valid);              // lanes of this wave with the same digit
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (digit >> bit) & 1u;
            const unsigned long long m = __ballot(valid && set);
            peers &= set ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0u) cnt[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        {                                                        // thread d: digit d's offsets for the four waves, in wave order
            uint32_t acc = base[tid];
            for (uint32_t w = 0; w < kSortWaves; w++) {
                const uint32_t c = cnt[w][tid];
                cnt[w][tid] = 0u;
                off[w][tid] = acc;
                acc += c;
            }
            base[tid] = acc;
        }
        __syncthreads();
        if (valid) {
            dst[off[wave][digit] + rank] = PASS == 3 ? __float_as_uint(float_of(key)) : key;   // < n: the offsets are a scan of the counts
        }
    }
}

template <int PASS>
int sort_pass(const uint32_t* src, uint32_t* dst, uint32_t* hist, uint32_t n, uint32_t blocks, uint32_t per_block, hipStream_t st) {
    int rc;
    if ((rc = launch_kernel(k_occ_hist<PASS>, blocks, kSortThreads, 0, st, src, n, per_block, hist)) ||
        (rc = launch_kernel(k_occ_scan, 1u, 1024u, 0, st, hist, 256u * blocks))) return rc;
    return launch_kernel(k_occ_scatter<PASS>, blocks, kSortThreads, 0, st, src, dst, n, per_block, (const uint32_t*)hist);
}

// ---- rank and filter ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_rank(OccRankArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t negN = a.n_neg;
    const float eps = 1.0e-5f, negNf = (float)negN;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_pos; i += stride) {
        const float Sl = a.pos[i];
        uint32_t lo = 0u, hi = negN;                             // std::upper_bound: the first negative above Sl
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (Sl < a.neg[mid]) hi = mid; else lo = mid + 1u;
        }
        const uint32_t FPl = negN - lo;
        OccCand c;
        c.window = i; c.score = Sl; c.fp = FPl; c.higher = 0.f; c.lower = 0.f;
        bool cand;
        if (FPl == negN) {
            cand = 1.0f < a.p_cutoff;                            // p = 1
        } else if (FPl < 10u && a.expf_branch) {
            cand = true;                                         // the host's expf decides
        } else if (FPl == 0u) {
            c.higher = a.neg[negN - 1u];                         // the reference reads one past the end here (bamm_em.h)
            c.lower = __builtin_inff();
            cand = true;
        } else {
            c.higher = a.neg[lo - 1u];
            c.lower = a.neg[lo];
            // ScoreSeqSet.cpp:118-124 with the host's operations, one rounding each (see the head of this file)
            const float num = (c.higher - Sl) + eps;
            const float den = (c.higher - c.lower) + eps;
            const float p = ((float)FPl + num / den) / negNf;
            cand = !(p >= a.p_cutoff) || !(fabsf(p) <= 3.402823466e38f);   // below the cut-off, NaN or infinite
        }
        // one atomic per wave: the first candidate lane reserves the wave's slots
        const unsigned long long m = __ballot(cand);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            unsigned long long start = 0ull;
            if ((int)lane == leader) start = atomicAdd(a.count, (unsigned long long)__popcll(m));
            const uint32_t s_lo = (uint32_t)__shfl((int)(uint32_t)start, leader);
            const uint32_t s_hi = (uint32_t)__shfl((int)(uint32_t)(start >> 32), leader);
            const unsigned long long slot = (((unsigned long long)s_hi << 32) | s_lo) + (unsigned long long)__popcll(m & below);
            if (cand && slot < a.cap) a.out[slot] = c;           // beyond the capacity: counted only, the host reruns
        }
    }
}

}  // namespace

uint32_t occ_sort_blocks(uint32_t n, uint32_t num_cus) {
    const uint32_t want = (n + 4095u) / 4096u;                   // at least 16 rounds of 256 keys per block
    return std::max(1u, std::min(want, std::min(2048u, num_cus * 8u)));
}

int launch_occ_sort(float* keys, uint32_t* alt, uint32_t* hist, uint32_t n, uint32_t blocks, hipStream_t st) {
    uint32_t per_block = (n + blocks - 1u) / blocks;
    per_block = (per_block + kSortThreads - 1u) / kSortThreads * kSortThreads;
    uint32_t* k = reinterpret_cast<uint32_t*>(keys);
    int rc;
    if ((rc = sort_pass<0>(k, alt, hist, n, blocks, per_block, st)) || (rc = sort_pass<1>(alt, k, hist, n, blocks, per_block, st)) ||
        (rc = sort_pass<2>(k, alt, hist, n, blocks, per_block, st)) || (rc = sort_pass<3>(alt, k, hist, n, blocks, per_block, st))) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_occ_rank(const OccRankArgs& a, uint32_t blocks, hipStream_t st) {
    if (int rc = launch_kernel(k_occ_rank, blocks, 256u, 0, st, a)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm
