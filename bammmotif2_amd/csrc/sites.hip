// The device half of bamm_em_sites (sites.cpp): dense r, wherever the E kernels or EM::mask left it, reduced to the
// windows whose r reaches a cut-off -- the rows of EM::write's .positions (EM.cpp:577-601) -- and to every sequence's
// best window as GibbsSampling.cpp:105-116 picks it.  Three launches over a run of sequences:
//
//   k_sites_count  one wavefront per sequence; the lanes stride over the window starts i = 0 .. L-W (neighbouring lanes
//                  read neighbouring floats), count r >= cutoff by ballot and keep the first maximum above 0
//   k_sites_scan   exclusive 64-bit prefix sum of the counts (one block: it is sequences, not positions)
//   k_sites_write  the same walk; a hit's rank inside its sequence is the hits of the earlier strides plus the hits in
//                  the lanes below it, its slot the sequence's offset plus that rank
//
// The list comes out in ascending (sequence, window start) order whatever the scheduling: no atomic decides a slot.
// Nothing holds a sequence in registers, so any length goes.  Plain loads and stores, ballots and shuffles only.

#include "common.h"

namespace bamm {
namespace {

constexpr uint32_t kSitesThreads = 256, kSitesWaves = kSitesThreads / 64;
constexpr uint32_t kNoWindow = 0xffffffffu;

struct SiteSeq {                 // one sequence's r and its windows
    const float* r;
    uint32_t L, windows;
};
__device__ __forceinline__ SiteSeq open_site_seq(const SitesArgs& a, uint32_t seq) {
    SiteSeq s;
    s.L = a.len[seq];
    s.windows = s.L >= a.W ? s.L - a.W + 1u : 0u;
    s.r = a.r + (a.pos_off[seq] - a.r_base);
    return s;
}
// where window start i lies: the reference's reversed index (EM.cpp:173), or the slot of the window's last column
__device__ __forceinline__ uint32_t r_index(const SitesArgs& a, const SiteSeq& s, uint32_t i) {
    return a.slot_layout ? i + a.W - 1u : s.L - a.W - i;
}

__global__ __launch_bounds__(kSitesThreads) void k_sites_count(SitesArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * kSitesWaves + (threadIdx.x >> 6), total_waves = gridDim.x * kSitesWaves;
    for (uint32_t t = wave; t < a.n_seqs; t += total_waves) {
        const uint32_t seq = a.seq_begin + t;
        const SiteSeq s = open_site_seq(a, seq);
        uint32_t hits = 0u, best_i = kNoWindow;
        float best = 0.0f;
        for (uint32_t i0 = 0u; i0 < s.windows; i0 += 64u) {      // wave-uniform trip count
            const uint32_t i = i0 + lane;
            const bool valid = i < s.windows;
            const float v = valid ? s.r[r_index(a, s, i)] : 0.0f;
            hits += (uint32_t)__popcll(__ballot(valid && v >= a.cutoff));
            if (valid && v > best) { best = v; best_i = i; }    // a lane's windows ascend: its first maximum stays
        }
        // the wave's maximum, the lowest window start among equals: what a strict `>` walking i upwards keeps
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(best, d);
            const uint32_t oi = (uint32_t)__shfl_xor((int)best_i, d);
            if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
        }
        if (lane == 0u) {
            const uint32_t o = seq - a.out_begin;
            a.count[o] = hits;
            a.z[o] = best_i == kNoWindow ? 0u : best_i + 1u;
            a.r_best[o] = best;
        }
    }
}

// one block; thread t sums a contiguous run of the counts, the runs' totals are scanned in LDS
__global__ __launch_bounds__(1024) void k_sites_scan(const uint32_t* __restrict__ count, unsigned long long* __restrict__ offset,
                                                     uint32_t n, unsigned long long base, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long part[1024];
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t b = min(threadIdx.x * per, n), e = min(b + per, n);
    unsigned long long sum = 0ull;
    for (uint32_t i = b; i < e; i++) sum += count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        const unsigned long long add = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = base + part[threadIdx.x] - sum;
    for (uint32_t i = b; i < e; i++) {
        offset[i] = run;
        run += count[i];
    }
    if (threadIdx.x == 1023u) *total = base + part[1023];
}

__global__ __launch_bounds__(kSitesThreads) void k_sites_write(SitesArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t wave = blockIdx.x * kSitesWaves + (threadIdx.x >> 6), total_waves = gridDim.x * kSitesWaves;
    for (uint32_t t = wave; t < a.n_seqs; t += total_waves) {
        const uint32_t seq = a.seq_begin + t;
        const SiteSeq s = open_site_seq(a, seq);
        unsigned long long at = a.offset[seq - a.out_begin] - a.out_base;   // the sequence's next free record
        for (uint32_t i0 = 0u; i0 < s.windows; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const bool valid = i < s.windows;
            const float v = valid ? s.r[r_index(a, s, i)] : 0.0f;
            const bool hit = valid && v >= a.cutoff;
            const unsigned long long m = __ballot(hit);
            const unsigned long long slot = at + (unsigned long long)__popcll(m & below);
            if (hit && slot < a.out_cap) a.out[slot] = SiteRec{seq, i, v};   // the offsets are a scan of the same test: always inside
            at += (unsigned long long)__popcll(m);
        }
    }
}

}  // namespace

int launch_sites_count(const SitesArgs& a, uint32_t blocks, hipStream_t st) {
    if (int rc = launch_kernel(k_sites_count, blocks, kSitesThreads, 0, st, a)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_sites_scan(const uint32_t* count, unsigned long long* offset, uint32_t n, unsigned long long base, unsigned long long* total,
                      hipStream_t st) {
    if (int rc = launch_kernel(k_sites_scan, 1u, 1024u, 0, st, count, offset, n, base, total)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_sites_write(const SitesArgs& a, uint32_t blocks, hipStream_t st) {
    if (int rc = launch_kernel(k_sites_write, blocks, kSitesThreads, 0, st, a)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm
