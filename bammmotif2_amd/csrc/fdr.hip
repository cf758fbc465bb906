// The device half of FDR::calculatePR's MOPS branch and of FDR::calculatePvalues (FDR.cpp:156-196, :278-333; restated
// for the host in host/fdr.cpp: fdr_statistics) over the window scores where k_score left them (fdr_stats.cpp).
//
// The reference sorts both score lists descending and walks them in one serial loop: step i takes the next positive iff
// it is strictly above the next negative (ties go to the negative, an exhausted list never wins), counts ip / in, and
// derives tp, fp from the counts.  That walk is a MERGE, so the counts after any number of steps follow from a
// merge-path search on that diagonal -- nothing is carried from step to step but the running maximum of tp:
//
//   k_fdr_partition   one search per block boundary (a block owns kFdrStepsPerBlock consecutive steps) in global memory;
//   tile_open         a block stages the scores its steps consume -- exactly as many floats as it has steps -- in LDS,
//                     every thread searches its own diagonal there and then merges kFdrStepsPerThread steps serially;
//   peak              E_TP is a running maximum (exact, associative), idx_max the LAST step whose tp equals the maximum
//                     in front of it: per-block maxima (k_fdr_block_max), one block turns them into the maximum in
//                     front of every block (k_fdr_scan_max), every block walks again with its carry-in and reports its
//                     last equality (k_fdr_last_eq; an integer atomicMax).  tp is recomputed, never stored;
//   k_fdr_rows        tp / fp / fdr / rec of a caller-chosen range of steps, by the same search;
//   k_fdr_pvalues     lower and upper bound of every positive score in the ascending negatives.
//
// The lists arrive ASCENDING (launch_occ_sort) and are read from the top.  Which block or thread owns a step is fixed by
// the step's index, so no result depends on a launch geometry.  All numbers come from fdr_rows.h, which the host path
// includes as well; build.py compiles this unit with IEEE division and fp32 denormals kept, no unit of the library is
// built with contraction or fast-math.

#include "common.h"
#include "fdr_rows.h"
#include "sort_key.h"

namespace bamm {
namespace {

constexpr uint32_t SPT = kFdrStepsPerThread, SPB = kFdrStepsPerBlock;

// element i of the descending order; beyond the list (never reached with finite scores): a value that loses every comparison
__device__ __forceinline__ float desc_at(const float* asc, uint64_t n, uint64_t i) { return i < n ? asc[n - 1u - i] : -__builtin_inff(); }

// The diagonal search of a merge of list A (na elements) with list B (nb): how many of the first k elements taken come from
// A -- the smallest i with NOT a_first(i, k - 1 - i), where a_first(i, j) says that A[i] is taken before B[j].
template <class I, class F>
__device__ __forceinline__ I merge_diagonal(I k, I na, I nb, F&& a_first) {
    I lo = k > nb ? k - nb : 0u, hi = k < na ? k : na;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);                 // lo <= mid < hi <= min(k, na); k - nb <= mid: 0 <= k - 1 - mid < nb
        if (a_first(mid, k - 1u - mid)) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// positives among the first k steps of the walk: the smallest i with NOT pos[i] > neg[k - 1 - i]
__device__ uint64_t merge_path(const FdrWalkArgs& a, uint64_t k) {
    return merge_diagonal<uint64_t>(k, a.n_pos, a.n_neg, [&](uint64_t i, uint64_t j) { return desc_at(a.pos, a.n_pos, i) > desc_at(a.neg, a.n_neg, j); });
}

__global__ __launch_bounds__(kFdrThreads) void k_fdr_partition(FdrWalkArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * kFdrThreads + threadIdx.x, total = a.n_pos + a.n_neg;
    if (g > a.n_blocks) return;
    const uint64_t k = g * SPB < total ? g * SPB : total;
    a.part[g] = merge_path(a, k);
}

// a block's share of the walk, staged: steps k0 .. k0 + n - 1 take positives ip0 .. ip0 + na - 1 and negatives
// in0 .. in0 + nc - 1 (descending indices), na + nc = n; this thread starts at step k0 + d with i / j of them taken
struct Tile {
    uint64_t k0, ip0, in0;
    uint32_t n, na, nc, d, i, j;
    const float *sP, *sN;
};

__device__ __forceinline__ Tile tile_open(const FdrWalkArgs& a, uint64_t blk, float* lds) {
    Tile t;
    const uint64_t total = a.n_pos + a.n_neg;
    t.k0 = blk * SPB;
    t.n = (uint32_t)((total - t.k0 < SPB) ? total - t.k0 : SPB);
    t.ip0 = a.part[blk];
    const uint64_t ip1 = a.part[blk + 1u];
    t.in0 = t.k0 - t.ip0;                                    // part[blk] <= k0 (merge_path's upper bound)
    const uint64_t na = ip1 > t.ip0 ? ip1 - t.ip0 : 0u;      // a merge never takes more than n; the clamps keep scores that do not
    t.na = (uint32_t)(na < t.n ? na : t.n);                  // order (NaN) inside the tile
    t.nc = t.n - t.na;
    for (uint32_t x = threadIdx.x; x < t.n; x += kFdrThreads)
        lds[x] = x < t.na ? desc_at(a.pos, a.n_pos, t.ip0 + x) : desc_at(a.neg, a.n_neg, t.in0 + (x - t.na));
    __syncthreads();
    t.sP = lds; t.sN = lds + t.na;
    t.d = threadIdx.x * SPT < t.n ? threadIdx.x * SPT : t.n;
    t.i = merge_diagonal<uint32_t>(t.d, t.na, t.nc, [&](uint32_t i, uint32_t j) { return t.sP[i] > t.sN[j]; });
    t.j = t.d - t.i;
    return t;
}

// f(step, ip, in) for this thread's steps, ip / in counted AFTER the step (FDR.cpp:174-179)
template <class F>
__device__ __forceinline__ void tile_walk(const Tile& t, F&& f) {
    uint32_t i = t.i, j = t.j;
    for (uint32_t s = 0; s < SPT && t.d + s < t.n; s++) {
        const bool take = i < t.na && (j >= t.nc || t.sP[i] > t.sN[j]);
        i += take ? 1u : 0u;
        j += take ? 0u : 1u;
        f(t.k0 + t.d + s, t.ip0 + i, t.in0 + j);
    }
}

// the reference's `if (E_TP < tp) E_TP = tp` as a combine: the earlier operand stays unless the later one is above it
__device__ __forceinline__ float later_max(float earlier, float later) { return earlier < later ? later : earlier; }

__device__ __forceinline__ float thread_max(const FdrWalkArgs& a, const Tile& t) {
    float m = -__builtin_inff();
    tile_walk(t, [&](uint64_t, uint64_t ip, uint64_t in) { m = later_max(m, fdr_tp(ip, in, a.m_fold)); });
    return m;
}

__global__ __launch_bounds__(kFdrThreads) void k_fdr_block_max(FdrWalkArgs a) {
    __shared__ float lds[SPB];
    __shared__ float red[kFdrThreads];
    const Tile t = tile_open(a, blockIdx.x, lds);
    red[threadIdx.x] = thread_max(a, t);
    __syncthreads();
    for (uint32_t w = kFdrThreads / 2u; w > 0u; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = later_max(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0u) a.block_max[blockIdx.x] = red[0];
}

// block_max[b] <- the running maximum in front of block b (0 in front of the first), peak->e_tp <- the maximum behind
// the last: one block, every thread a contiguous run
__global__ __launch_bounds__(1024) void k_fdr_scan_max(FdrWalkArgs a) {
    __shared__ float part[1024];
    const uint64_t per = (a.n_blocks + 1023u) / 1024u;
    const uint64_t b = threadIdx.x * per < a.n_blocks ? threadIdx.x * per : a.n_blocks, e = b + per < a.n_blocks ? b + per : a.n_blocks;
    float m = -__builtin_inff();
    for (uint64_t i = b; i < e; i++) m = later_max(m, a.block_max[i]);
    part[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        const float front = threadIdx.x >= d ? part[threadIdx.x - d] : -__builtin_inff();
        __syncthreads();
        part[threadIdx.x] = later_max(front, part[threadIdx.x]);
        __syncthreads();
    }
    float run = 0.0f;                                        // E_TP starts at 0 (FDR.cpp:163)
    if (threadIdx.x > 0u) run = later_max(run, part[threadIdx.x - 1u]);
    for (uint64_t i = b; i < e; i++) {
        const float c = a.block_max[i];
        a.block_max[i] = run;
        run = later_max(run, c);
    }
    if (threadIdx.x == 1023u) { a.peak->e_tp = run; a.peak->pad = 0u; }
}

__global__ __launch_bounds__(kFdrThreads) void k_fdr_last_eq(FdrWalkArgs a) {
    __shared__ float lds[SPB];
    __shared__ float sc[kFdrThreads];
    __shared__ unsigned long long last[kFdrThreads];
    const Tile t = tile_open(a, blockIdx.x, lds);
    sc[threadIdx.x] = thread_max(a, t);
    __syncthreads();
    for (uint32_t d = 1u; d < kFdrThreads; d <<= 1) {         // inclusive scan of the threads' maxima
        const float front = threadIdx.x >= d ? sc[threadIdx.x - d] : -__builtin_inff();
        __syncthreads();
        sc[threadIdx.x] = later_max(front, sc[threadIdx.x]);
        __syncthreads();
    }
    float e_tp = a.block_max[blockIdx.x];                    // the maximum in front of the block (k_fdr_scan_max)
    if (threadIdx.x > 0u) e_tp = later_max(e_tp, sc[threadIdx.x - 1u]);
    unsigned long long mine = 0ull;
    tile_walk(t, [&](uint64_t k, uint64_t ip, uint64_t in) {
        const FdrPeakStep s = fdr_peak_step(e_tp, fdr_tp(ip, in, a.m_fold));
        if (s.equal) mine = k + 1ull;
        e_tp = s.e_tp;
    });
    last[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t w = kFdrThreads / 2u; w > 0u; w >>= 1) {
        if (threadIdx.x < w && last[threadIdx.x] < last[threadIdx.x + w]) last[threadIdx.x] = last[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0u && last[0]) atomicMax(&a.peak->last_eq, last[0]);
}

__global__ __launch_bounds__(kFdrThreads) void k_fdr_rows(FdrWalkArgs a, uint64_t first_block, uint64_t begin, uint64_t end, float e_tp,
                                                          float* __restrict__ tp_out, float* __restrict__ fp_out,
                                                          float* __restrict__ fdr_out, float* __restrict__ rec_out) {
    __shared__ float lds[SPB];
    const Tile t = tile_open(a, first_block + blockIdx.x, lds);
    tile_walk(t, [&](uint64_t k, uint64_t ip, uint64_t in) {
        if (k < begin || k >= end) return;
        const float tp = fdr_tp(ip, in, a.m_fold), fp = fdr_fp(in, a.m_fold);
        if (tp_out) tp_out[k - begin] = tp;
        if (fp_out) fp_out[k - begin] = fp;
        if (fdr_out) fdr_out[k - begin] = fdr_fdr(tp, fp);
        if (rec_out) rec_out[k - begin] = fdr_rec(tp, e_tp);
    });
}

__global__ __launch_bounds__(kFdrThreads) void k_fdr_pvalues(const float* __restrict__ pos, const float* __restrict__ neg, uint64_t n_neg,
                                                             uint64_t begin, uint64_t end, float* __restrict__ p) {
    const uint64_t i = begin + (uint64_t)blockIdx.x * kFdrThreads + threadIdx.x;
    if (i >= end) return;
    const float x = pos[i];
    uint64_t lo = 0u, hi = n_neg;                            // std::lower_bound: the first negative not below x
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (neg[mid] < x) lo = mid + 1u; else hi = mid;
    }
    const uint64_t low = lo;
    hi = n_neg;                                              // std::upper_bound: the first negative above x (not in front of `low`)
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (x < neg[mid]) hi = mid; else lo = mid + 1u;
    }
    p[i - begin] = fdr_pvalue(low, lo, n_neg);
}

// one wave per segment
__global__ __launch_bounds__(kFdrThreads) void k_fdr_gather(const float* __restrict__ src, float* __restrict__ dst,
                                                            const FdrSeg* __restrict__ seg, uint32_t n_seg) {
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (kFdrThreads / 64u);
    for (uint32_t s = blockIdx.x * (kFdrThreads / 64u) + (threadIdx.x >> 6); s < n_seg; s += waves) {
        const FdrSeg g = seg[s];
        for (uint32_t k = lane; k < g.len; k += 64u) dst[g.dst + k] = src[g.src + k];
    }
}

// ---- merge of two ascending runs (launch_occ_sort's output) into one: what sorting their concatenation gives --------------
// Element k of the output is A[i] or B[k - i] with i from the diagonal search over the sort's own keys (sort_key.h); equal
// keys take A's element first, and since the sort writes canonical bits (-0 comes out as +0) equal keys are equal bits: the
// output does not depend on which run an element came from.  Geometry is the walk's: a block owns SPB consecutive outputs,
// its boundaries come from one search each in global memory (k_fdr_merge_partition), it stages exactly the keys it consumes
// in LDS, every thread searches its own diagonal there and emits SPT outputs serially -- into registers, then through the
// same LDS block, so that the stores to global memory are coalesced.
__device__ __forceinline__ uint64_t merge_blocks(const FdrMergeArgs& m) { return (m.na + m.nb + SPB - 1u) / SPB; }

__global__ __launch_bounds__(kFdrThreads) void k_fdr_merge_partition(FdrMergeArgs m) {
    const uint64_t g = (uint64_t)blockIdx.x * kFdrThreads + threadIdx.x, total = m.na + m.nb;
    if (g > merge_blocks(m)) return;
    const uint64_t k = g * SPB < total ? g * SPB : total;
    m.part[g] = merge_diagonal<uint64_t>(k, m.na, m.nb, [&](uint64_t i, uint64_t j) { return key_of(m.a[i]) <= key_of(m.b[j]); });
}

__global__ __launch_bounds__(kFdrThreads) void k_fdr_merge(FdrMergeArgs m) {
    __shared__ uint32_t lds[SPB];
    const uint64_t total = m.na + m.nb, k0 = (uint64_t)blockIdx.x * SPB;
    const uint32_t n = (uint32_t)(total - k0 < SPB ? total - k0 : SPB);
    const uint64_t ia0 = m.part[blockIdx.x], ia1 = m.part[blockIdx.x + 1u], ib0 = k0 - ia0;   // part[b] <= k0 (the search's upper bound)
    // keys are totally ordered, so the path advances by at most one per output: 0 <= ia1 - ia0 <= n, ia1 <= na and
    // ib0 + (n - (ia1 - ia0)) = k0 + n - ia1 <= nb (the search's lower bound at the next boundary); the clamps restate it
    uint32_t na = (uint32_t)(ia1 > ia0 ? (ia1 - ia0 < n ? ia1 - ia0 : n) : 0u);
    if (ia0 + na > m.na) na = (uint32_t)(m.na - ia0);
    const uint32_t nb = n - na;
    for (uint32_t x = threadIdx.x; x < n; x += kFdrThreads) {
        const uint64_t jb = ib0 + (x - na);
        lds[x] = x < na ? key_of(m.a[ia0 + x]) : (jb < m.nb ? key_of(m.b[jb]) : 0xffffffffu);
    }
    __syncthreads();
    const uint32_t *sA = lds, *sB = lds + na;
    const uint32_t d = threadIdx.x * SPT < n ? threadIdx.x * SPT : n;
    uint32_t i = merge_diagonal<uint32_t>(d, na, nb, [&](uint32_t x, uint32_t y) { return sA[x] <= sB[y]; });
    uint32_t j = d - i;
    uint32_t out[SPT];
    uint32_t ka = i < na ? sA[i] : 0u, kb = j < nb ? sB[j] : 0u;     // the heads of the two runs; one LDS read per output refills the taken one
#pragma unroll
    for (uint32_t s = 0; s < SPT; s++) {
        const bool take = i < na && (j >= nb || ka <= kb);
        out[s] = take ? ka : kb;
        i += take ? 1u : 0u;
        j += take ? 0u : 1u;
        const uint32_t next = take ? i : na + j;             // < n wherever the value is used
        const uint32_t v = next < n ? lds[next] : 0u;
        ka = take ? v : ka;
        kb = take ? kb : v;
    }
    __syncthreads();                                         // every thread has read its inputs: the block becomes the output tile
#pragma unroll
    for (uint32_t s = 0; s < SPT; s++)
        if (d + s < n) lds[d + s] = out[s];
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < n; x += kFdrThreads) m.out[k0 + x] = float_of(lds[x]);
}

}  // namespace

int launch_fdr_merge(const FdrMergeArgs& m, hipStream_t st) {
    const uint64_t total = m.na + m.nb;
    if (!total) return BAMM_OK;
    const uint32_t nb = (uint32_t)((total + kFdrStepsPerBlock - 1u) / kFdrStepsPerBlock);   // <= 2^20: a list holds fewer than 2^32 scores
    int rc;
    if ((rc = launch_kernel(k_fdr_merge_partition, nb / kFdrThreads + 1u, kFdrThreads, 0, st, m)) ||
        (rc = launch_kernel(k_fdr_merge, nb, kFdrThreads, 0, st, m))) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_fdr_peak(const FdrWalkArgs& a, hipStream_t st) {
    const uint32_t nb = (uint32_t)a.n_blocks;                // <= 2^21: each list holds fewer than 2^32 scores
    int rc;
    if ((rc = launch_kernel(k_fdr_partition, nb / kFdrThreads + 1u, kFdrThreads, 0, st, a)) ||
        (rc = launch_kernel(k_fdr_block_max, nb, kFdrThreads, 0, st, a)) ||
        (rc = launch_kernel(k_fdr_scan_max, 1u, 1024u, 0, st, a)) ||
        (rc = launch_kernel(k_fdr_last_eq, nb, kFdrThreads, 0, st, a))) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_fdr_rows(const FdrWalkArgs& a, uint64_t begin, uint64_t end, float e_tp, float* tp, float* fp, float* fdr, float* rec, hipStream_t st) {
    if (begin >= end) return BAMM_OK;
    const uint64_t b0 = begin / kFdrStepsPerBlock, b1 = (end - 1u) / kFdrStepsPerBlock;   // end <= n_pos + n_neg: b1 < n_blocks
    if (int rc = launch_kernel(k_fdr_rows, (uint32_t)(b1 - b0 + 1u), kFdrThreads, 0, st, a, b0, begin, end, e_tp, tp, fp, fdr, rec)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_fdr_pvalues(const float* pos, const float* neg, uint64_t n_neg, uint64_t begin, uint64_t end, float* p, hipStream_t st) {
    if (begin >= end) return BAMM_OK;
    const uint64_t blocks = (end - begin + kFdrThreads - 1u) / kFdrThreads;
    if (int rc = launch_kernel(k_fdr_pvalues, (uint32_t)blocks, kFdrThreads, 0, st, pos, neg, n_neg, begin, end, p)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_fdr_gather(const float* src, float* dst, const FdrSeg* seg, uint32_t n_seg, uint32_t blocks, hipStream_t st) {
    if (!n_seg) return BAMM_OK;
    if (int rc = launch_kernel(k_fdr_gather, blocks, kFdrThreads, 0, st, src, dst, seg, n_seg)) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm
