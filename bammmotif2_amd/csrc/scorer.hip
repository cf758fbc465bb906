// The log-odds scorer with the table in LDS: ScoreSeqSet::calcLogOdds, seq_scoring/ScoreSeqSet.cpp:41-66.
//
//   k_score              one wavefront per sequence of a length class (up to 8192 positions)
//   k_score_tile         the same over one tile of one longer sequence
//   k_score_tile_reduce  that sequence's maximum (ScoreSeqSet.cpp:46-57) over its tiles
//   k_score_slice, k_score_tile_slice   the first two over a slice of the motif's columns: tables beyond the LDS of a CU
//
// A window's score is W additions, left to right, of table entries picked by the k-mers inside the window: it depends on
// nothing else in the sequence.  Lane l holds M consecutive positions in registers, the table lives in LDS as [W][Y+1]
// (row Y = 0.0f), and the window sums are a systolic chain whose only cross-lane traffic is one wave_shr1 per motif
// column.  That chain exists once, in score_chain, and so does the wave's first arg-max (wave_first_max, device_utils.h):
// both kernels load the table, pick a sequence or a tile, decode it, run score_chain, emit their windows and fold the
// maximum -- so every route adds the same numbers in the same order, bit for bit what k_long_score (long_seq.hip) and
// the reference give.
//
// Tiles: a sequence beyond the length classes is cut into tiles of 64 * M positions that overlap by at least W - 1.  A
// tile starts on a multiple of the stride, the stride is a multiple of 16 (a tile starts on a word of the 2-bit stream)
// and at most 64 * M - (W - 1); a tile emits the windows that start in [t0, t0 + stride), the sequence's last tile up to
// L - W.  A tile is found from its index: the launch carries the prefix sums of the bucket's tile counts, one entry per
// long sequence, and a wave searches them.  A sequence the mask leaves out has no tiles.  Every tile leaves (best, first
// window that reaches it), the reduction folds a sequence's tiles with the scorer's rule (strict >, the lowest index
// among equals) -- no float atomics, nothing that depends on scheduling.
//
// No contraction, no fast math (build.py): the additions are IEEE fp32.
#include "device_utils.h"
#include "mclass.h"
#include "tiles.h"

#include <algorithm>
#include <cfloat>

// The tiles' one geometry (positions per lane, threads per block: a class of BAMM_FOR_EACH_MCLASS, mclass.h), chosen by
// measurement (profiles/score_tiles_ab.txt).  tools/score_tiles_ab.py builds the other candidates by overriding the two.
#ifndef BAMM_SCORE_TILE_M
#define BAMM_SCORE_TILE_M 32
#define BAMM_SCORE_TILE_THREADS 512
#endif

namespace bamm {
namespace {

constexpr int kTileM = BAMM_SCORE_TILE_M, kTileThreads = BAMM_SCORE_TILE_THREADS;
constexpr uint32_t kTilePositions = 64u * (uint32_t)kTileM;
static_assert(kTileThreads % 64 == 0 && kTileThreads <= 1024, "whole waves");

// The scoring chain, once.  y[m]: the k-mer at position lane * M + m of the sequence or tile the wave holds; s_lds: the
// table [W][Ys].  After column j, U[m] is the sum of columns 0..j of the window that ends j columns further on: W
// additions per window, left to right (ScoreSeqSet.cpp:49-54; 0.0f + s == s).  Slot p = lane * M + m is left holding the
// score of window i = p + 1 - W.
// (The emit loops behind it stay with their kernels.  In one function with the chain, every spelling of the emit guard
// tried cost one of the two callers: `p < end` is the compare k_score's decode makes too and keeps its 23 classes'
// registers, but k_score_tile<32, 512> then needs 149 VGPRs instead of 118 and loses a wave per SIMD; `i < n_emit` keeps
// the tile kernel's and puts more scratch into k_score<56> and <64>.  profiles/scorer_refactor_isa.txt)
// It is written as its two pieces -- the first column, and n further columns from any state of U -- because the sum can be
// cut at any column: a slice of columns (k_score_slice, k_score_tile_slice below) puts back the U its predecessor left
// and goes on with score_chain_columns, so the additions stand here and nowhere else.
template <int M>
__device__ __forceinline__ void score_chain_open(const uint32_t (&y)[M], const float* s0, float (&U)[M]) {
#pragma unroll
    for (int m = 0; m < M; m++) U[m] = s0[y[m]];
}

// n further columns; sj: the table row of the first of them
template <int M>
__device__ __forceinline__ void score_chain_columns(const uint32_t (&y)[M], const float* sj, uint32_t n, uint32_t Ys, float (&U)[M]) {
    for (uint32_t j = 0; j < n; j++, sj += Ys) {
        const float carry = wave_shr1(0.0f, U[M - 1]);
#pragma unroll
        for (int m = M - 1; m >= 1; m--) U[m] = U[m - 1] + sj[y[m]];
        U[0] = carry + sj[y[0]];
    }
}

template <int M>
__device__ __forceinline__ void score_chain(const uint32_t (&y)[M], const float* s_lds, uint32_t W, uint32_t Ys, float (&U)[M]) {
    score_chain_open<M>(y, s_lds, U);
    score_chain_columns<M>(y, s_lds + Ys, W - 1u, Ys, U);
}

// the block's copy of the log-odds table
__device__ __forceinline__ void load_table(float* s_lds, const float* s, uint32_t cells) {
    for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) s_lds[i] = s[i];
    __syncthreads();
}

template <int M, int THREADS>
__global__ void __launch_bounds__(THREADS) k_score(ScoreKernelArgs a) {
    extern __shared__ float lds[];
    const uint32_t W = a.W, Ys = a.Y + 1u;
    load_table(lds, a.s, W * Ys);

    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t total_waves = gridDim.x * waves_per_block;

    for (uint32_t t = blockIdx.x * waves_per_block + wave; t < a.sv.count; t += total_waves) {
        const uint32_t seq = pick_sequence(a.sv, t);
        if (a.sv.mask && !a.sv.mask[seq]) continue;
        const uint32_t L = a.sv.len[seq];
        uint32_t y[M];
        decode_positions<M>(a.sv, seq, L, a.Y, L, lane, y);   // full windows (ScoreSeqSet.cpp:49-54)
        const uint32_t p0 = (uint32_t)lane * M;
        float U[M];
        score_chain<M>(y, lds, W, Ys, U);
        float best = -FLT_MAX;                              // ScoreSeqSet.cpp:46
        uint32_t best_i = 0;
        float* mo = a.mops ? a.mops + a.mops_off[seq] : nullptr;
#pragma unroll
        for (int m = 0; m < M; m++) {
            const uint32_t p = p0 + m;
            if (p + 1u >= W && p < L) {                     // every window of the sequence
                const uint32_t i = p + 1u - W;
                if (mo) mo[i] = U[m];
                if (U[m] > best) { best = U[m]; best_i = i; }   // ascending i per lane: the first maximum stays
            }
        }
        const WaveMax r = wave_first_max(best, best_i);
        if (lane == 0) { a.zoops[seq] = r.best; a.z[seq] = r.best_i; }
    }
}

template <int M, int THREADS>
__global__ void __launch_bounds__(THREADS) k_score_tile(ScoreTileArgs a) {
    extern __shared__ float lds[];
    const uint32_t W = a.k.W, Ys = a.k.Y + 1u;
    load_table(lds, a.k.s, W * Ys);

    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t total_waves = gridDim.x * waves_per_block;

    for (uint32_t g = blockIdx.x * waves_per_block + wave; g < a.n_tiles; g += total_waves) {
        const uint32_t t = tile_owner(a.tile_off, a.k.sv.count, g);
        const uint32_t seq = pick_sequence(a.k.sv, t);
        const uint32_t L = a.k.sv.len[seq];
        const uint32_t t0 = (g - a.tile_off[t]) * a.stride;
        const uint32_t n_emit = min(a.stride, L - W + 1u - t0);   // windows t0 .. t0 + n_emit - 1 are this tile's
        uint32_t y[M];
        decode_tile<M>(a.k.sv, seq, L, a.k.Y, t0, lane, y);
        const uint32_t p0 = (uint32_t)lane * M;
        float U[M];
        score_chain<M>(y, lds, W, Ys, U);
        float best = -FLT_MAX;
        uint32_t best_i = 0;
        float* mo = a.k.mops ? a.k.mops + a.k.mops_off[seq] + t0 : nullptr;
#pragma unroll
        for (int m = 0; m < M; m++) {
            const uint32_t p = p0 + m;                       // U[m]: the window that ends at tile position p
            if (p + 1u >= W && p + 1u - W < n_emit) {
                const uint32_t i = p + 1u - W;
                if (mo) mo[i] = U[m];
                if (U[m] > best) { best = U[m]; best_i = t0 + i; }
            }
        }
        const WaveMax r = wave_first_max(best, best_i);
        if (lane == 0) { a.tile_best[g] = r.best; a.tile_idx[g] = r.best_i; }
    }
}

// a wave per sequence: lane l folds tiles l, l + 64, ... in ascending order (strict >: the first maximum stays), then the
// lanes' results fold with the lowest index among equals -- what one walk over the tiles in ascending order leaves
__global__ void __launch_bounds__(256) k_score_tile_reduce(ScoreTileArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves_per_block = blockDim.x >> 6, total_waves = gridDim.x * waves_per_block;
    for (uint32_t t = blockIdx.x * waves_per_block + (threadIdx.x >> 6); t < a.k.sv.count; t += total_waves) {
        const uint32_t g0 = a.tile_off[t], g1 = a.tile_off[t + 1u];
        if (g0 == g1) continue;                             // outside the mask: the zeros stay
        float best = -FLT_MAX;
        uint32_t best_i = 0;
        for (uint32_t g = g0 + (uint32_t)lane; g < g1; g += 64u) {
            const float b = a.tile_best[g];
            if (b > best) { best = b; best_i = a.tile_idx[g]; }
        }
        const WaveMax r = wave_first_max(best, best_i);
        if (lane == 0) {
            const uint32_t seq = pick_sequence(a.k.sv, t);
            a.k.zoops[seq] = r.best;
            a.k.z[seq] = r.best_i;
        }
    }
}

// ---- column slices: log-odds tables beyond the LDS of a CU (score_slice_geometry) ----
// A launch holds the columns [j0, j1) of the table and adds only those.  After column j slot p holds the sum of columns
// 0..j of window p - j, so the state of the chain after column j1 - 1 is one float per window: the slice writes
// partial[p + 1 - j1] from slot p, its successor reads partial[p + 1 - j0] back into the same slot -- the registers as the
// unsliced chain would hold them there -- and goes on adding.  Slots that hold no window of the sequence (of the tile's emit
// range) restart from 0.0f: their sums are never emitted and never reach a slot that is.  A wave reads and writes the
// windows of its own sequence or tile only, the launches of a call follow each other on one stream, and the last slice
// emits and folds the maximum as the unsliced kernels do: the same additions in the same order.

// f(m, i) for every slot m of the lane that holds one of the windows i = 0 .. nwin - 1 after `cols` columns.  The guard in
// the spelling of the caller's unsliced kernel (see score_chain): BY_END compares the slot with the windows' end as k_score
// does, otherwise the window with their number as k_score_tile does.
template <int M, bool BY_END, class F>
__device__ __forceinline__ void for_each_window(uint32_t p0, uint32_t cols, uint32_t nwin, F&& f) {
    const uint32_t end = nwin + cols - 1u;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const uint32_t p = p0 + m;
        if (p + 1u >= cols && (BY_END ? p < end : p + 1u - cols < nwin)) f(m, p + 1u - cols);
    }
}

// where slot 0 of the lane finds its window after `cols` columns in an array of the sequence's windows: slot m's is
// lane_windows(...)[m], one address per lane and a constant beside it (only slots that hold a window are touched)
__device__ __forceinline__ float* lane_windows(float* windows, uint32_t p0, uint32_t cols) {
    return windows + ((ptrdiff_t)p0 + 1 - (ptrdiff_t)cols);
}

// this slice's columns over the windows 0 .. nwin - 1, whose carrier starts at part; false: U holds the windows' scores
template <int M, bool BY_END>
__device__ __forceinline__ bool score_chain_slice(const uint32_t (&y)[M], const float* lds, const ScoreSlice& sl, uint32_t W, uint32_t Ys,
                                                  uint32_t p0, uint32_t nwin, float* part, float (&U)[M]) {
    if (sl.j0 == 0) {
        score_chain_open<M>(y, lds, U);
    } else {
#pragma unroll
        for (int m = 0; m < M; m++) U[m] = 0.0f;
        const float* in = lane_windows(part, p0, sl.j0);
        for_each_window<M, BY_END>(p0, sl.j0, nwin, [&](int m, uint32_t) { U[m] = in[m]; });
    }
    const uint32_t first = sl.j0 == 0 ? 1u : 0u;
    score_chain_columns<M>(y, lds + first * Ys, sl.j1 - sl.j0 - first, Ys, U);
    if (sl.j1 == W) return false;
    float* out = lane_windows(part, p0, sl.j1);
    for_each_window<M, BY_END>(p0, sl.j1, nwin, [&](int m, uint32_t) { out[m] = U[m]; });
    return true;
}

template <int M, int THREADS>
__global__ void __launch_bounds__(THREADS) k_score_slice(ScoreKernelArgs a, ScoreSlice sl) {
    extern __shared__ float lds[];
    const uint32_t W = a.W, Ys = a.Y + 1u;
    load_table(lds, a.s + (size_t)sl.j0 * Ys, (sl.j1 - sl.j0) * Ys);

    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t total_waves = gridDim.x * waves_per_block;

    for (uint32_t t = blockIdx.x * waves_per_block + wave; t < a.sv.count; t += total_waves) {
        const uint32_t seq = pick_sequence(a.sv, t);
        if (a.sv.mask && !a.sv.mask[seq]) continue;
        const uint32_t L = a.sv.len[seq];
        uint32_t y[M];
        decode_positions<M>(a.sv, seq, L, a.Y, L, lane, y);
        const uint32_t p0 = (uint32_t)lane * M, nwin = L - W + 1u;
        float U[M];
        if (score_chain_slice<M, true>(y, lds, sl, W, Ys, p0, nwin, sl.partial + a.mops_off[seq], U)) continue;
        float best = -FLT_MAX;
        uint32_t best_i = 0;
        float* mo = a.mops ? lane_windows(a.mops + a.mops_off[seq], p0, W) : nullptr;
        for_each_window<M, true>(p0, W, nwin, [&](int m, uint32_t i) {
            if (mo) mo[m] = U[m];
            if (U[m] > best) { best = U[m]; best_i = i; }
        });
        const WaveMax r = wave_first_max(best, best_i);
        if (lane == 0) { a.zoops[seq] = r.best; a.z[seq] = r.best_i; }
    }
}

template <int M, int THREADS>
__global__ void __launch_bounds__(THREADS) k_score_tile_slice(ScoreTileArgs a, ScoreSlice sl) {
    extern __shared__ float lds[];
    const uint32_t W = a.k.W, Ys = a.k.Y + 1u;
    load_table(lds, a.k.s + (size_t)sl.j0 * Ys, (sl.j1 - sl.j0) * Ys);

    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t total_waves = gridDim.x * waves_per_block;

    for (uint32_t g = blockIdx.x * waves_per_block + wave; g < a.n_tiles; g += total_waves) {
        const uint32_t t = tile_owner(a.tile_off, a.k.sv.count, g);
        const uint32_t seq = pick_sequence(a.k.sv, t);
        const uint32_t L = a.k.sv.len[seq];
        const uint32_t t0 = (g - a.tile_off[t]) * a.stride;
        const uint32_t n_emit = min(a.stride, L - W + 1u - t0);   // the tile's windows, in the carrier as in mops
        uint32_t y[M];
        decode_tile<M>(a.k.sv, seq, L, a.k.Y, t0, lane, y);
        const uint32_t p0 = (uint32_t)lane * M;
        float U[M];
        if (score_chain_slice<M, false>(y, lds, sl, W, Ys, p0, n_emit, sl.partial + a.k.mops_off[seq] + t0, U)) continue;
        float best = -FLT_MAX;
        uint32_t best_i = 0;
        float* mo = a.k.mops ? lane_windows(a.k.mops + a.k.mops_off[seq] + t0, p0, W) : nullptr;
        for_each_window<M, false>(p0, W, n_emit, [&](int m, uint32_t i) {
            if (mo) mo[m] = U[m];
            if (U[m] > best) { best = U[m]; best_i = t0 + i; }
        });
        const WaveMax r = wave_first_max(best, best_i);
        if (lane == 0) { a.tile_best[g] = r.best; a.tile_idx[g] = r.best_i; }
    }
}

// a launch's slice: whole columns of a table that does not fit, inside the motif, its part of the table within the LDS
bool bad_slice(const ScoreKernelArgs& a, const ScoreSlice& sl, size_t* lds) {
    *lds = (size_t)(sl.j1 - sl.j0) * (a.Y + 1) * sizeof(float);
    if (sl.partial && sl.j0 < sl.j1 && sl.j1 <= a.W && *lds <= 160 * 1024 && a.mops_off) return false;
    set_error("score slice [%u, %u) of W=%u: %zu bytes of LDS, carrier %p", sl.j0, sl.j1, a.W, *lds, (void*)sl.partial);
    return true;
}

}  // namespace

int launch_score_slice(int mclass, const ScoreKernelArgs& a, const ScoreSlice& sl, uint32_t blocks, uint32_t threads, hipStream_t st) {
    size_t lds = 0;
    if (bad_slice(a, sl, &lds)) return BAMM_ERR_ARG;
    if (threads > max_threads_for_mclass(mclass) || (threads & 63u) || threads == 0 || blocks == 0) {
        set_error("bad launch geometry %u x %u for M class %d", blocks, threads, mclass);
        return BAMM_ERR_ARG;
    }
    if (int rc = with_mclass(mclass, [&](auto M, auto T) { return launch_kernel(&k_score_slice<M, T>, blocks, threads, lds, st, a, sl); }))
        return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_score_tiles_slice(const ScoreTileArgs& a, const ScoreSlice& sl, uint32_t blocks, hipStream_t st) {
    if (a.n_tiles == 0) return BAMM_OK;
    size_t lds = 0;
    uint32_t tp = 0, stride = 0;
    if (bad_slice(a.k, sl, &lds)) return BAMM_ERR_ARG;
    if (!score_tile_geometry(a.k.W, &tp, &stride) || stride != a.stride || blocks == 0) {
        set_error("k_score_tile_slice: W=%u, stride %u or %u blocks is outside the tiles' envelope", a.k.W, a.stride, blocks);
        return BAMM_ERR_ARG;
    }
    if (int rc = launch_kernel(&k_score_tile_slice<kTileM, kTileThreads>, blocks, (uint32_t)kTileThreads, lds, st, a, sl)) return rc;
    BAMM_HIP(hipGetLastError());
    if (sl.j1 < a.k.W) return BAMM_OK;
    hipLaunchKernelGGL(k_score_tile_reduce, dim3(std::min((a.k.sv.count + 3u) / 4u, 1024u)), dim3(256), 0, st, a);
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_score(int mclass, const ScoreKernelArgs& a, uint32_t blocks, uint32_t threads, hipStream_t st) {
    const size_t lds = (size_t)a.W * (a.Y + 1) * sizeof(float);
    if (lds > 160 * 1024) {
        set_error("log-odds table needs %zu bytes of LDS (> 160 KiB)", lds);
        return BAMM_ERR_UNSUPPORTED;
    }
    if (threads > max_threads_for_mclass(mclass) || (threads & 63u) || threads == 0 || blocks == 0) {
        set_error("bad launch geometry %u x %u for M class %d", blocks, threads, mclass);
        return BAMM_ERR_ARG;
    }
    if (int rc = with_mclass(mclass, [&](auto M, auto T) { return launch_kernel(&k_score<M, T>, blocks, threads, lds, st, a); }))
        return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

bool score_tile_geometry(uint32_t W, uint32_t* tile_positions, uint32_t* stride) {
    if (W == 0 || W > kTilePositions) return false;
    const uint32_t st = (kTilePositions - (W - 1u)) & ~15u;  // the largest multiple of 16 that leaves an overlap of W - 1
    if (st < 16u) return false;
    if (tile_positions) *tile_positions = kTilePositions;
    if (stride) *stride = st;
    return true;
}

uint32_t score_tile_threads() { return (uint32_t)kTileThreads; }

int launch_score_tiles(const ScoreTileArgs& a, uint32_t blocks, hipStream_t st) {
    if (a.n_tiles == 0) return BAMM_OK;
    const size_t lds = (size_t)a.k.W * (a.k.Y + 1) * sizeof(float);
    uint32_t tp = 0, stride = 0;
    if (lds > 160 * 1024 || !score_tile_geometry(a.k.W, &tp, &stride) || stride != a.stride || blocks == 0) {
        set_error("k_score_tile: W=%u, stride %u, a table of %zu bytes or %u blocks is outside the tiles' envelope", a.k.W, a.stride, lds, blocks);
        return BAMM_ERR_ARG;
    }
    if (int rc = launch_kernel(&k_score_tile<kTileM, kTileThreads>, blocks, (uint32_t)kTileThreads, lds, st, a)) return rc;
    BAMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_score_tile_reduce, dim3(std::min((a.k.sv.count + 3u) / 4u, 1024u)), dim3(256), 0, st, a);
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm
