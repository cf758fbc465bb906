// The EM pass over sequences beyond the length classes (more than 8192 positions), tile by tile on the whole GPU:
// EM::EStep refinement/EM.cpp:149-196, EM::MStep EM.cpp:231-243, the sum over r of EM::optimize_q EM.cpp:509-513 and
// EM::getR's layout EM.cpp:173 -- what k_long_em (long_seq.hip) computes with one workgroup per sequence.
//
//   k_em_tile<M, THREADS, PASS_Z>  every tile's share of its sequence's sum over windows (EM.cpp:180)
//   k_em_tile_norm                 every sequence's Z, 1 / Z and its three pass statistics
//   k_em_tile<M, THREADS, PASS_R>  responsibilities (EM.cpp:185-187), written out and / or counted (EM.cpp:236-242)
//
// A tile is the scorer's (tiles.h): 64 * M positions that start on a multiple of the stride, one wavefront per tile, lane
// l holding M consecutive positions in registers.  The odds table lives in LDS as [W][Y+1] (row Y = 1.0f), the window
// products are k_em_seq's chain for more than 16 positions per lane -- left to right, one v_mul_f32_dpp per column across
// the lanes -- so a product has the bits of window_product (long_seq.hip) and of the reference.  Two things differ from
// the scorer's tiles: positions at or beyond LW1 = L - W + 1 take no part (EM.cpp:167: they read the neutral row and get
// no count), and a sequence the fold mask leaves out is skipped inside the kernels, its tiles being planned all the same
// (getR runs without the mask).
//
// Z is a sum over all tiles of a sequence, hence the three launches.  A tile sums its owned windows' terms in double in a
// fixed order (per lane ascending slot, then an xor butterfly), the sequence's wave sums the tiles in a fixed order (lane l
// takes tiles l, l + 64, ..., then the same butterfly) and rounds once to fp32: k_long_em sums the same fp32 terms in
// double in another order, so the two Z agree except within n * 2^-53 of a rounding boundary (then 1 ulp, r 3 ulps).  A
// sequence's Z depends on its own tiles only -- not on the launch geometry, the other sequences, the mask or the caller
// -- so the pass's integer sums stay exact and order-free.
//
// M-step: the dense count walk of k_em_seq (device_utils.h) on 2^-40 fixed-point addends into a per-block count table
// [W][Y+1][copies] in LDS; a window is counted by the tile that owns it (the addends of the others are 0), a position in
// the overlap receives from this tile's windows here and from the next tile's there.  Block epilogue as k_em_seq's.
//
// No contraction, no fast math (build.py).
#include "device_utils.h"
#include "tiles.h"

#include <algorithm>

// The tiles' one geometry (positions per lane, threads per block), chosen by measurement (profiles/em_tiles_ab.txt).
// tools/em_tiles_ab.py builds the other candidates by overriding the two.
#ifndef BAMM_EM_TILE_M
#define BAMM_EM_TILE_M 32
#define BAMM_EM_TILE_THREADS 512
#endif

namespace bamm {
namespace {

constexpr int kTileM = BAMM_EM_TILE_M, kTileThreads = BAMM_EM_TILE_THREADS;
constexpr uint32_t kTilePositions = 64u * (uint32_t)kTileM;
static_assert(kTileThreads % 64 == 0 && kTileThreads <= 1024, "whole waves");

constexpr int PASS_Z = 0, PASS_R = 1;

// the same value in every lane: a + b == b + a at every step
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the launch takes the sequence (launch_em_tiles sets the range to everything unless the pass only writes a range's r)
__device__ __forceinline__ bool takes_part(const EmKernelArgs& e, uint32_t seq) {
    if (seq < e.seq_begin || seq >= e.seq_end) return false;
    return !(e.sv.mask && !e.sv.mask[seq]);
}

template <int M, int THREADS, int PASS>
__global__ void __launch_bounds__(THREADS) k_em_tile(EmTileArgs a, int accum, int write_r) {
    if (a.e.stop != nullptr && *a.e.stop != 0u) return;  // optimize(): the stop rule fired in an earlier pass

    extern __shared__ __align__(16) float lds[];
    const uint32_t W = a.e.W, Y = a.e.Y, Ys = a.e.Y + 1u;
    float* s_lds = lds;                                  // [W][Y+1], row Y = 1.0f
    // [W][Y+1][C] 64-bit fixed point, C = 2^logC private copies (copy = lane mod C); row Y is never written
    unsigned long long* n_lds = reinterpret_cast<unsigned long long*>(lds + ((W * Ys + 1u) & ~1u));
    const uint32_t logC = (PASS == PASS_R && accum) ? a.e.logC : 0u;
    for (uint32_t i = threadIdx.x; i < W * Ys; i += blockDim.x) s_lds[i] = a.e.s[i];
    if constexpr (PASS == PASS_R)
        if (accum)
            for (uint32_t i = threadIdx.x; i < (W * Ys) << logC; i += blockDim.x) n_lds[i] = 0ull;
    __syncthreads();

    const float q = *a.e.q;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t total_waves = gridDim.x * waves_per_block;

    for (uint32_t g = blockIdx.x * waves_per_block + wave; g < a.n_tiles; g += total_waves) {
        const uint32_t t = tile_owner(a.tile_off, a.e.sv.count, g);
        const uint32_t seq = pick_sequence(a.e.sv, t);
        if (!takes_part(a.e, seq)) continue;
        const uint32_t L = a.e.sv.len[seq], LW1 = L - W + 1u;
        const uint32_t t0 = (g - a.tile_off[t]) * a.stride;
        const uint32_t n_own = min(a.stride, LW1 - t0);      // windows t0 .. t0 + n_own - 1 are this tile's
        const uint32_t p0 = (uint32_t)lane * M;
        uint32_t y[M];
        decode_tile<M>(a.e.sv, seq, L, Y, t0, lane, y);
        // EM.cpp:167: only positions ij < LW1 take part; everything beyond reads the neutral row
#pragma unroll
        for (int m = 0; m < M; m++) y[m] = (p0 + (uint32_t)m < LW1 - t0) ? y[m] : Y;

        // U[m] after column j = prod_{j'<=j} s[j'][y(p-j+j')]  (EM.cpp:167-176); column 0 starts the chain
        float U[M];
        const float* sj = s_lds;
#pragma unroll
        for (int m = 0; m < M; m++) U[m] = sj[y[m]];
        for (uint32_t j = 1; j < W; j++) {
            sj += Ys;
            const float u0 = mul_wave_shr1(sj[y[0]], U[M - 1]);    // one v_mul_f32_dpp: lane 0 multiplies by 1
#pragma unroll
            for (int m = M - 1; m >= 1; m--) U[m] = U[m - 1] * sj[y[m]];
            U[0] = u0;
        }
        // slot p now holds the product of window t0 + p - (W - 1); this tile's are those with W - 1 <= p < W - 1 + n_own
        const float pos_i = q / (float)LW1;                  // EM.cpp:160

        if constexpr (PASS == PASS_Z) {
            double z = 0.0;
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t p = p0 + m;
                const bool owned = (p + 1u >= W) && (p + 1u - W < n_own);
                z += owned ? (double)(U[m] * pos_i) : 0.0;   // EM.cpp:180
            }
            z = wave_sum_f64(z);
            if (lane == 0) a.tile_z[g] = z;
        } else {
            const float invZ = a.rec_invz[t];
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t p = p0 + m;
                const bool owned = (p + 1u >= W) && (p + 1u - W < n_own);
                U[m] = owned ? U[m] * pos_i * invZ : 0.0f;   // EM.cpp:185-187
            }
            if (write_r) {                                   // EM::getR layout: r[L-W-i], i = t0 + p - (W - 1)
                float* ro = a.e.r_out + (a.e.sv.pos_off[seq] - a.e.r_base);
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const uint32_t p = p0 + m;
                    if ((p + 1u >= W) && (p + 1u - W < n_own)) ro[L - 1u - (t0 + p)] = U[m];
                }
            }
            if (accum) {
                // EM.cpp:236-242: position p, column j receives r of the window in slot p + (W - 1 - j), which lies inside
                // the tile for every window the tile owns
                unsigned long long F[M], nz[M], padm[M];
                uint32_t ya[M];                              // byte offset of (row y, private copy) inside a column
                const uint32_t copy = (uint32_t)lane & ((1u << logC) - 1u);
                const uint32_t cstride = (Ys << logC) * 8u;
#pragma unroll
                for (int m = 0; m < M; m++) {
                    F[m] = to_fixed40(U[m] * a.e.fix_scale);
                    nz[m] = __ballot(F[m] != 0ull);          // adding an exact 0 is a no-op: those lanes sit out
                    padm[m] = __ballot(y[m] != Y);           // positions beyond LW1 take no part (EM.cpp:236)
                    ya[m] = ((y[m] << logC) + copy) * 8u;
                }
                dense_count_walk<M>(W, lds_offset(n_lds) + (W - 1u) * cstride, cstride, ya, F, nz, padm, y, Y);
            }
        }
    }

    if constexpr (PASS == PASS_R) {
        if (!accum) return;
        // block epilogue: this block's table into the pass's accumulator
        lds_drain();
        __syncthreads();
        for (uint32_t o = threadIdx.x; o < W * Y; o += blockDim.x) {       // o = y*W + j: consecutive global cells
            const uint32_t yy = o / W, j = o - yy * W;
            unsigned long long acc = 0ull;
            for (uint32_t c = 0; c < (1u << logC); c++) acc += n_lds[(((size_t)j * Ys + yy) << logC) + c];
            if (acc) acc_add(a.e.acc + o, (long long)acc);
        }
    }
}

// a wave per sequence: lane l adds tiles l, l + 64, ... in ascending order, then the butterfly
__global__ void __launch_bounds__(256) k_em_tile_norm(EmTileArgs a) {
    if (a.e.stop != nullptr && *a.e.stop != 0u) return;
    const int lane = threadIdx.x & 63;
    const uint32_t waves_per_block = blockDim.x >> 6, total_waves = gridDim.x * waves_per_block;
    const float q = *a.e.q, one_minus_q = 1.0f - q;
    // rounded to the accumulator's units before they are summed (device_utils.h): a wave's sums are exact, whichever sequences it takes
    double llh_acc = 0.0, sumr_acc = 0.0;
    uint32_t seq_cnt = 0;
    for (uint32_t t = blockIdx.x * waves_per_block + (threadIdx.x >> 6); t < a.e.sv.count; t += total_waves) {
        const uint32_t seq = pick_sequence(a.e.sv, t);
        if (!takes_part(a.e, seq)) continue;
        const uint32_t g1 = a.tile_off[t + 1u];
        double z = 0.0;
        for (uint32_t g = a.tile_off[t] + (uint32_t)lane; g < g1; g += 64u) z += a.tile_z[g];
        z = wave_sum_f64(z);
        const float Z = one_minus_q + (float)z;              // EM.cpp:154,181
        const float invZ = 1.0f / Z;
        if (lane == 0) a.rec_invz[t] = invZ;
        llh_acc += stat_round_llh((double)logf(Z));          // EM.cpp:195
        sumr_acc += 1.0 - stat_round_sumr((double)one_minus_q / (double)Z);   // = sum_i r[i]  (EM.cpp:509-513)
        seq_cnt++;
    }
    if (a.e.acc && seq_cnt != 0u && lane < 3)
        acc_add_stat(a.e.acc, a.e.W * a.e.Y, (uint32_t)lane, lane == 0 ? llh_acc : (lane == 1 ? sumr_acc : (double)seq_cnt));
}

size_t tile_lds_bytes(uint32_t W, uint32_t Y, bool accum, uint32_t logC) {
    const size_t cells = (size_t)W * (Y + 1);
    return ((cells + 1) & ~size_t(1)) * sizeof(float) + (accum ? (cells << logC) * 8 : 0);
}

}  // namespace

bool em_tile_geometry(uint32_t W, uint32_t* tile_positions, uint32_t* stride) {
    const uint32_t st = tile_stride(W, kTilePositions);
    if (st < 16u) return false;
    if (tile_positions) *tile_positions = kTilePositions;
    if (stride) *stride = st;
    return true;
}

uint32_t em_tile_threads() { return (uint32_t)kTileThreads; }

int launch_em_tiles(const EmTileArgs& args, bool accum, bool write_r, uint32_t blocks, hipStream_t st) {
    if (blocks == kPrimeOnly) return prime_kernel(reinterpret_cast<const void*>(&k_em_tile<kTileM, kTileThreads, PASS_R>));
    if (args.n_tiles == 0) return BAMM_OK;
    EmTileArgs a = args;
    uint32_t stride = 0;
    if (tile_lds_bytes(a.e.W, a.e.Y, accum, 0) > 160 * 1024 || !em_tile_geometry(a.e.W, nullptr, &stride) || stride != a.stride || blocks == 0) {
        set_error("k_em_tile: W=%u, stride %u, tables of %zu bytes or %u blocks are outside the tiles' envelope", a.e.W, a.stride,
                  tile_lds_bytes(a.e.W, a.e.Y, accum, 0), blocks);
        return BAMM_ERR_ARG;
    }
    if (!(write_r && !accum && a.e.seq_end != 0u)) { a.e.seq_begin = 0u; a.e.seq_end = 0xffffffffu; }   // only getR names a range
    a.e.logC = 0;
    while (accum && a.e.logC < 4u && tile_lds_bytes(a.e.W, a.e.Y, true, a.e.logC + 1u) <= 160 * 1024) a.e.logC++;
    if (int rc = launch_kernel(&k_em_tile<kTileM, kTileThreads, PASS_Z>, blocks, (uint32_t)kTileThreads, tile_lds_bytes(a.e.W, a.e.Y, false, 0), st, a, 0, 0))
        return rc;
    BAMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_em_tile_norm, dim3(std::min((a.e.sv.count + 3u) / 4u, 1024u)), dim3(256), 0, st, a);
    BAMM_HIP(hipGetLastError());
    if (!accum && !write_r) return BAMM_OK;
    if (int rc = launch_kernel(&k_em_tile<kTileM, kTileThreads, PASS_R>, blocks, (uint32_t)kTileThreads, tile_lds_bytes(a.e.W, a.e.Y, accum, a.e.logC), st, a,
                               accum ? 1 : 0, write_r ? 1 : 0))
        return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace bamm
