// Tiles of a sequence beyond the length classes, shared by the scorer (scorer.hip) and the EM pass (em_tiles.hip): a
// sequence is cut into tiles of 64 * M positions that overlap by at least W - 1.  A tile starts on a multiple of the
// stride, the stride is a multiple of 16 (a tile starts on a word of the 2-bit stream) and at most 64 * M - (W - 1); a
// tile owns the windows that start in [t0, t0 + stride), the sequence's last tile up to L - W, and every window it owns
// lies wholly inside it.  A tile is found from its index: the launch carries the prefix sums of the bucket's tile counts,
// one entry per long sequence, and a wave searches them.
#pragma once
#include "device_utils.h"

namespace bamm {

// the largest multiple of 16 that leaves a tile of `tile_positions` an overlap of W - 1; 0 when W leaves none of at least 16
inline uint32_t tile_stride(uint32_t W, uint32_t tile_positions) {
    if (W == 0 || W > tile_positions) return 0u;
    return (tile_positions - (W - 1u)) & ~15u;
}

namespace {

// decode_positions' arithmetic (device_utils.h) for the positions t0 + lane*M + m of a sequence, t0 a multiple of 16:
// y[m] = kmer_[t0 + lane*M + m] mod Y (Sequence.cpp:35-41).  The word in front of the tile is read when t0 > 0 (a
// position's k-mer reaches up to K <= 10 bases back); it is zero at the start of a sequence.  Of the sequence's
// exceptions only those inside the tile are visited: one binary search for the first, then the run up to the tile's end
// -- never the whole list, which holds millions of entries for a chromosome.  (Kept apart from decode_positions so that
// the kernels built on that one compile to what they did.  Moving only the unpack loop that decode_positions and
// decode_raw share into one forceinline helper changed the instructions of 114 of the 163 kernels of kernels.hip --
// k_em_seq<64,false,false,512> 4035 -> 3526, k_m_slice<32,512> 10189 -> 10236, k_m_list<64,512> 256 -> 191 VGPRs --
// none of which has been timed: this unpack loop stays a copy until somebody measures those.)
template <int M>
__device__ __forceinline__ void decode_tile(const SeqView& sv, uint32_t seq, uint32_t L, uint32_t Y, uint32_t t0, int lane,
                                            uint32_t (&y)[M]) {
    constexpr int NSEL = (M + 14) / 16 + 1;  // candidate words per position
    const uint32_t* wp = sv.words + sv.word_off[seq] + (t0 >> 4);
    const uint32_t nw = ((L + 15u) >> 4) - (t0 >> 4);        // words from the tile's first to the sequence's last
    const uint32_t p0 = (uint32_t)lane * M;
    const uint32_t wi0 = p0 >> 4;
    uint32_t w[NSEL + 1];  // w[0] = word wi0-1, w[1] = word wi0, ...
    if (wi0 >= 1u) w[0] = (wi0 - 1u < nw) ? wp[wi0 - 1u] : 0u;
    else w[0] = t0 ? *(wp - 1) : 0u;
#pragma unroll
    for (int i = 0; i < NSEL; i++) w[i + 1] = (wi0 + i < nw) ? wp[wi0 + i] : 0u;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const uint32_t p = p0 + m;                           // (t0 + p) & 15 == p & 15
        const uint32_t sel = (p >> 4) - wi0;
        uint32_t lo = w[1], hi = w[0];
#pragma unroll
        for (int c = 1; c < NSEL; c++) {
            lo = (sel == (uint32_t)c) ? w[c + 1] : lo;
            hi = (sel == (uint32_t)c) ? w[c] : hi;
        }
        const uint32_t sh = 30u - 2u * (p & 15u);
        y[m] = __builtin_amdgcn_alignbit(hi, lo, sh) & (Y - 1u);
    }
    // positions whose k-mer the 2-bit stream cannot express (N randomisation, Sequence.cpp:38), rebased by t0
    const uint64_t e1 = sv.exc_off[seq + 1];
    uint64_t e = sv.exc_off[seq], hi = e1;
    while (e < hi) {                                         // first exception at or behind t0
        const uint64_t mid = e + ((hi - e) >> 1);
        if (sv.exc[mid].x < t0) e = mid + 1u; else hi = mid;
    }
    for (; e < e1; e++) {                                    // a tile inside a run of N: 64 * M of them (slow, accepted)
        const uint2 x = sv.exc[e];
        const uint32_t pos = __builtin_amdgcn_readfirstlane(x.x) - t0, val = __builtin_amdgcn_readfirstlane(x.y);
        if (pos >= 64u * (uint32_t)M) break;
        if constexpr (M >= 10 && M <= 32) {                  // one indexed register write in the owning lane (see decode_raw)
            const uint32_t owner = pos / (uint32_t)M, slot = pos % (uint32_t)M;
            if ((uint32_t)lane == owner) y[slot] = val;
        } else {
            const uint32_t mm = pos - p0;
#pragma unroll
            for (int m = 0; m < M; m++) y[m] = (mm == (uint32_t)m) ? val : y[m];
        }
    }
}

// the bucket slot whose tiles include tile g: the last t with tile_off[t] <= g (sequences without tiles are stepped over)
__device__ __forceinline__ uint32_t tile_owner(const uint32_t* tile_off, uint32_t count, uint32_t g) {
    uint32_t lo = 0, hi = count;                             // tile_off[lo] <= g < tile_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace
}  // namespace bamm
