// Lane records of the mixed-row kernel (mixed_kernel.h): what a lane of k_em_mix needs from its sequence that depends on
// the sequence, the motif width and the row layout alone -- never on the model -- derived once per handle
// (lane_records.hip: k_mix_records, from plan_launches) instead of in every pass: an optimize() call runs some 34 passes
// over the same resident set, the loop is bound by vector instructions and registers, and the vector-memory path that
// brings the record is idle (4 % of the HBM bandwidth).
//
// One uint2 per (launch slot t of the bucket, lane), 512 bytes per sequence, read as one coalesced 8-byte load per lane:
//   x = the lane's 32-bit stream window (it ends at the lane's last position)
//   y = the y of the fix lane's up to four columns, 7 bits each (Y = 64: none), bit 31 = the lane IS a fix lane of this
//       sequence (it rewrites its virtual odds cell and clears its virtual count cell even when every field is Y: the
//       wave's previous sequence left both behind)
// The records follow the bucket's launch slots, not the sequence numbers: the load does not wait for the index list,
// and consecutive waves read consecutive memory.
#pragma once
#include "grouped_kernel.h"

namespace bamm {
namespace {

constexpr uint32_t kMixBj = 6u, kMixNe = 3u, kMixBv = kMixBj + kMixNe;   // virtual rows per wave: exceptions, edge
constexpr uint32_t kMixFixBit = 1u << 31;                    // lane record, word y: a fix lane (the sign: one compare tests it)

// the record of `lane` for the sequence `cur` was fetched for: M positions per lane, motif width W, T groups of which the
// first B are narrow (fix-lane roles: lane = row * T + group)
template <int M>
__device__ __forceinline__ uint2 mix_lane_record(const RawSeqG<M>& cur, int lane, uint32_t W, uint32_t T, uint32_t B) {
    constexpr uint32_t Y = 64u;                              // K = 2
    const uint32_t L = __builtin_amdgcn_readfirstlane(cur.L);
    const uint32_t LW1 = L - W + 1u;
    const uint32_t p0 = (uint32_t)lane * M;

    // ---- one 32-bit stream window per lane (it ends at the lane's last position); sE = the window ending at LW1-1
    uint32_t X, sE;
    {
        constexpr int NSEL = RawSeqG<M>::NSEL;
        const uint32_t wi0 = p0 >> 4;
        const uint32_t pE = LW1 - 1u, lpE = pE / (uint32_t)M;
        const uint32_t pe = p0 + (uint32_t)(M - 1);
        const uint32_t sel = (pe >> 4) - wi0;
        uint32_t lo = cur.w[1], hi = cur.w[0];
#pragma unroll
        for (int c = 1; c < NSEL; c++) {
            lo = (sel == (uint32_t)c) ? cur.w[c + 1] : lo;
            hi = (sel == (uint32_t)c) ? cur.w[c] : hi;
        }
        X = __builtin_amdgcn_alignbit(hi, lo, 30u - 2u * (pe & 15u));
        sE = (uint32_t)__builtin_amdgcn_readlane((int)X, (int)lpE) >> (2u * ((uint32_t)(M - 1) - (pE - lpE * (uint32_t)M)));
    }

    // ---- virtual rows (one index for both tables): B group ends from xlo on next to an exception, the
    // positions LW1 .. LW1+2 whose groups are cut by the edge
    const uint32_t lane_b = (uint32_t)lane / T, lane_t = (uint32_t)lane - lane_b * T;     // fix-lane roles: (row, group)
    const uint32_t lane_G = lane_t >= B ? 4u : 3u;
    const uint32_t xw = __builtin_amdgcn_readfirstlane(cur.xr.x);
    const uint32_t Bx = (xw >> 12) & 0xfu;
    const uint32_t xlo = xw & 0xfffu;
    const uint32_t nE = min(kMixNe, L - LW1);
    uint32_t yfix = Y | (Y << 7) | (Y << 14) | (Y << 21);
    const bool fixJ = lane_b < Bx;
    const bool fixE = lane_b >= kMixBj && lane_b < kMixBj + nE;
    if (fixJ || fixE) {
        const uint32_t pv = fixJ ? xlo + lane_b : LW1 + (lane_b - kMixBj);         // the row's position
        const uint32_t xfields = xrec_fields<7>(cur.xr.y, cur.xr.z, cur.xr.w, lane_b + 4u - lane_G);     // the fields of the group's columns
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t yc = Y;                                                       // the column's neutral entry
            if ((uint32_t)c < lane_G) {
                const uint32_t pos = pv - (lane_G - 1u) + (uint32_t)c;           // wraps for positions before the sequence
                if (fixJ) {                                                        // record fields start at position xlo-3
                    yc = (xfields >> (7u * (uint32_t)c)) & 0x7fu;
                } else {
                    yc = (sE >> (2u * ((LW1 - 1u - pos) & 15u))) & (Y - 1u);
                }
                if (pos >= LW1) yc = Y;                                            // EM.cpp:167 (also pos < 0)
            }
            yfix = (yfix & ~(0x7fu << (7 * c))) | (yc << (7 * c));
        }
        yfix |= kMixFixBit;
    }
    return make_uint2(X, yfix);
}

// what k_em_mix fetches per sequence, one sequence ahead: the lane's record and, of the sequence record, the first word
// (xlo / Bx place the virtual rows among the lane's slots)
struct MixSeq {
    uint32_t seq, L, xw;
    uint2 rec;
    bool ok;
};

__device__ __forceinline__ MixSeq fetch_mix_seq(const SeqView& sv, const uint4* xrec, const uint2* lane_rec, uint32_t t, int lane) {
    MixSeq r;
    r.rec = lane_rec[(size_t)t * 64u + (uint32_t)lane];      // by launch slot: in flight before the index list answers
    r.seq = pick_sequence(sv, t);
    r.ok = !(sv.mask && !sv.mask[r.seq]);
    r.L = sv.len[r.seq];
    r.xw = reinterpret_cast<const uint32_t*>(xrec + r.seq)[0];
    return r;
}

}  // namespace
}  // namespace bamm
