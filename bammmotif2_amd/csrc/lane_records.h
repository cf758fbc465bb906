// Lane records of the mixed-row kernel (mixed_kernel.h): what a lane of k_em_mix needs from its sequence that depends on
// the sequence, the motif width and the row layout alone -- never on the model -- derived once per handle
// (lane_records.hip: k_mix_records, from plan_launches) instead of in every pass: an optimize() call runs some 34 passes
// over the same resident set, the loop is bound by vector instructions and registers, and the vector-memory path that
// brings the record is idle (4 % of the HBM bandwidth).
//
// One uint2 per (launch slot t of the bucket, lane), 512 bytes per sequence, read as one coalesced 8-byte load per lane:
//   x = the lane's stream window (it ends at the lane's last position) in bits 0..30 -- the rows of M <= 10 positions
//       take 2 (M - 1) + 12 <= 30 of them --, bit 31 = the lane IS a fix lane of this sequence (it rewrites its virtual
//       odds cell and reads its virtual count cell even when every field is Y: the wave's previous sequence left both
//       behind); the flag rides in the word whose every other use masks it out
//   y = the y of the fix lane's up to four columns, 7 bits each (Y = 64: none; bits 28..30 stay 0), bit 31 = something
//       is LEFT TO LOG: some column of the lane has a y and no resident bin (mix_fix_word: the layout's n1c leading
//       columns have one).  Both flags are the sign of their word: one compare each.
// The records follow the bucket's launch slots, not the sequence numbers: the load does not wait for the index list,
// and consecutive waves read consecutive memory.
#pragma once
#include "grouped_kernel.h"

namespace bamm {
namespace {

constexpr uint32_t kMixBj = 6u, kMixNe = 3u, kMixBv = kMixBj + kMixNe;   // virtual rows per wave: exceptions, edge
constexpr uint32_t kMixFixBit = 1u << 31;                    // lane record, word x: a fix lane (the sign: one compare tests it)
constexpr uint32_t kMixLogBit = 1u << 31;                    // lane record, word y: some column's sum goes to the log
constexpr uint32_t kMixNoY = 64u | (64u << 7) | (64u << 14) | (64u << 21);   // bit 6 (the value Y) of every 7-bit field

// per lane, fixed for the launch: bit 6 of every field of the y word whose column has a resident bin (the motif's first
// n1c columns) -- OR-ed into a sequence's codes it marks those columns "nothing to log"
__host__ __device__ inline uint32_t mix_resident_fill(uint32_t lane_col0, uint32_t n1c) {
    uint32_t fill = 0u;
    for (uint32_t c = 0; c < 4u; c++)
        if (lane_col0 + c < n1c) fill |= 64u << (7u * c);
    return fill;
}

// the first column of group t: B narrow groups of 3 columns, then the wide ones of 4
__host__ __device__ inline uint32_t mix_group_col0(uint32_t t, uint32_t B) { return t >= B ? 3u * B + 4u * (t - B) : 3u * t; }

// Word y of `lane`'s record for one sequence -- plain integer arithmetic, also compiled for the host
// (bamm_mix_fix_word: the CPU test of the encoding).  L: length; xw: first word of the sequence record (xlo | Bx << 12:
// the Bx group ends from position xlo on sit next to an exception); xfields: the y of the four positions that end at
// the lane's junction row, 7 bits each (xrec_fields: Y = before the sequence); sE: the stream window that ends at
// position L - W.  *fix: the lane rewrites its virtual cells for this sequence.
__host__ __device__ inline uint32_t mix_fix_word(uint32_t lane, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c, uint32_t L, uint32_t xw,
                                                 uint32_t xfields, uint32_t sE, bool* fix) {
    constexpr uint32_t Y = 64u;                              // K = 2
    const uint32_t LW1 = L - W + 1u;
    const uint32_t lane_b = lane / T, lane_t = lane - lane_b * T;                        // fix-lane roles: (row, group)
    const uint32_t lane_G = lane_t >= B ? 4u : 3u;
    const uint32_t Bx = (xw >> 12) & 0xfu;
    const uint32_t xlo = xw & 0xfffu;
    const uint32_t nE = L - LW1 < kMixNe ? L - LW1 : kMixNe;
    uint32_t yfix = kMixNoY;
    const bool fixJ = lane_b < Bx;
    const bool fixE = lane_b >= kMixBj && lane_b < kMixBj + nE;
    *fix = fixJ || fixE;
    if (!*fix) return yfix;
    const uint32_t pv = fixJ ? xlo + lane_b : LW1 + (lane_b - kMixBj);                 // the row's position
    for (uint32_t c = 0; c < 4u; c++) {
        uint32_t yc = Y;                                                               // the column's neutral entry
        if (c < lane_G) {
            const uint32_t pos = pv - (lane_G - 1u) + c;                               // wraps for positions before the sequence
            if (fixJ) {                                                                // record fields start at position xlo-3
                yc = (xfields >> (7u * c)) & 0x7fu;
            } else {
                yc = (sE >> (2u * ((LW1 - 1u - pos) & 15u))) & (Y - 1u);
            }
            if (pos >= LW1) yc = Y;                                                    // EM.cpp:167 (also pos < 0)
        }
        yfix = (yfix & ~(0x7fu << (7u * c))) | (yc << (7u * c));
    }
    // what the loop used to work out per sequence from a per-lane constant: is any field below Y once the resident
    // columns' fields are filled?
    if ((~(yfix | mix_resident_fill(mix_group_col0(lane_t, B), n1c)) & kMixNoY) != 0u) yfix |= kMixLogBit;
    return yfix;
}

// the 32-bit window of a sequence's 2-bit stream (wp: its first word) that ends at position pe; 0 before the sequence.  Words
// past the sequence's end only feed positions whose rows are overridden; the stream buffer carries 80 words of slack
// behind the last sequence (bamm_seqs_upload)
__device__ __forceinline__ uint32_t mix_stream_window(const uint32_t* wp, int pe) {
    if (pe < 0) return 0u;
    const uint32_t wi = (uint32_t)pe >> 4;
    const uint32_t lo = wp[wi], hi = wi ? wp[wi - 1u] : 0u;
    return __builtin_amdgcn_alignbit(hi, lo, 30u - 2u * ((uint32_t)pe & 15u));
}

// the record of `lane` for a sequence of length L with stream words wp and sequence record xr: M slots per lane, slot 0 of
// lane 0 at position `frame` (0, or mix_anchor_frame(B) for the start-anchored flavour), motif width W, T groups of which
// the first B are narrow (fix-lane roles: lane = row * T + group)
template <int M>
__device__ __forceinline__ uint2 mix_lane_record(const uint32_t* wp, uint32_t L, uint4 xr, int lane, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c,
                                                 int frame) {
    static_assert(2 * (M - 1) + 12 <= 31, "bit 31 of the window word is the fix-lane flag");
    const uint32_t LW1 = L - W + 1u;
    // ---- one 32-bit stream window per lane (it ends at the position of the lane's last slot); sE = the window ending at LW1-1
    uint32_t X = mix_stream_window(wp, lane * M + (M - 1) + frame);
    const uint32_t sE = mix_stream_window(wp, (int)LW1 - 1);

    // ---- virtual rows (one index for both tables): B group ends from xlo on next to an exception, the
    // positions LW1 .. LW1+2 whose groups are cut by the edge
    const uint32_t lane_b = (uint32_t)lane / T, lane_t = (uint32_t)lane - lane_b * T;     // fix-lane roles: (row, group)
    const uint32_t lane_G = lane_t >= B ? 4u : 3u;
    const uint32_t xfields = xrec_fields<7>(xr.y, xr.z, xr.w, lane_b + 4u - lane_G);     // the fields of the group's columns
    bool fix;
    const uint32_t yfix = mix_fix_word((uint32_t)lane, W, T, B, n1c, L, xr.x, xfields, sE, &fix);
    X = (X & ~kMixFixBit) | (fix ? kMixFixBit : 0u);
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
