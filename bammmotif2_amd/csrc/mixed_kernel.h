// gfx950 kernel of the fused EM pass at K = 2 with MIXED table rows: the motif's first B groups of 3 columns
// on 5-mer rows as in k_em_grp (grouped_kernel.h), its last A = W mod 3 groups of FOUR columns on 6-mer rows.
//
// Same computation as k_em_grp / k_em_seq: EM::EStep refinement/EM.cpp:149-196, EM::MStep EM.cpp:231-243, the
// sum over r of EM.cpp:509-513 -- file:line relative to /root/reference/src.
//
// Why: k_em_grp is bound by LDS instructions, T = ceil(W/3) gathers of group odds and T count adds per
// position, and a predicated ds_add_u64 costs 6.4-6.7 LDS cycles however few lanes take part (DESIGN.md
// section 4).  When W is not a multiple of 3 the last group of the uniform layout is mostly padding: W = 20 is
// 7 groups.  A 6-mer row holds four columns, so 20 = 3+3+3+3 + 4+4 is SIX groups: 42 adds instead of 49 per
// sequence of 7 positions per lane, and one b128 + one b64 gather per position instead of two b128.  An LDS-only
// loop of that mix (tools/lds_mix_bench.hip) runs in 165 ns per sequence and CU against 197 ns.  The price is
// LDS: a wide group takes 16 KB of odds and 32 KB of counts (4096 rows) against 4 + 8 KB, so at most two of
// them fit, the count tables are group-major (no padding cell), and the bins of the virtual rows only exist
// in the block epilogue (the fix lanes log their sums, as k_em_grp does at K = 3).
//
//   U_t(p) = U_{t-1}(p - G_t) * tab_t[row_t(p)]     narrow t < B: G_t = 3, row = kmer_[p] mod 4^5; wide: 4, 4^6
//   cnt_t[row_t(p)] += r(window whose group t ends at p)          (2^-40 fixed point, marginalised per block)
//
// Everything else is k_em_grp's: one wavefront per sequence, M positions per lane, per-wave virtual rows for the
// group ends next to an N exception (Sequence.cpp:38) and for those cut by the EM.cpp:167 edge -- one virtual
// row index serves both tables --, wave priorities by phase, the straight-line chain.
//
// What a lane needs of its sequence apart from the model -- its stream window, the fix lanes' column codes -- is not derived
// here: it is loaded, one record per lane, built once per handle (lane_records.h).
#pragma once
#include "lane_records.h"

namespace bamm {
namespace {

// one 7-bit field of a lane record's word y as ONE instruction whose result stays in its register for both of its uses (left to
// itself the compiler folds the extract into each use's own shift and mask: three instructions per column where two do)
__device__ __forceinline__ uint32_t field7(uint32_t w, int at) {
    uint32_t f;
    asm("v_bfe_u32 %0, %1, %2, 7" : "=v"(f) : "v"(w), "n"(at));
    return f;
}

// The rows of one slot in the two tables.  `special` is 0 for a slot that takes its rows from the stream window -- the 6-mer
// that ends at bit `at` of X and the 5-mer in its low ten bits -- and else the slot's row in the 6-mer table: the neutral row
// (4096) or a virtual one behind it; the 5-mer table has the same rows kMixRow5Bias = 4096 - 1024 lower.  A special row is above
// every stream row, so each table's row is one maximum instead of a compare and two selects; the 5-mer row comes out
// kMixRow5Bias too high for stream and special rows alike (the 6-mer's two high bits set: one OR of the shared extract), which
// the two base addresses it is scaled onto take back.
constexpr uint32_t kMixRow5Bias = 3072u;
__device__ __forceinline__ void mix_rows(uint32_t X, int at, uint32_t special, uint32_t& row5_biased, uint32_t& row6) {
    const uint32_t six = (X >> at) & 4095u;
    row6 = max(six, special);
    row5_biased = max(six | kMixRow5Bias, special);
}

// a 64-bit LDS cell by its byte address: a plain load, the compiler's to schedule and wait for
__device__ __forceinline__ unsigned long long lds_read_u64(uint32_t byte_addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(3))) unsigned long long*)(size_t)byte_addr;
#else
    return 0ull;
#endif
}

template <int OFF>
__device__ __forceinline__ void lds_add_u64_exec_big(uint32_t byte_addr, unsigned long long v, unsigned long long mask) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
    lds_add_u64_exec<OFF>(byte_addr, v, mask);
}

// ANCH, the start-anchored flavour (layout bit kMixAnchorBit): the same tables, rows, fix lanes and harvest in another frame.
// Above, a window's product travels up to the slot of its LAST position, so the slots must reach position L - 1 although no
// row from L - W + 3 on is anything but neutral.  Here the product of window s stays in the slot of its first quad entry's
// group end (position s + 2 - 3 pad) and the gathered odds come DOWN to it (grp_pull: by 3, 6, 9 slots for the quad's
// entries, 13 and 17 for the wide groups); the M-step's integers start there and move UP through the group ends (3, 3, 3, 4, 4;
// integer adds commute, so the first group's go first).  Slot lane * M + m holds position lane * M + m + 1 - 3 pad; M slots per
// lane reach every row that is not neutral when 64 M >= L - W + 3 + 3 pad, which for 200 bp on both strands (L = 401, W = 20)
// is 6 per lane instead of 7.  Same factors in the same order: a window's unnormalised product has the same bits in both
// flavours; Z sums them over another assignment of windows to lanes.
template <int M, int A, int NQ, bool ACCUM, bool WRITE_R, int THREADS, bool ANCH = false>
__global__ void __launch_bounds__(THREADS) k_em_mix(GrpKernelArgs ga) {
    static_assert(M >= 4 && 2 * (M - 1) + 12 <= 32, "a wide group within one lane's run, rows out of one stream window");
    static_assert(!ANCH || NQ == 1, "the start-anchored chain is written for one quad of narrow groups");
    static_assert(A == 1 || A == 2, "wide groups");
    constexpr uint32_t WAVES = THREADS / 64, V = WAVES * kMixBv;
    constexpr uint32_t R5N = 1024u, R5V0 = R5N + 1u, R5T = R5V0 + V;          // neutral row, first virtual row, rows
    constexpr uint32_t R6N = 4096u, R6V0 = R6N + 1u, R6T = R6V0 + V;
    constexpr uint32_t Y = 64u, Ys = 65u;                      // K = 2
    static_assert(Ys * 8u == kMixBinBytes, "a resident column's bins and its dump cell (mix_geometry)");
    if (ga.e.stop != nullptr && *ga.e.stop != 0u) return;    // optimize(): the stop rule fired in an earlier pass
    extern __shared__ __align__(16) unsigned char lds_raw[];
    BAMM_PHASE(0);
    const EmKernelArgs& a = ga.e;
    const GrpGeom& g = ga.g;
    const uint32_t W = a.W, T = g.T, B = g.mixB;             // T = B + A groups
    const uint32_t pad = 4u * NQ - B;                        // neutral slots in front of the first narrow group
    const uint32_t rs5 = g.rowstride;                        // floats per narrow odds row
    float* sg5 = reinterpret_cast<float*>(lds_raw + g.off_sg);                            // [R5T][rs5]
    float* sg6 = reinterpret_cast<float*>(lds_raw + g.off_sg6);                           // [R6T][A]
    // The single-column table [W][Y+1] serves the prologue (staged where the counts will be) and the fix lanes, who
    // read it from global memory through L2: four loads per sequence on the otherwise idle vector-memory path instead
    // of four LDS reads (0.875 -> 0.855 ms), and 5 KB of LDS for the bins below.
    const float* s1_stage = reinterpret_cast<const float*>(lds_raw + g.off_s1);            // prologue only: over the counts
    double* stat_lds = reinterpret_cast<double*>(lds_raw + g.off_stat);                   // [16][3], epilogue only: over sg5
    // count tables, group-major, groups stored LAST TO FIRST (the M-step walks them in that order and reaches the
    // next group through the add's immediate offset): cnt5[B-1-t][row], cnt6[T-1-t][row]
    unsigned long long* cnt5 = reinterpret_cast<unsigned long long*>(lds_raw + g.off_ng);
    unsigned long long* cnt6 = reinterpret_cast<unsigned long long*>(lds_raw + g.off_ng6);
    unsigned long long* n1 = reinterpret_cast<unsigned long long*>(lds_raw + g.off_n1);   // epilogue only: over sg6
    // bins [j][y] of the motif's first n1c columns, resident: what the fix lanes take out of their virtual count rows
    // for those columns is added here; only the other columns' sums go through the log (each logged entry costs a
    // store request in the loop and a read in the epilogue: all of them 0.875 ms, a third of them 0.814 ms).
    // Ys = Y + 1 cells per column: the code Y ("no bin": neutral, beyond the edge) lands in a dump cell nobody reads, so
    // a lane's add needs no compare of its code -- the sum a fix lane holds goes to the cell of every resident column's code
    unsigned long long* n1p = reinterpret_cast<unsigned long long*>(lds_raw + g.off_wave);
    const uint32_t n1c = ACCUM ? mix_resident_cols(g) : 0u;

    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total_waves = gridDim.x * WAVES;
    uint32_t t = blockIdx.x * WAVES + wave;
    MixSeq nxt{};
    if (t < a.sv.count) nxt = fetch_mix_seq(a.sv, ga.xrec, ga.lane_rec, t, lane);

    // ---- block prologue
    // fused update (update_kernel.h): the previous pass's model update runs here, in every block, from the all-reduced
    // accumulator -- its odds table lands where the prologue stages it anyway, and in this block's global copy for
    // the fix lanes; block 0 publishes the model.  Inside optimize() a fired stop rule ends the block here.
    [[maybe_unused]] float q_fused = 0.0f;
    {
        float* s1w = reinterpret_cast<float*>(lds_raw + g.off_s1);
        const float* s1 = s1_stage;
        bool staged = false;
        if constexpr (ACCUM) {
            if (ga.fused) {
                const UpdateOut uo = model_update_lds<false>(ga.upd, lds_raw + ga.upd_off, s1w, blockIdx.x == 0);
                if (uo.fired) {                              // block-uniform: the model is final, no pass follows
                    if (blockIdx.x == 0) { __syncthreads(); publish_odds(ga.upd, s1w, nullptr, true); }
                    return;
                }
                q_fused = uo.q;
                staged = true;
            }
        }
        BAMM_PHASE(1);                                       // the fused update is done
        if (!staged)
            for (uint32_t i = threadIdx.x; i < W * Ys; i += THREADS) s1w[i] = a.s[i];
        for (uint32_t i = threadIdx.x; i < (R5T - R5N) * rs5; i += THREADS) sg5[R5N * rs5 + i] = 1.0f;
        for (uint32_t i = threadIdx.x; i < (R6T - R6N) * A; i += THREADS) sg6[R6N * A + i] = 1.0f;
        __syncthreads();
        if constexpr (ACCUM)
            if (staged) publish_odds(ga.upd, s1w, ga.s_block + (size_t)blockIdx.x * (W * Ys), blockIdx.x == 0);
        for (uint32_t row = threadIdx.x; row < R5N; row += THREADS) {      // a group's 3 column odds in column order
            float* out = sg5 + row * rs5;
            for (uint32_t slot = 0; slot < pad; slot++) out[slot] = 1.0f;
            for (uint32_t slot = pad + B; slot < rs5; slot++) out[slot] = 1.0f;
            for (uint32_t tt = 0; tt < B; tt++) {
                float f = 1.0f;
#pragma unroll
                for (int c = 0; c < 3; c++) f *= s1[(3u * tt + c) * Ys + ((row >> (2 * (2 - c))) & 63u)];
                out[pad + tt] = f;
            }
        }
        for (uint32_t row = threadIdx.x; row < R6N; row += THREADS) {
#pragma unroll
            for (int w = 0; w < A; w++) {
                float f = 1.0f;
#pragma unroll
                for (int c = 0; c < 4; c++) f *= s1[(3u * B + 4u * w + c) * Ys + ((row >> (2 * (3 - c))) & 63u)];
                sg6[row * A + w] = f;
            }
        }
        __syncthreads();
        if (ACCUM) {                                         // the staging area becomes the count tables
            for (uint32_t i = threadIdx.x; i < B * R5T; i += THREADS) cnt5[i] = 0ull;
            for (uint32_t i = threadIdx.x; i < A * R6T; i += THREADS) cnt6[i] = 0ull;
            for (uint32_t i = threadIdx.x; i < n1c * Ys; i += THREADS) n1p[i] = 0ull;
            __syncthreads();
        }
    }

    BAMM_PHASE(2);                                           // tables built, counts zeroed
    if constexpr (ACCUM) {
        // in-kernel all-reduce: an earlier launch gave up waiting for a peer -- nothing is added any more (the prologue above
        // only read; block 0's publication of the model it computed from sums that never completed is as invalid as the handle,
        // whose next read fails with BAMM_ERR_COMM).  Checked HERE, not at the entry: the scalar round trip through the
        // kernel-argument segment is then behind the table build instead of in front of the first sequence fetch.
        const __attribute__((address_space(4))) GrpKernelArgs* kq =
            (const __attribute__((address_space(4))) GrpKernelArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kq));
        if (kq->peer.world > 1u && *kq->peer.err != 0u) return;
    }
    const float q = (ACCUM && ga.fused) ? q_fused : *a.q;
    const float one_minus_q = 1.0f - q;
    const uint32_t lane_b = (uint32_t)lane / T, lane_t = (uint32_t)lane - lane_b * T;     // fix-lane roles: (row, group)
    const bool lane_wide = lane_t >= B;
    const uint32_t lane_col0 = mix_group_col0(lane_t, B);
    const uint32_t vbase5 = R5V0 + wave * kMixBv, vbase6 = R6V0 + wave * kMixBv;
    const uint32_t sg6_base = lds_offset(sg6);
    const uint32_t sg5_base_biased = lds_offset(sg5) - kMixRow5Bias * (rs5 * 4u);   // for rows kMixRow5Bias too high (mix_rows; mod 2^32)

    // per lane, fixed for the launch: bit 6 (the value Y) of every 7-bit field of `yfix` whose column has a resident bin (OR-ed
    // into the sequence's codes it marks those columns "nothing to log"), shifted to where the log's code word has its
    // fields, next to the lane's group -- the code word is one shift-and-OR of the record's word
    const uint32_t resident_fill = mix_resident_fill(lane_col0, n1c);
    [[maybe_unused]] uint32_t code_fill = lane_t | (resident_fill << 3);
    asm volatile("" : "+v"(code_fill));                      // opaque: the compiler does not take the constant apart again (OR, then shift-and-OR)
    // a fourth column has a resident bin only in a wide group (a narrow lane's fourth field is always Y): with none
    // among the resident columns -- W = 20: 11 of them, all narrow -- the fourth predicated add is not issued at all
    [[maybe_unused]] const bool resident_wide = __builtin_amdgcn_readfirstlane((uint32_t)(n1c > 3u * B + 3u)) != 0u;
    // per column, fixed for the launch: the lanes whose column has a resident bin, as a mask for the scalar unit (opaque: kept
    // as the 64 bits it is, not turned back into a per-lane flag and compared again in every sequence)
    [[maybe_unused]] unsigned long long resident_lanes[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        resident_lanes[c] = __builtin_amdgcn_ballot_w64(((resident_fill >> (7 * c + 6)) & 1u) != 0u);
        asm volatile("" : "+s"(resident_lanes[c]));
    }
    // byte offset of the lane's first column in the single-column table [W][Y+1] and LDS address of its first column's
    // resident bins; the other columns follow at constant distances, which the instructions' offset fields take.  (A narrow
    // lane's fourth column is the next group's first: within the motif, a wide group follows; its field is always Y.)
    const uint32_t fix_s1 = __umul24(lane_col0, Ys * 4u);
    // the lane's virtual odds cell, in whichever table its group is: one address, one write per sequence for narrow and wide lanes alike
    float* const fix_odds = lane_wide ? sg6 + ((vbase6 + lane_b) * A + (lane_t - B)) : sg5 + (__umul24(vbase5 + lane_b, rs5) + pad + lane_t);
    [[maybe_unused]] const uint32_t fix_bin = lds_offset(n1p) + lane_col0 * (Ys * 8u);
    // the lane's virtual count cell, its own for the whole launch, and the total it held when the lane last looked: the cell is
    // never cleared (a ds_write_b64 per sequence); what one sequence's window added is the difference of two totals, exact
    // in 64-bit modular arithmetic.  The prologue zeroed the cell; the epilogue reads table rows only, never a virtual one.
    [[maybe_unused]] const uint32_t fix_cell = lds_offset(lane_wide ? cnt6 + (size_t)(T - 1u - lane_t) * R6T + vbase6 + lane_b
                                                                    : cnt5 + (size_t)(B - 1u - lane_t) * R5T + vbase5 + lane_b);
    [[maybe_unused]] unsigned long long fix_total = 0ull;
    double llh_acc = 0.0, sumr_acc = 0.0;
    uint32_t seq_cnt = 0, last_LW1 = 0;
    float pos_i = 0.0f;
    float pos_m[M];
    constexpr bool kCacheSpec = M <= 7 || THREADS < 1024;
    [[maybe_unused]] int spec[kCacheSpec ? M : 1];           // per slot: offset from the neutral row, -1 = a stream row
    [[maybe_unused]] uint32_t spec_LW1 = 0, spec_xw = 0xffffffffu;
#pragma unroll
    for (int m = 0; m < M; m++) pos_m[m] = 0.0f;
#pragma unroll
    for (int m = 0; m < (kCacheSpec ? M : 1); m++) spec[m] = 0;
    [[maybe_unused]] GrpLogEntry* my_log = nullptr;          // the fix lanes' non-zero sums (8-byte entries)
    [[maybe_unused]] uint32_t nlog = 0;
    if constexpr (ACCUM)
        my_log = reinterpret_cast<GrpLogEntry*>(ga.fix_log) + (size_t)(blockIdx.x * WAVES + wave) * ga.fix_log_cap;

    for (; t < a.sv.count; t += total_waves) {
        const MixSeq cur = nxt;
        // Pointers that are needed once per sequence are read again from the kernel-argument segment (scalar loads,
        // scalar cache) instead of living in SGPRs across the whole loop body: the body is 100 SGPRs over budget, and
        // what hipcc spills it parks in VGPR lanes and fetches back with v_readlane -- VALU instructions of a
        // VALU-bound loop (0.853 -> 0.842 ms per pass at 1M for the sequence set's pointers alone).
        const __attribute__((address_space(4))) GrpKernelArgs* kp =
            (const __attribute__((address_space(4))) GrpKernelArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));                         // opaque per iteration: the loads are not hoisted out of the loop
        if (t + total_waves < a.sv.count) {
            SeqView sv2;
            sv2.words = nullptr; sv2.word_off = nullptr; sv2.len = kp->e.sv.len; sv2.pos_off = nullptr;
            sv2.exc_off = nullptr; sv2.exc = nullptr; sv2.mask = kp->e.sv.mask; sv2.idx = kp->e.sv.idx; sv2.count = a.sv.count;
            nxt = fetch_mix_seq(sv2, kp->xrec, kp->lane_rec, t + total_waves, lane);
        }
        const uint32_t seq = cur.seq;
        if (WRITE_R && (seq < a.seq_begin || seq >= a.seq_end)) continue;
        if (!cur.ok) continue;
        __builtin_amdgcn_s_setprio(0);                       // decode, fix lanes
        const uint32_t L = __builtin_amdgcn_readfirstlane(cur.L);
        const uint32_t LW1 = L - W + 1u;
        // position of the lane's first slot (ANCH: may lie before the sequence -- the wrapped value is beyond every edge, a neutral row)
        const uint32_t p0 = ANCH ? (uint32_t)lane * M + (uint32_t)mix_anchor_frame(B) : (uint32_t)lane * M;

        // ---- the lane's record (lane_records.h): its 32-bit stream window (it ends at the lane's last position) and, for a
        // fix lane, the y of its up to four columns -- 7 bits each (Y = none), in ONE register: it lives until the virtual
        // count rows are read back after the M-step, and the kernel runs at the 128-VGPR limit of a 1024-thread block.
        // Virtual rows (one index for both tables): B group ends from xlo on next to an exception, the positions
        // LW1 .. LW1+2 whose groups are cut by the edge.  The fix lanes' reads of the single-column table are issued
        // first and waited for after the rows of all positions are decoded: the wave is not yet bound by the LDS pipe
        // here, the round trip is latency it would otherwise sit out.
        const uint32_t X = cur.rec.x, yfix = cur.rec.y;      // the flags stay in: every use extracts fields or shifts them out
        const bool fix = (int)X < 0;                         // kMixFixBit, the sign: one compare
        const uint32_t xw = __builtin_amdgcn_readfirstlane(cur.xw);
        const uint32_t Bx = (xw >> 12) & 0xfu;
        const uint32_t xlo = xw & 0xfffu;
        const uint32_t nE = min(kMixNe, L - LW1);
        float fs[4];                                         // a fix lane's column odds; no other lane reads them
        uint32_t yf[4];                                      // the columns' codes, extracted once for both uses
#pragma unroll
        for (int c = 0; c < 4; c++) yf[c] = field7(yfix, 7 * c);
        const char* const sfix_now = reinterpret_cast<const char*>((ACCUM && kp->fused) ? kp->s_block + (size_t)blockIdx.x * (W * Ys) : kp->e.s);
        if (fix) {
            // a 32-bit byte offset beside the uniform base: the load takes the base from SGPRs, the lane pays one extract
            // and one shift-and-add per column (no 64-bit address arithmetic)
#pragma unroll
            for (int c = 0; c < 4; c++)
                fs[c] = *reinterpret_cast<const float*>(sfix_now + ((yf[c] << 2) + fix_s1) + c * (int)(Ys * 4u));    // global, through L1 / L2
        }
        // Which slots do not take their row from the stream -- beyond the EM.cpp:167 edge (neutral row), a
        // virtual row -- depends on (L, the record's first word) only, and sets of one length with the strand
        // junction in one place repeat both: the slot's offset from the neutral row (the virtual rows follow it
        // in both tables; -1: a stream row) is kept until either changes.  2 bit-field extracts, 1 compare, 2 adds
        // and 2 selects per slot instead of 17 instructions.
        // (8 positions per lane at 1024 threads have no registers to spare for it: the offsets are recomputed)
        auto slot_offsets = [&](int (&o)[M]) {
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t k2 = p0 + m - xlo, k3 = p0 + m - LW1;
                o[m] = (p0 + m < LW1) ? 0 : (int)R6N;                                    // EM.cpp:167
                if (k2 < Bx) o[m] = (int)(R6N + 1u + wave * kMixBv + k2);
                if (k3 < nE) o[m] = (int)(R6N + 1u + wave * kMixBv + kMixBj + k3);
            }
        };
        static_assert(R6N - R5N == kMixRow5Bias && R5N == 1024u && R6N == 4096u, "mix_rows");
        uint32_t row5[M], row6[M];                           // row5: kMixRow5Bias too high (mix_rows)
        if constexpr (kCacheSpec) {
            if (LW1 != spec_LW1 || xw != spec_xw) {
                spec_LW1 = LW1; spec_xw = xw;
                slot_offsets(spec);
            }
#pragma unroll
            for (int m = 0; m < M; m++) mix_rows(X, 2 * (M - 1 - m), (uint32_t)spec[m], row5[m], row6[m]);
        } else {
            int o[M];
            slot_offsets(o);
#pragma unroll
            for (int m = 0; m < M; m++) mix_rows(X, 2 * (M - 1 - m), (uint32_t)o[m], row5[m], row6[m]);
        }
        if (fix) {
            const float f = ((fs[0] * fs[1]) * fs[2]) * fs[3];                         // column order; a neutral entry is 1.0f
            *fix_odds = f;
        }
        wave_lds_sync();

        // ---- E-step: narrow groups (straight-line over NQ quads, neutral slots in front), then the wide ones
        __builtin_amdgcn_s_setprio(2);
        float U[M];
        {
            uint32_t ra[M];
#pragma unroll
            for (int m = 0; m < M; m++) ra[m] = sg5_base_biased + __umul24(row5[m], rs5 * 4u);   // v_mad_u32_u24: full rate
            // the wide groups' odds are on their way while the narrow groups are chained (one round trip, not two)
            float2 pr[M];
#pragma unroll
            for (int m = 0; m < M; m++) {
#ifdef BAMM_PLAIN_LDS
                if constexpr (A == 2) pr[m] = lds_load<float2>(sg6_base + row6[m] * 8u);
                else pr[m].x = lds_load<float>(sg6_base + row6[m] * 4u);
#else
                if constexpr (A == 2) asm volatile("ds_read_b64 %0, %1" : "=v"(pr[m]) : "v"(sg6_base + row6[m] * 8u));
                else asm volatile("ds_read_b32 %0, %1" : "=v"(pr[m].x) : "v"(sg6_base + row6[m] * 4u));
#endif
            }
            if constexpr (ANCH) {
                // the product stays, the odds of the later groups come down to it: ((((x y) z) w) w0) w1 as above
                f32x4 sv[M];
#pragma unroll
                for (int m = 0; m < M; m++) sv[m] = lds_read_b128_off<0>(ra[m]);
                lds_wait(sv);                                // lgkmcnt(0): the wide groups' odds have landed as well
                lds_wait(pr);
                float f[M];
#pragma unroll
                for (int m = 0; m < M; m++) U[m] = sv[m].x;
#pragma unroll
                for (int m = 0; m < M; m++) f[m] = sv[m].y;
                grp_pull<M, 3>(U, f);
#pragma unroll
                for (int m = 0; m < M; m++) f[m] = sv[m].z;
                grp_pull<M, 6>(U, f);
#pragma unroll
                for (int m = 0; m < M; m++) f[m] = sv[m].w;
                grp_pull<M, 9>(U, f);
#pragma unroll
                for (int m = 0; m < M; m++) f[m] = pr[m].x;
                grp_pull<M, 13>(U, f);
                if constexpr (A == 2) {
#pragma unroll
                    for (int m = 0; m < M; m++) f[m] = pr[m].y;
                    grp_pull<M, 17>(U, f);
                }
            } else {
                grp_chain<M, 3, NQ>(ra, U);                      // waits with lgkmcnt(0): the reads above have landed as well
                lds_wait(pr);
                float w0[M];
#pragma unroll
                for (int m = 0; m < M; m++) w0[m] = pr[m].x;
                grp_step<M, 4>(U, w0);
                if constexpr (A == 2) {
                    float w1[M];
#pragma unroll
                    for (int m = 0; m < M; m++) w1[m] = pr[m].y;
                    grp_step<M, 4>(U, w1);
                }
            }
        }
        __builtin_amdgcn_s_setprio(1);                       // normalisation, statistics
        if (LW1 != last_LW1) {                           // EM.cpp:160; one IEEE division per distinct length
            pos_i = q / (float)LW1;
            last_LW1 = LW1;
            // q/LW1 for the slots that hold a window (it ends at p: p + 1 >= W and p < L), 0 for the others: kept
            // per distinct length, one multiply per slot instead of two compares, a select and a multiply
            // (ANCH: the slot holds the window that starts at lane * M + m - 1, whatever pad is)
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t p = p0 + m, s = (uint32_t)lane * M + m - 1u;
                pos_m[m] = (ANCH ? s < LW1 : (p + 1u >= W) && (p < L)) ? pos_i : 0.0f;
            }
        }
        float zpart = 0.0f;
#pragma unroll
        for (int m = 0; m < M; m++) {
            U[m] = mul_legacy(U[m], pos_m[m]);   // EM.cpp:180; v_mul_legacy: 0 * anything = 0
            zpart += U[m];
        }
        const float Z = one_minus_q + wave_sum(zpart);       // EM.cpp:154,181
        float invZ = __builtin_amdgcn_rcpf(Z);
        invZ = fmaf(fmaf(-Z, invZ, 1.0f), invZ, invZ);
        const float invZs = ACCUM ? invZ * (a.fix_scale * 256.0f) : invZ;    // 2^8: the fixed-point split below starts there
#pragma unroll
        for (int m = 0; m < M; m++) U[m] = U[m] * invZs;     // EM.cpp:185-187
        llh_acc += stat_round_llh((double)(__builtin_amdgcn_logf(Z) * 0.693147180559945309f));          // EM.cpp:195
        sumr_acc += stat_round_sumr((double)one_minus_q * (double)invZ);                 // 1 - sum_i r[i]  (EM.cpp:509-513)
        seq_cnt++;

        if (WRITE_R) {                                       // EM::getR layout: r[L-W-i], i = p-W+1
            float* ro = a.r_out + (a.sv.pos_off[seq] - a.r_base);
            if constexpr (ANCH) {                            // keyed by the window's start; the W - 1 entries behind the last window are 0
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const uint32_t s = (uint32_t)lane * M + m - 1u;
                    if (s < LW1) ro[LW1 - 1u - s] = U[m];
                }
                if ((uint32_t)lane < W - 1u) ro[LW1 + (uint32_t)lane] = 0.0f;
            } else {
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const uint32_t p = p0 + m;
                    if (p < L) ro[L - 1u - p] = U[m];
                }
            }
        }

        if (ACCUM) {
            // ---- M-step (EM.cpp:236-242): the adjoint chain, wide groups first (they are the motif's last)
            __builtin_amdgcn_s_setprio(3);
            unsigned long long F[M], nz[M];
            uint32_t rad6[M], rad5[M];
            const uint32_t c5 = lds_offset(cnt5), c6 = lds_offset(cnt6);
#pragma unroll
            for (int m = 0; m < M; m++) {
                F[m] = to_fixed40_pre(U[m]);
                nz[m] = __ballot(F[m] != 0ull);
                rad6[m] = c6 + row6[m] * 8u;
                rad5[m] = c5 - kMixRow5Bias * 8u + row5[m] * 8u;                 // (mod 2^32: the bias goes out again)
            }
            // F is a ring: logical slot m lives in F[(m + off) mod M]; a step of G moves the G slots that arrive
            // from the next lane in place (one DPP pair each) and their non-zero masks with them
            if constexpr (ANCH) {
                // forward: the integers start at the first quad entry's group end and move up to each later group's, the G
                // slots that arrive from the PREVIOUS lane in place; after d slots logical slot m lives in F[(m - d) mod M]
                static_for<4 * NQ + A>([&](auto ec) {
                    constexpr int e = decltype(ec)::value;
                    constexpr int d = e < 4 * NQ ? 3 * e : 3 * (4 * NQ - 1) + 4 * (e - 4 * NQ + 1);
                    constexpr int off = (M - d % M) % M;
                    if constexpr (e > 0) {
                        constexpr int G = e < 4 * NQ ? 3 : 4;
#pragma unroll
                        for (int c = 0; c < G; c++) {
                            const int idx = (c + off) % M;
                            F[idx] = wave_shr1_u64(F[idx]);
                            nz[idx] <<= 1;
                        }
                    }
                    if constexpr (e < 4 * NQ) {
                        constexpr int u = 4 * NQ - 1 - e;    // the groups are stored last to first
                        if ((uint32_t)u < B) {
#pragma unroll
                            for (int m = 0; m < M; m++)
                                lds_add_u64_exec_big<(int)(u * R5T * 8u)>(rad5[m], F[(m + off) % M], nz[(m + off) % M]);
                        }
                    } else {
                        constexpr int w = A - 1 - (e - 4 * NQ);
#pragma unroll
                        for (int m = 0; m < M; m++)
                            lds_add_u64_exec_big<(int)(w * R6T * 8u)>(rad6[m], F[(m + off) % M], nz[(m + off) % M]);
                    }
                });
            } else {
                static_for<A>([&](auto wc) {
                    constexpr int w = decltype(wc)::value;
                    constexpr int off = (4 * w) % M;
#pragma unroll
                    for (int m = 0; m < M; m++)
                        lds_add_u64_exec_big<(int)(w * R6T * 8u)>(rad6[m], F[(m + off) % M], nz[(m + off) % M]);
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const int idx = (c + off) % M;
                        F[idx] = wave_shl1_u64(F[idx]);
                        nz[idx] >>= 1;
                    }
                });
                static_for<4 * NQ>([&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    if ((uint32_t)u < B) {
                        constexpr int off = (4 * A + 3 * u) % M;
#pragma unroll
                        for (int m = 0; m < M; m++)
                            lds_add_u64_exec_big<(int)(u * R5T * 8u)>(rad5[m], F[(m + off) % M], nz[(m + off) % M]);
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const int idx = (c + off) % M;
                            F[idx] = wave_shl1_u64(F[idx]);
                            nz[idx] >>= 1;
                        }
                    }
                });
            }
            // ---- what the virtual count rows collected (one window per cell) goes to the log
            wave_lds_sync();
            unsigned long long acc = 0ull;
            if (fix) {
                const unsigned long long now = lds_read_u64(fix_cell);
                acc = now - fix_total;
                fix_total = now;
            }
            // code: group (3 bits), then the y of its up to four columns (7 bits each, >= Y = nothing to log: neutral,
            // beyond the edge, or a resident bin, which takes the sum here)
            // (fields of columns beyond the lane's group hold Y already: yfix is built that way)
            // a column with a resident bin: added here, not logged (a code Y: to the column's dump cell).  The lanes that add, as
            // masks: one compare's result and one fixed for the launch, combined by the scalar unit
            const unsigned long long has_acc = __builtin_amdgcn_ballot_w64(acc != 0ull);
            static_for<4>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                if (c == 3 && !resident_wide) return;                            // wave-uniform: no lane has a fourth resident column
                lds_add_u64_exec<c * (int)(Ys * 8u)>(fix_bin + (yf[c] << 3), acc, has_acc & resident_lanes[c]);
            });
            // what is left to log: fields still below Y once the resident columns' are filled -- whether there is any
            // (none also: a group wholly beyond the edge) is the sign of the record's word
            const uint32_t code = code_fill | (yfix << 3);       // (the flag, bit 31, falls off here)
            const bool to_log = acc != 0ull && (int)yfix < 0;    // kMixLogBit
            const unsigned long long nzm = has_acc & __builtin_amdgcn_ballot_w64((int)yfix < 0);
            if (to_log) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(nzm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nzm, 0u));
                GrpLogEntry* const log_now = reinterpret_cast<GrpLogEntry*>(kp->fix_log) + (size_t)(blockIdx.x * WAVES + wave) * kp->fix_log_cap;
                grp_log_store(log_now, nlog + rank, acc, code);
            }
            nlog += (uint32_t)__builtin_popcountll(nzm);
            wave_lds_sync();
        }
    }

    // ---- block epilogue (the statistics take the narrow odds table's place: every wave must be past its last sequence)
    lds_drain();
    BAMM_PHASE(3);                                           // wave 0 is through its sequences
    __syncthreads();
    BAMM_PHASE(4);                                           // ... and the block's slowest wave
    if (lane == 0) {
        stat_lds[wave * 3 + 0] = llh_acc;
        stat_lds[wave * 3 + 1] = (double)seq_cnt - sumr_acc;
        stat_lds[wave * 3 + 2] = (double)seq_cnt;
    }
    __syncthreads();
    if (a.acc == nullptr) return;                            // getR(): responsibilities only
    if constexpr (ACCUM) {
        // logged virtual-row sums -> single-column bins [j][y], which take the wide odds table's place
        for (uint32_t i = threadIdx.x; i < W * Y; i += THREADS) n1[i] = 0ull;
        __syncthreads();
        BAMM_PHASE(7);                                       // statistics parked, bins zeroed
        constexpr uint32_t NB = 8;
        for (uint32_t e0 = 0; e0 < nlog; e0 += 64u * NB) {
            unsigned long long acc[NB];
            uint32_t code[NB];
#pragma unroll
            for (uint32_t u = 0; u < NB; u++)
                grp_log_load(my_log, min(e0 + u * 64u + (uint32_t)lane, nlog - 1u), acc[u], code[u]);
#pragma unroll
            for (uint32_t u = 0; u < NB; u++) {
                if (e0 + u * 64u + (uint32_t)lane < nlog) {
                    const uint32_t tt = code[u] & 7u;
                    const uint32_t col0 = tt >= B ? 3u * B + 4u * (tt - B) : 3u * tt;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const uint32_t yc = (code[u] >> (3 + 7 * c)) & 127u;
                        if (yc < Y) atomicAdd(&n1[(col0 + (uint32_t)c) * Y + yc], acc[u]);
                    }
                }
            }
        }
        __syncthreads();
        BAMM_PHASE(5);                                       // the log is folded
        // Marginalisation in units of 16 table rows, every lane of every read instruction at work: a cell of a wide group
        // (64 rows carry its 3-mer) is four units on the four lanes of a quad, summed across the quad with two DPP adds; a
        // narrow cell is one unit; the wide units come first and fill whole rounds of the block, so no wave runs both
        // kinds (one item per cell made every wave issue 16 + 64 reads per round with 60 / 40 % of its lanes: the LDS
        // pipe's 2 us per round).  Every lane starts its sixteen rows elsewhere ((lane + lane / 4) mod 16): at equal
        // steps the lanes' rows differ in digits that do not reach the bank, rotated they spread over all of them.
        // Integer sums: any order gives the same total.  The totals go to the bins and from there out in the
        // accumulator's order (a scattered atomic instruction costs the L2 one operation per cache line it touches).
        constexpr uint32_t kWideUnits = 4u * (uint32_t)A * 4u * Y;           // [w][c][y][quarter]
        const uint32_t narrow_cells = 3u * B * Y;
        const uint32_t rot = ((uint32_t)lane + ((uint32_t)lane >> 2)) & 15u;
        for (uint32_t u = threadIdx.x; u < kWideUnits + narrow_cells; u += THREADS) {
            unsigned long long acc = 0ull;
            uint32_t j, yy;
            bool owner = true;
            unsigned long long v[16];
            if (u < kWideUnits) {                                               // quad-uniform: THREADS and kWideUnits are multiples of 4
                const uint32_t cell = u >> 2, quarter = u & 3u;
                yy = cell & (Y - 1u);
                const uint32_t wc = cell >> 6, w = wc >> 2, c = wc & 3u;
                j = 3u * B + 4u * w + c;
                const unsigned long long* tab = cnt6 + (size_t)((uint32_t)A - 1u - w) * R6T;
                const uint32_t lowd = 2u * (3u - c), lmask = (1u << lowd) - 1u;
#pragma unroll
                for (uint32_t rr = 0; rr < 16u; rr++) {
                    const uint32_t r = quarter * 16u + ((rr + rot) & 15u), h = r >> lowd, l = r & lmask;
                    v[rr] = tab[((((h << 6) | yy) << lowd) | l) & 4095u];
                }
#pragma unroll
                for (uint32_t rr = 0; rr < 16u; rr++) acc += v[rr];
                acc += quad_perm_u64<0xB1>(acc);                                 // lanes 1,0,3,2
                acc += quad_perm_u64<0x4E>(acc);                                 // lanes 2,3,0,1
                owner = quarter == 0u;
            } else {
                const uint32_t cell = u - kWideUnits;
                yy = cell & (Y - 1u);
                j = cell >> 6;
                const uint32_t tt = j / 3u, c = j - 3u * tt;
                const unsigned long long* tab = cnt5 + (size_t)(B - 1u - tt) * R5T;
                const uint32_t lowd = 2u * (2u - c), lmask = (1u << lowd) - 1u;
#pragma unroll
                for (uint32_t rr = 0; rr < 16u; rr++) {
                    const uint32_t r = (rr + rot) & 15u, h = r >> lowd, l = r & lmask;
                    v[rr] = tab[((((h << 6) | yy) << lowd) | l) & 1023u];
                }
#pragma unroll
                for (uint32_t rr = 0; rr < 16u; rr++) acc += v[rr];
            }
            if (owner) n1[j * Y + yy] += acc + (j < n1c ? n1p[j * Ys + yy] : 0ull);     // the cell's total, in its bin
        }
        BAMM_PHASE(13);
        __syncthreads();
        BAMM_PHASE(14);
        for (uint32_t o = threadIdx.x; o < W * Y; o += THREADS) {               // o = y*W + j: consecutive global cells
            const uint32_t yy = o / W, j = o - yy * W;
            const unsigned long long acc = n1[j * Y + yy];
            if (acc) acc_add(a.acc + o, (long long)acc);
        }
    }
    if (threadIdx.x < 3) {
        double acc = 0.0;
        for (uint32_t w = 0; w < WAVES; w++) acc += stat_lds[w * 3 + threadIdx.x];
        acc_add_stat(a.acc, W * Y, threadIdx.x, acc);
    }
    BAMM_PHASE(6);                                           // marginalised, atomics issued (thread 0's)
    if constexpr (ACCUM) {
        // in-kernel all-reduce: the last block to get here sums the GPUs' totals.  Its arguments are read from the
        // kernel-argument segment HERE (opaque pointer: the scalar loads cannot be hoisted above the sequence loop, where
        // every live SGPR is one more spill -- 44 -> 100 spilled SGPRs and +3 % on the pass when they were ordinary arguments)
        const __attribute__((address_space(4))) GrpKernelArgs* kq =
            (const __attribute__((address_space(4))) GrpKernelArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kq));
        if (kq->peer.world > 1u) {
            __syncthreads();                                 // the LDS is nobody's any more
            peer_allreduce_tail(&kq->peer, kq->e.acc, reinterpret_cast<uint32_t*>(lds_raw));
        }
    }
}

template <int M, int A, int NQ, int THREADS, bool ANCH>
int launch_mix_flavour(bool accum, bool write_r, const GrpKernelArgs& a, uint32_t blocks, hipStream_t st) {
    const size_t lds = a.g.lds_bytes;
    if (write_r) return launch_kernel(&k_em_mix<M, A, NQ, false, true, THREADS, ANCH>, blocks, THREADS, lds, st, a);
    if (accum) return launch_kernel(&k_em_mix<M, A, NQ, true, false, THREADS, ANCH>, blocks, THREADS, lds, st, a);
    return launch_kernel(&k_em_mix<M, A, NQ, false, false, THREADS, ANCH>, blocks, THREADS, lds, st, a);
}

template <int M, int A, int NQ, int THREADS>
int launch_mix_variant(bool accum, bool write_r, const GrpKernelArgs& a, uint32_t blocks, hipStream_t st) {
    return (a.g.layout & kMixAnchorBit) ? launch_mix_flavour<M, A, NQ, THREADS, true>(accum, write_r, a, blocks, st)
                                        : launch_mix_flavour<M, A, NQ, THREADS, false>(accum, write_r, a, blocks, st);
}

// the launcher of the translation unit for A wide groups (grouped_mix.hip: A = 2, grouped_mix1.hip: A = 1); arguments
// checked by launch_em_grp.  The planner keeps the narrow groups within one quad (mix_geometry: more of them lost to the
// uniform rows), so only NQ = 1 is instantiated.
template <int A>
int launch_mix(int mclass, bool accum, bool write_r, const GrpKernelArgs& a, uint32_t blocks, uint32_t threads, hipStream_t st) {
    if (threads != grp_max_threads(kMClasses[mclass]) || a.g.mixA != (uint32_t)A || a.g.Tq != 1u) {
        set_error("mixed-row kernel: bad launch (%u threads, A=%u, %u quads)", threads, a.g.mixA, a.g.Tq);
        return BAMM_ERR_ARG;
    }
    int rc = BAMM_ERR_UNSUPPORTED;
    switch (mclass) {
        case 3: rc = launch_mix_variant<4, A, 1, 1024>(accum, write_r, a, blocks, st); break;
        case 4: rc = launch_mix_variant<5, A, 1, 1024>(accum, write_r, a, blocks, st); break;
        case 5: rc = launch_mix_variant<6, A, 1, 1024>(accum, write_r, a, blocks, st); break;
        case 6: rc = launch_mix_variant<7, A, 1, 1024>(accum, write_r, a, blocks, st); break;
        case 7: rc = launch_mix_variant<8, A, 1, 1024>(accum, write_r, a, blocks, st); break;
        case 8: rc = launch_mix_variant<10, A, 1, 768>(accum, write_r, a, blocks, st); break;
        default: set_error("no mixed-row kernel for M class %d", mclass);
    }
    if (rc) return rc;
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

}  // namespace
}  // namespace bamm
