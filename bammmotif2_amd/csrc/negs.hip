// SeqGenerator's negative sampler on the device (/root/reference/src/seq_generator/SeqGenerator.cpp:63-348, restated on the
// host in bammmotif2_amd/host/fdr.cpp: kmer_frequency, rescale, draw).
//
// The reference draws m negatives per positive sequence, base by base, each base from the order-s conditionals of the whole
// set rescaled by the positive's own s-mer counts (:112-186), every base one rand() of libc's single stream (:222-341).  Which
// draw a base gets is known up front -- negative f of positive i consumes draws [d0[i] + f L, d0[i] + (f+1) L) -- so every
// negative can be sampled on its own once its generator state is known.  glibc's generator is linear (glibc_rand.h): the state
// after d draws is the seed state times t^d mod (t^31 - t^28 - 1), and t^d is the product of the host-made powers t^(2^b)
// over the set bits of d: a lane applies at most 48 of them to its 34-word state (each: 31 words of look-ahead, 34 x 31
// multiply-adds on registers), then steps through its L draws.
//   k_neg_counts   a wave per positive: its (k+1)-mer counts for k = 0..s from the resident set (the stream + the order-s
//                  exception list), added into the set's totals (:63-110; the host turns the totals into v and the bars)
//   k_neg_sample   a wave per positive: the counts again, lane 0 rescales the tables in the reference's float order into LDS
//                  (:112-186; --genericNeg: the set's own bars), then a lane per kept negative: state, draws, bases, 2-bit words
// Both for positives up to BAMM_MAX_SEQ_POSITIONS.  A longer positive's negatives are cut into segments, a lane per segment
// (k_neg_counts_long, k_neg_tables, k_neg_segments, k_neg_entry: further down); both kinds write the one output buffer.
// Float expressions are the host restatement's, in its order (-ffp-contract=off, IEEE division): the negatives are the
// reference's, base for base (tests/test_negs_gpu.py against host/fdr.cpp::sample_negatives, which the CPU suite pins to the
// reference's own sequences).
#include "negs.h"

namespace bamm {
namespace {

__device__ __forceinline__ uint32_t bgoff(uint32_t k) { return ((1u << (2 * (k + 1))) - 4u) / 3u; }

// (k+1)-mer counts of one sequence, k = 0..s, into the wave's LDS table (zeroed by the caller): SeqGenerator.cpp:63-110
// (words [w0, w1) of it: the counts are integers, so a long sequence may be cut between several waves)
__device__ __forceinline__ void seq_counts(const NegArgs& a, uint64_t n, uint32_t* cnt, int lane, uint32_t w0, uint32_t w1) {
    const uint32_t L = a.len[n], s = a.s;
    const uint32_t* w = a.words + a.word_off[n];
    const uint64_t e0 = a.exc_off[n], e1 = a.exc_off[n + 1];
    const uint32_t mask = (1u << (2 * (s + 1))) - 1u;
    for (uint32_t wi = w0 + lane; wi < w1; wi += 64) {
        const unsigned long long both = ((unsigned long long)(wi ? w[wi - 1] : 0u) << 32) | w[wi];
        uint64_t lo = e0, hi = e1;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (a.exc[mid].x < 16u * wi) lo = mid + 1; else hi = mid; }
        for (uint32_t i = 0; i < 16u && 16u * wi + i < L; i++) {
            const uint32_t j = 16u * wi + i;
            uint32_t y = (uint32_t)(both >> (30u - 2u * i)) & mask;
            if (lo < e1 && a.exc[lo].x == j) { y = a.exc[lo].y & mask; lo++; }
            for (uint32_t k = 0; k <= s; k++)
                if (j >= k) atomicAdd(&cnt[bgoff(k) + (y & ((1u << (2 * (k + 1))) - 1u))], 1u);
        }
    }
}

__global__ void __launch_bounds__(256) k_neg_counts(NegArgs a) {
    __shared__ uint32_t cnt_all[4][kNegTable];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* cnt = cnt_all[wv];
    const uint32_t tot = bgoff(a.s + 1);
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t n = (uint64_t)blockIdx.x * 4 + wv; n < a.n; n += waves) {
        if (a.len[n] > BAMM_MAX_SEQ_POSITIONS) continue;      // k_neg_counts_long's
        for (uint32_t i = lane; i < tot; i += 64) cnt[i] = 0u;
        __builtin_amdgcn_wave_barrier();
        seq_counts(a, n, cnt, lane, 0u, (a.len[n] + 15u) / 16u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t i = lane; i < tot; i += 64)
            if (cnt[i]) atomicAdd(&a.total_counts[i], (unsigned long long)cnt[i]);
        __builtin_amdgcn_wave_barrier();
    }
}

// the largest q in [0, n) with off[q] <= g; off[0] = 0 <= g < off[n]
__device__ __forceinline__ uint64_t owner_of(const uint64_t* off, uint64_t n, uint64_t g) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

// A wave per chunk of kNegCountWords words of a long positive: its counts into the positive's own table (the integers
// k_neg_sample gathers in LDS, whatever the cut) and into the set's totals.
__global__ void __launch_bounds__(256) k_neg_counts_long(NegArgs a, NegLongArgs la) {
    __shared__ uint32_t cnt_all[4][kNegTable];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* cnt = cnt_all[wv];
    const uint32_t tot = bgoff(a.s + 1);
    const uint64_t g = (uint64_t)blockIdx.x * 4 + wv;        // wave-uniform
    if (g >= la.n_chunks) return;
    const uint64_t li = owner_of(la.chunk_off, la.n_long, g), n = la.long_pos[li];
    const uint32_t nwords = (a.len[n] + 15u) / 16u;
    const uint64_t w0 = (g - la.chunk_off[li]) * kNegCountWords;
    if (w0 >= nwords) return;
    const uint32_t w1 = (uint32_t)(nwords - w0 > kNegCountWords ? w0 + kNegCountWords : nwords);
    for (uint32_t i = lane; i < tot; i += 64) cnt[i] = 0u;
    __builtin_amdgcn_wave_barrier();
    seq_counts(a, n, cnt, lane, (uint32_t)w0, w1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t i = lane; i < tot; i += 64)
        if (cnt[i]) {
            atomicAdd(&la.cnt[li * kNegTable + i], cnt[i]);
            atomicAdd(&a.total_counts[i], (unsigned long long)cnt[i]);
        }
}

// the state after the set bits of `d` were applied: r[0..33] = the next 34 outputs' history, oldest first
__device__ __forceinline__ void rand_jump(uint32_t (&r)[34], unsigned long long d, const uint32_t* pow2) {
    for (uint32_t b = 0; d != 0ull; b++, d >>= 1) {
        if (!(d & 1ull)) continue;
        const uint32_t* P = pow2 + 31u * b;                   // t^(2^b) mod (t^31 - t^28 - 1), uniform over the lanes
        uint32_t y[65];
#pragma unroll
        for (int k = 0; k < 34; k++) y[k] = r[k];
#pragma unroll
        for (int k = 34; k < 65; k++) y[k] = y[k - 3] + y[k - 31];
#pragma unroll
        for (int j = 0; j < 34; j++) {
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 31; c++) v += P[c] * y[c + j];
            r[j] = v;
        }
    }
}

// The bars of one positive from its counts `cnt` and the set's conditionals: SeqGenerator.cpp:112-186, written for s = 2, the
// host's float order.  One lane; k_neg_sample's tables are in LDS, k_neg_tables' in global memory.
__device__ __forceinline__ void rescale_bars(const NegArgs& a, const uint32_t* cnt, uint32_t L, float* bar) {
    const float* v = a.v;
    const float A0 = a.A[0], A1 = a.A[1], A2 = a.A[2];
    float vs[kNegTable];
    float sum = 0.f;
    for (uint32_t y = 0; y < 4; y++) { vs[y] = v[y]; sum += vs[y]; bar[y] = sum; }
    {
        const uint32_t o1 = 4, o0 = 0;
        for (uint32_t y = 0; y < 16; y++) {
            const uint32_t y2 = y % 4;
            vs[o1 + y] = v[o1 + y] * ((float)cnt[o1 + y] + A0 * v[o0 + y2]) / v[o0 + y2] / ((float)L + A0);
        }
        float norm[4] = {0.f, 0.f, 0.f, 0.f};
        for (uint32_t y = 0; y < 16; y++) {
            const uint32_t yk = y / 4;
            vs[o1 + y] = ((float)cnt[o1 + y] + A1 * vs[o1 + y]) / ((float)cnt[o0 + yk] + A1);
            norm[yk] += vs[o1 + y];
        }
        for (uint32_t y = 0; y < 16; y++) vs[o1 + y] /= norm[y / 4];
        for (uint32_t y = 0; y < 16; y++) {
            if (y % 4 == 0) sum = 0.0f;
            sum += vs[o1 + y];
            bar[o1 + y] = sum;
        }
    }
    {
        const uint32_t o2 = 20, o1 = 4;
        for (uint32_t y = 0; y < 64; y++) {
            const uint32_t y2 = y % 16, yk = y / 4;
            vs[o2 + y] = ((float)cnt[o2 + y] + A2 * vs[o1 + y2]) / ((float)cnt[o1 + yk] + A2);
            if (y % 4 == 0) sum = 0.0f;
            sum += vs[o2 + y];
            bar[o2 + y] = sum;
        }
    }
}

__global__ void __launch_bounds__(256) k_neg_sample(NegArgs a) {
    __shared__ uint32_t cnt_all[4][kNegTable];
    __shared__ float bar_all[4][kNegTable];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* cnt = cnt_all[wv];
    float* bar = bar_all[wv];
    const uint32_t s = a.s, tot = bgoff(s + 1);
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    const uint64_t total_neg = a.n * a.m_fold;
    for (uint64_t n = (uint64_t)blockIdx.x * 4 + wv; n < a.n; n += waves) {
        const uint32_t L = a.len[n];
        if (L > BAMM_MAX_SEQ_POSITIONS) continue;             // segment by segment: k_neg_segments (wave-uniform)
        if (a.generic) {
            for (uint32_t i = lane; i < tot; i += 64) bar[i] = a.bar[i];
        } else {
            for (uint32_t i = lane; i < tot; i += 64) cnt[i] = 0u;
            __builtin_amdgcn_wave_barrier();
            seq_counts(a, n, cnt, lane, 0u, (L + 15u) / 16u);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane == 0) rescale_bars(a, cnt, L, bar);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // this positive's kept negatives, a lane each
        const uint64_t first = n * a.m_fold;
        const uint32_t nwords = (L + 15u) / 16u;
        uint64_t kept_before = 0;                             // kept negatives of this positive in front of the current round
        for (uint64_t f0 = 0; f0 < a.m_fold; f0 += 64) {
            const uint64_t f = f0 + (uint64_t)lane, idx = first + f;
            const bool mine = f < a.m_fold && (a.keep_stride <= 1 || (idx % a.keep_stride == 0 && idx + a.keep_stride <= total_neg));
            const unsigned long long km = __ballot(mine);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
            if (mine) {
                uint32_t r[34];
#pragma unroll
                for (int k = 0; k < 34; k++) r[k] = a.seed_state[k];
                rand_jump(r, a.draw0[n] + f * (uint64_t)L, a.pow2);
                uint32_t* out = a.out_words + a.out_word_off[n] + (kept_before + rank) * (uint64_t)nwords;
                uint32_t word = 0, ctx = 0, pos = 0, bad = 0;
                const uint32_t ctx_mask = (1u << (2 * s)) - 1u;
                uint32_t seq_first[kNegMaxOrder];             // the first s bases (0-based codes) for the lower-order contexts
                while (pos < L) {
#pragma unroll
                    for (int j = 0; j < 34; j++) {
                        if (pos < L) {
                            const uint32_t v = r[(j + 3) % 34] + r[(j + 31) % 34];
                            r[j] = v;
                            const float random = (float)(int)(v >> 1) / 2147483647.0f;       // rand() / RAND_MAX in floats (:223)
                            uint32_t base;                    // 0..3
                            if (pos >= s) {
                                const float* b4 = bar + bgoff(s) + ctx * 4u;
                                base = (random > b4[0]) + (random > b4[1]) + (random > b4[2]);
                            } else if (pos == 0) {
                                base = random <= bar[0] ? 0u : (random <= bar[1] ? 1u : (random <= bar[2] ? 2u : (random <= bar[3] ? 3u : 4u)));
                                if (base == 4u) { bad = 1u; base = 0u; }      // the reference leaves seq[0] unset there (rand() == RAND_MAX)
                            } else {
                                uint32_t yk = 0;
                                for (uint32_t k = pos; k > 0; k--) yk += seq_first[pos - k] << (2 * k);
                                const float* b4 = bar + bgoff(pos) + yk;
                                base = (random > b4[0]) + (random > b4[1]) + (random > b4[2]);
                            }
                            if (pos < s) {
#pragma unroll
                                for (uint32_t q = 0; q < kNegMaxOrder; q++) if (q == pos) seq_first[q] = base;
                            }
                            ctx = ((ctx << 2) | base) & ctx_mask;
                            word |= base << (30u - 2u * (pos & 15u));
                            if ((pos & 15u) == 15u || pos + 1u == L) { out[pos >> 4] = word; word = 0; }
                            pos++;
                        }
                    }
                }
                if (bad) atomicAdd(a.bad, 1u);
            }
            kept_before += (uint64_t)__builtin_popcountll(km);
        }
        __builtin_amdgcn_wave_barrier();                      // the tables are rewritten for the next positive
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Positives beyond BAMM_MAX_SEQ_POSITIONS, segment by segment.  From position s = 2 on a base is a function of the two bases
// before it (16 contexts) and of its own draw, which is known up front: position i is a map context -> context, a segment
// of S positions the composition of its positions' maps, 16 x 4 bits.  Composition is associative and reorders nothing
// in floating point -- every compare is the host's `random > bar` on the same floats -- so the negatives stay the reference's:
//   k_neg_tables          a lane per long positive: its bars (rescale_bars; --genericNeg: the set's) into a global table
//   k_neg_segments<false> a lane per (kept negative, segment): the generator at the segment's first draw (rand_jump, kept
//                         for the second walk), then the segment for all 16 entry contexts at once -- one chain as soon as
//                         all 16 agree; segment 0 walks its one real chain -- and leaves the packed map
//   k_neg_entry           a wave per kept negative: a scan of its maps, every segment's entry context
//   k_neg_segments<true>  the same lanes walk their segment from its entry context and write its words of the 2-bit stream
// No block waits for another: the four are launches of their own.  Every loop ends at the record's length or the segment count.

constexpr unsigned long long kMapIdentity = 0xFEDCBA9876543210ull;   // nibble e = the context entry context e leaves in

__global__ void __launch_bounds__(256) k_neg_tables(NegArgs a, NegLongArgs la) {
    const uint64_t li = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= la.n_long) return;
    float* bar = la.bar + li * kNegTable;
    if (a.generic) { for (uint32_t i = 0; i < kNegTable; i++) bar[i] = a.bar[i]; }
    else rescale_bars(a, la.cnt + li * kNegTable, a.len[la.long_pos[li]], bar);
}

// the base (0..3) context `ctx` draws at `random`: the bars of order 2 below it, counted (neg_sampler.h: next_base)
__device__ __forceinline__ uint32_t next_base(const float* bar2, uint32_t ctx, float random) {
    const float4 b = *reinterpret_cast<const float4*>(bar2 + ctx * 4u);       // 16-byte aligned: rows of 84 floats, order 2 at 20
    return (uint32_t)(random > b.x) + (uint32_t)(random > b.y) + (uint32_t)(random > b.z);
}

// one position applied to all 16 chains of a map
__device__ __forceinline__ unsigned long long map_step(unsigned long long map, const float* bar2, float random) {
    uint32_t nb = 0;                                          // the base every context draws here, 2 bits each
#pragma unroll 4
    for (uint32_t c = 0; c < 16; c++) nb |= next_base(bar2, c, random) << (2u * c);
    unsigned long long out = 0;
#pragma unroll 4
    for (uint32_t e = 0; e < 16; e++) {
        const uint32_t c = (uint32_t)(map >> (4u * e)) & 15u;
        out |= (unsigned long long)(((c << 2) | ((nb >> (2u * c)) & 3u)) & 15u) << (4u * e);
    }
    return out;
}

template <bool kBases>
__global__ void __launch_bounds__(256) k_neg_segments(NegArgs a, NegLongArgs la) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= la.n_seg) return;
    const uint64_t q = owner_of(la.seg_off, la.n_rec, g);
    const NegLongRec rc = la.rec[q];
    const uint32_t L = rc.L, S = la.S;
    const uint64_t first_pos = (g - la.seg_off[q]) * S;
    if (first_pos >= L) { if (!kBases) la.map[g] = kMapIdentity; return; }   // no such segment in a record of L positions
    const uint32_t p0 = (uint32_t)first_pos, p1 = L - p0 > S ? p0 + S : L;
    const float* bar = la.bar + (uint64_t)rc.tab * kNegTable;
    const float* bar2 = bar + bgoff(kNegMaxOrder);
    uint32_t r[34];
    if (kBases) {
#pragma unroll
        for (int k = 0; k < 34; k++) r[k] = la.state[(uint64_t)k * la.n_seg + g];
    } else {
#pragma unroll
        for (int k = 0; k < 34; k++) r[k] = a.seed_state[k];
        rand_jump(r, rc.draw_start + p0, a.pow2);
#pragma unroll
        for (int k = 0; k < 34; k++) la.state[(uint64_t)k * la.n_seg + g] = r[k];
    }
    uint32_t* out = a.out_words + rc.out_off;
    unsigned long long map = kMapIdentity;
    bool one = kBases || p0 == 0;                             // one chain: its context is known
    uint32_t ctx = kBases ? la.entry[g] : 0u;
    uint32_t word = 0, base0 = 0, bad = 0, pos = p0;
    while (pos < p1) {
#pragma unroll
        for (int k = 0; k < 34; k++) {
            if (pos < p1) {
                const uint32_t v = r[(k + 3) % 34] + r[(k + 31) % 34];
                r[k] = v;
                const float random = (float)(int)(v >> 1) / 2147483647.0f;           // rand() / RAND_MAX in floats (:223)
                uint32_t base = 0;
                if (k < (int)kNegMaxOrder && pos < kNegMaxOrder) {                    // the record's first bases: segment 0, as k_neg_sample
                    if (pos == 0) {
                        base = random <= bar[0] ? 0u : (random <= bar[1] ? 1u : (random <= bar[2] ? 2u : (random <= bar[3] ? 3u : 4u)));
                        if (base == 4u) { bad = 1u; base = 0u; }                      // the reference leaves seq[0] unset there
                        base0 = base;
                    } else {
                        const float* b4 = bar + bgoff(1) + (base0 << 2);
                        base = (uint32_t)(random > b4[0]) + (uint32_t)(random > b4[1]) + (uint32_t)(random > b4[2]);
                    }
                    ctx = ((ctx << 2) | base) & 15u;
                } else if (kBases || one) {
                    base = next_base(bar2, ctx, random);
                    ctx = ((ctx << 2) | base) & 15u;
                } else {
                    map = map_step(map, bar2, random);
                    if (map == (map & 15ull) * 0x1111111111111111ull) { one = true; ctx = (uint32_t)map & 15u; }   // chains that met stay together
                }
                if (kBases) {
                    word |= base << (30u - 2u * (pos & 15u));
                    if ((pos & 15u) == 15u || pos + 1u == L) { out[pos >> 4] = word; word = 0; }
                }
                pos++;
            }
        }
    }
    if (!kBases) la.map[g] = one ? (unsigned long long)ctx * 0x1111111111111111ull : map;
    else if (bad) atomicAdd(a.bad, 1u);
}

// `then` after `first`
__device__ __forceinline__ unsigned long long map_compose(unsigned long long first, unsigned long long then) {
    unsigned long long out = 0;
#pragma unroll
    for (uint32_t e = 0; e < 16; e++) out |= ((then >> (4u * ((uint32_t)(first >> (4u * e)) & 15u))) & 15ull) << (4u * e);
    return out;
}

__global__ void __launch_bounds__(256) k_neg_entry(NegLongArgs la) {
    const int lane = threadIdx.x & 63;
    const uint64_t q = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);         // wave-uniform
    if (q >= la.n_rec) return;
    const uint64_t s0 = la.seg_off[q], nseg = la.seg_off[q + 1] - s0;
    uint32_t carry = 0;                                       // the context behind the segments in front of this round (segment 0's map is constant)
    for (uint64_t j0 = 0; j0 < nseg; j0 += 64) {
        const uint64_t j = j0 + (uint64_t)lane;
        unsigned long long m = j < nseg ? la.map[s0 + j] : kMapIdentity;
        for (int d = 1; d < 64; d <<= 1) {                    // inclusive scan: lane l holds segments j0 .. j0 + l composed
            const unsigned long long before = __shfl_up(m, d, 64);
            if (lane >= d) m = map_compose(before, m);
        }
        const unsigned long long prev = __shfl_up(m, 1, 64);
        if (j < nseg) la.entry[s0 + j] = (uint8_t)(lane == 0 ? carry : (uint32_t)(prev >> (4u * carry)) & 15u);
        carry = (uint32_t)(__shfl(m, 63, 64) >> (4u * carry)) & 15u;
    }
}

}  // namespace

int launch_neg_counts(const NegArgs& a, hipStream_t st) {
    if (a.n == 0) return BAMM_OK;
    const uint64_t want = (a.n + 3) / 4;
    hipLaunchKernelGGL(k_neg_counts, dim3((uint32_t)(want > 4096 ? 4096 : want)), dim3(256), 0, st, a);
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_neg_sample(const NegArgs& a, hipStream_t st) {
    if (a.n == 0) return BAMM_OK;
    const uint64_t want = (a.n + 3) / 4;
    hipLaunchKernelGGL(k_neg_sample, dim3((uint32_t)(want > 65535 ? 65535 : want)), dim3(256), 0, st, a);
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

namespace {
// blocks of a launch with one item per `per_block`; a grid beyond 2^31 - 1 blocks is refused
int blocks_for(uint64_t items, uint32_t per_block, uint32_t* blocks) {
    const uint64_t want = (items + per_block - 1) / per_block;
    if (want > 0x7fffffffull) { set_error("the negative sampler's segments exceed one launch (%llu items)", (unsigned long long)items); return BAMM_ERR_ARG; }
    *blocks = (uint32_t)want;
    return BAMM_OK;
}
}  // namespace

int launch_neg_counts_long(const NegArgs& a, const NegLongArgs& la, hipStream_t st) {
    if (la.n_chunks == 0) return BAMM_OK;
    uint32_t blocks = 0;
    if (int rc = blocks_for(la.n_chunks, 4, &blocks)) return rc;
    hipLaunchKernelGGL(k_neg_counts_long, dim3(blocks), dim3(256), 0, st, a, la);
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}

int launch_neg_sample_long(const NegArgs& a, const NegLongArgs& la, hipStream_t st) {
    if (la.n_long == 0 || la.n_seg == 0) return BAMM_OK;
    uint32_t b_tab = 0, b_seg = 0, b_rec = 0;
    int rc;
    if ((rc = blocks_for(la.n_long, 256, &b_tab)) || (rc = blocks_for(la.n_seg, 256, &b_seg)) || (rc = blocks_for(la.n_rec, 4, &b_rec))) return rc;
    hipLaunchKernelGGL(k_neg_tables, dim3(b_tab), dim3(256), 0, st, a, la);
    hipLaunchKernelGGL(k_neg_segments<false>, dim3(b_seg), dim3(256), 0, st, a, la);
    hipLaunchKernelGGL(k_neg_entry, dim3(b_rec), dim3(256), 0, st, la);
    hipLaunchKernelGGL(k_neg_segments<true>, dim3(b_seg), dim3(256), 0, st, a, la);
    BAMM_HIP(hipGetLastError());
    return BAMM_OK;
}
}  // namespace bamm
