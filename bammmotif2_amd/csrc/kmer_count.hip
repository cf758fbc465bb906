// Exact w-mer counts of a resident set, w = 6..8: the histogram the de novo seeder ranks (host/seeder.cpp).
//
// Every window of w consecutive positions of a record that touches neither an unknown base nor the strand separator adds 1
// to the cell of its w bases read as a base-4 number, oldest base most significant.  With both strands the reverse
// complement of a forward window IS a window of the record, behind the separator, so one walk over the record's positions
// counts both and a reverse-palindromic window adds 2 to its own cell; nothing is read twice.  The bases the packer drew for
// unknown positions are in the stream like any other: the set's list of unknown forward positions (packed_set.h) says
// which windows to skip -- those over a listed position z, and with both strands those over its copy 2 L0 - z behind the
// separator at L0.
//
// Work: a wave per record, a lane per 32-bit word (16 positions) of it, 64 words at a time.  A lane owns the windows that END
// in its word and takes the w - 1 positions before it from the previous word, so nothing is shared between lanes, and a
// record longer than `seg_words` words is simply a list of (record, first word) segments: the w - 1 positions of overlap
// between two segments are the previous word a lane reads anyway.  Per lane: the two words as one 64-bit register (the window
// ending at a position is a shift and a mask of it), and a 32-bit mask of the positions it must not touch -- before the
// record, behind it, the separator, the unknown positions and their copies (two binary searches in the record's list; most
// records have none and skip them).  The next record's header and first words are fetched before the current one is counted.
//
// Table: privatised per workgroup in LDS, 32-bit cells, added with ds_add_u32 (no return), flushed into the 64-bit table in
// global memory with one vector atomic per non-zero cell.  4^6 and 4^7 cells fit (16 / 64 KiB).  4^8 cells do not (256 KiB
// against 160): the launch then has two workgroups per block index, (b, 0) and (b, 1), which walk the same records and keep
// the half of the table whose leading base is A/C resp. G/T (128 KiB each).  Both halves decode every window, each adds
// half of them: the adds' lanes are not doubled, the instructions are (each half issues every add with about half its lanes),
// and so are the decode and the read of the stream (2 bits per position).  The counters (profiles/kmer_counts.txt) show the
// vector decode as the binding resource, not the LDS adds: w = 8 costs 1.67 x the time of w = 7 per position.
//
// No cell wraps: the waves of a workgroup work in rounds of kEntriesPerRound entries each; after a round the workgroup adds an
// upper bound of the windows it added (16 per word) to a running total and flushes the table when the total has reached
// `flush_windows` (at most 2^31).  A round adds fewer than 16 waves x 8 entries x 2^20 positions = 2^27 windows, so no cell
// exceeds 2^31 + 2^27 between two flushes.
//
// Dyads (k_kmer_counts_gapped, w = 6 or 8): a window of span S = w + g <= 16 whose first and last h = w / 2 positions form the
// cell and whose g positions between them only have to be known.  The same walk, with the grid's z axis over the gaps asked
// for: workgroup (b, p, z) serves gap gap_lo + z alone and adds into table z, so the bound of 16 windows per word and
// workgroup, and with it the flush rule, stands as it is.  A lane's own word is bits 16..31 of its 32 positions, so a
// window that ends there (i >= 16) starts at bit i - S + 1 >= 1: its two halves are two shifts of the same 64-bit
// register and its validity a run of S bits of the same mask, and the S - 1 positions of overlap between two segments are
// still the previous word a lane reads anyway -- for the same reason as w - 1 above, which is the case g = 0.  The
// contiguous kernels take none of this: the gap is a template switch, not a branch on their path.
#include "kmer_count.h"

namespace bamm {
namespace {

constexpr uint32_t kEntriesPerRound = 8;

struct Entry {                   // a record, or a segment of a long one, as one wave sees it
    const uint32_t* wp;          // the record's words
    const uint32_t* up;          // its unknown forward positions [nu]
    uint32_t L, wb, we, nu;      // the record's positions; the entry's words [wb, we) (none: nothing to do)
    uint32_t cur, prev;          // word wb + lane and the word before it
};

__device__ __forceinline__ Entry fetch_entry(const KmerCountArgs& a, uint64_t t, uint64_t total, int lane) {
    Entry e{};
    if (t >= total) return e;
    uint32_t s = (uint32_t)t, wb = 0;
    const bool whole = t < a.n;
    if (!whole) { const uint2 it = a.items[t - a.n]; s = it.x; wb = it.y; }
    const uint32_t L = a.len[s];
    const uint32_t nw = (L >> 4) + ((L & 15u) != 0u);
    if (whole && nw > a.seg_words) return e;                  // its segments are among the items
    e.L = L;
    e.wb = wb;
    e.we = whole ? nw : (nw - wb < a.seg_words ? nw : wb + a.seg_words);
    e.wp = a.words + a.word_off[s];
    const uint64_t u0 = a.unk_off[s];
    e.up = a.unk_pos + u0;
    e.nu = (uint32_t)(a.unk_off[s + 1] - u0);                 // (at most one per forward position)
    const uint32_t wi = wb + (uint32_t)lane;
    if (wi < e.we) { e.cur = e.wp[wi]; e.prev = wi ? e.wp[wi - 1u] : 0u; }
    return e;
}

// the positions lo .. lo + 31 (bit i = position lo + i) that hold an unknown base or, with both strands, the copy of one
__device__ __forceinline__ uint32_t unknown_bits(const Entry& e, int64_t lo, bool ds, int64_t L0) {
    auto first_at_least = [&](int64_t x) {
        uint32_t b = 0, t = e.nu;
        while (b < t) { const uint32_t mid = (b + t) >> 1; if ((int64_t)e.up[mid] < x) b = mid + 1u; else t = mid; }
        return b;
    };
    uint32_t bad = 0;
    for (uint32_t i = first_at_least(lo); i < e.nu; i++) {
        const int64_t z = e.up[i];
        if (z >= lo + 32) break;
        bad |= 1u << (uint32_t)(z - lo);
    }
    if (ds) {
        const int64_t zhi = 2 * L0 - lo;                      // the forward position whose copy is position lo
        for (uint32_t i = first_at_least(zhi - 31); i < e.nu; i++) {
            const int64_t z = e.up[i];
            if (z > zhi) break;
            bad |= 1u << (uint32_t)(zhi - z);
        }
    }
    return bad;
}

// kGapped: the window's halves lie `gap` positions apart (the same in every lane of the launch's workgroup)
template <int W, bool kGapped>
__device__ __forceinline__ void count_entry(const KmerCountArgs& a, const Entry& e, uint32_t* hist, uint32_t pass, int lane, uint32_t gap) {
    constexpr uint32_t kMask = (1u << (2 * W)) - 1u, kRun = (1u << W) - 1u;
    constexpr uint32_t kCellBits = 2 * W > 15 ? 15 : 2 * W;
    constexpr uint32_t kHalf = W / 2, kMaskHalf = (1u << W) - 1u;   // (gapped: W is even)
    const uint32_t span = (uint32_t)W + gap;                  // <= 16
    const uint32_t run = (1u << span) - 1u;
    const bool ds = a.single_strand == 0u;
    const int64_t L = e.L, L0 = (L - 1) / 2;                  // both strands: L = 2 L0 + 1, the separator at L0
    bool first = true;
    for (uint32_t wi = e.wb + (uint32_t)lane; wi < e.we; wi += 64u, first = false) {
        const uint32_t cur = first ? e.cur : e.wp[wi];
        const uint32_t prev = first ? e.prev : e.wp[wi - 1u];
        const int64_t lo = 16 * (int64_t)wi - 16;             // bit i of `bad` = position lo + i; the lane's own word is bits 16..31
        uint32_t bad = wi ? 0u : 0xffffu;                     // before the record
        if (L - lo < 32) bad |= ~0u << (uint32_t)(L - lo);    // behind it (L - lo >= 17: the word holds a position)
        if (ds && L0 >= lo && L0 < lo + 32) bad |= 1u << (uint32_t)(L0 - lo);
        if (e.nu) bad |= unknown_bits(e, lo, ds, L0);
        const unsigned long long both = ((unsigned long long)prev << 32) | cur;
        if constexpr (!kGapped) {
#pragma unroll
            for (int i = 16; i < 32; i++) {                   // the window that ends at position lo + i
                const bool ok = ((bad >> (i - W + 1)) & kRun) == 0u;
                const uint32_t y = (uint32_t)(both >> (62 - 2 * i)) & kMask;
                if (ok && (y >> kCellBits) == pass) atomicAdd(&hist[y & ((1u << kCellBits) - 1u)], 1u);
            }
        } else {
            // the left half ends h + gap positions before the window does, and the span starts at bit i - span + 1 >= 1: both as
            // one shift per word by what depends on the gap, then the constant shifts of the contiguous case
            const unsigned long long lefts = both >> (2u * (kHalf + gap));
            const uint32_t bads = bad >> (16u - span);
#pragma unroll
            for (int i = 16; i < 32; i++) {                   // the window that ends at position lo + i
                const bool ok = ((bads >> (i - 15)) & run) == 0u;
                const uint32_t right = (uint32_t)(both >> (62 - 2 * i)) & kMaskHalf;
                const uint32_t left = (uint32_t)(lefts >> (62 - 2 * i)) & kMaskHalf;
                const uint32_t y = (left << W) | right;
                if (ok && (y >> kCellBits) == pass) atomicAdd(&hist[y & ((1u << kCellBits) - 1u)], 1u);
            }
        }
    }
}

// the walk of workgroup (blockIdx.x, blockIdx.y) of `threads` threads over the records, into `table` [4^W] (the kernel reads
// its own blockDim: only there does the compiler know the workgroups of a launch to be of one size)
template <int W, bool kGapped>
__device__ __forceinline__ void count_records(const KmerCountArgs& a, unsigned long long* table, uint32_t gap, const uint32_t threads) {
    extern __shared__ uint32_t kmer_lds[];                    // [cells] the table, [1] windows added since the last flush (upper bound)
    constexpr uint32_t kCells = 2 * W > 15 ? (1u << 15) : (1u << (2 * W));
    uint32_t* hist = kmer_lds;
    uint32_t* added_total = kmer_lds + kCells;
    const uint32_t pass = blockIdx.y;
    unsigned long long* out = table + (size_t)pass * kCells;
    for (uint32_t i = threadIdx.x; i < kCells; i += threads) hist[i] = 0u;
    if (threadIdx.x == 0) *added_total = 0u;
    __syncthreads();
    auto flush = [&]() {                                      // every cell belongs to one thread
        for (uint32_t i = threadIdx.x; i < kCells; i += threads) {
            const uint32_t v = hist[i];
            if (v) { atomicAdd(&out[i], (unsigned long long)v); hist[i] = 0u; }
        }
    };
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6, waves = threads >> 6;
    const uint64_t total = a.n + a.n_items;
    const uint64_t per_round = (uint64_t)waves * kEntriesPerRound;
    for (uint64_t base = (uint64_t)blockIdx.x * per_round; base < total; base += (uint64_t)gridDim.x * per_round) {   // (the same trip count for every wave of the block)
        const uint64_t t0 = base + (uint64_t)wave * kEntriesPerRound;
        uint32_t added = 0;
        Entry nxt = fetch_entry(a, t0, total, lane);
        for (uint32_t r = 0; r < kEntriesPerRound; r++) {
            const Entry cur = nxt;
            if (r + 1u < kEntriesPerRound) nxt = fetch_entry(a, t0 + r + 1u, total, lane);
            added += (cur.we - cur.wb) * 16u;
            count_entry<W, kGapped>(a, cur, hist, pass, lane, gap);
        }
        if (lane == 0 && added) atomicAdd(added_total, added);
        __syncthreads();
        const bool full = *added_total >= a.flush_windows;
        __syncthreads();                                      // everybody has read the total: the next round may add to it
        if (full) {
            if (threadIdx.x == 0) *added_total = 0u;
            flush();
            __syncthreads();
        }
    }
    flush();
}

template <int W>
__global__ void __launch_bounds__(1024) k_kmer_counts(KmerCountArgs a) {
    count_records<W, false>(a, a.counts, 0u, blockDim.x);
}

// workgroup (b, p, z): the walk of (b, p) for gap gap_lo + z, into table z of a.counts [gaps][4^W]
template <int W>
__global__ void __launch_bounds__(1024) k_kmer_counts_gapped(KmerCountArgs a, uint32_t gap_lo) {
    count_records<W, true>(a, a.counts + ((size_t)blockIdx.z << (2 * W)), gap_lo + blockIdx.z, blockDim.x);
}

}  // namespace

KmerLaunch kmer_count_geometry(uint32_t w, int num_cus, uint32_t blocks, uint32_t threads) {
    KmerLaunch g{};
    g.cells = w >= 8u ? (1u << 15) : (1u << (2u * w));
    g.passes = (1u << (2u * w)) / g.cells;
    g.lds = (size_t)g.cells * sizeof(uint32_t) + 16;
    // as many workgroups per CU as the table leaves room for in its 160 KiB, sixteen waves per CU in all
    const uint32_t per_cu = w == 6u ? 4u : w == 7u ? 2u : 1u;
    g.threads = (threads && threads % 64u == 0u && threads <= 1024u) ? threads : 1024u / per_cu;
    g.blocks = blocks ? blocks : (uint32_t)(num_cus > 0 ? num_cus : 1) * per_cu;
    return g;
}

int launch_kmer_counts(const KmerCountArgs& a, uint32_t w, const KmerLaunch& g, hipStream_t st) {
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(reinterpret_cast<const void*>(kernel), g.lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3(g.blocks, g.passes), dim3(g.threads), g.lds, st, a);
        BAMM_HIP(hipGetLastError());
        return BAMM_OK;
    };
    switch (w) {
        case 6: return go(k_kmer_counts<6>);
        case 7: return go(k_kmer_counts<7>);
        case 8: return go(k_kmer_counts<8>);
    }
    set_error("launch_kmer_counts: w = %u outside 6..8", w);
    return BAMM_ERR_ARG;
}

int launch_kmer_counts_gapped(const KmerCountArgs& a, uint32_t w, uint32_t gap_lo, uint32_t n_gaps, const KmerLaunch& g, hipStream_t st) {
    if (n_gaps == 0u || w + gap_lo + n_gaps - 1u > 16u) {     // (the kernel's shifts rest on span <= 16)
        set_error("launch_kmer_counts_gapped: gaps %u..%u leave the span of 16 at w = %u", gap_lo, gap_lo + n_gaps - 1u, w);
        return BAMM_ERR_ARG;
    }
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(reinterpret_cast<const void*>(kernel), g.lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3(g.blocks, g.passes, n_gaps), dim3(g.threads), g.lds, st, a, gap_lo);
        BAMM_HIP(hipGetLastError());
        return BAMM_OK;
    };
    switch (w) {
        case 6: return go(k_kmer_counts_gapped<6>);
        case 8: return go(k_kmer_counts_gapped<8>);
    }
    set_error("launch_kmer_counts_gapped: w = %u is neither 6 nor 8", w);
    return BAMM_ERR_ARG;
}

}  // namespace bamm
