// Exact w-mer counts of a resident set (csrc/kmer_count.hip): what bamm_kmer_counts launches.  No reference counterpart:
// the reference has no seeding stage of its own.
#pragma once
#include "common.h"

namespace bamm {

struct KmerCountArgs {
    const uint32_t* words;       // the set's 2-bit stream, word_off, len as in SeqView
    const uint64_t* word_off;
    const uint32_t* len;
    const uint64_t* unk_off;     // [n + 1] into unk_pos
    const uint32_t* unk_pos;     // forward positions that held an unknown base, ascending within a record
    uint64_t n;                  // records
    const uint2* items;          // the segments of the records of more than seg_words words: (record, first word)
    uint32_t n_items;
    uint32_t seg_words;          // words per segment
    uint32_t single_strand;
    uint32_t flush_windows;      // a workgroup flushes its table once it has added this many windows
    unsigned long long* counts;  // [4^w], added into (the gapped launch: [gaps][4^w])
};

// One launch: `blocks` x `passes` workgroups of `threads`; workgroup (b, h) holds the `cells` cells of the table whose
// index starts with h (the leading base's high bit at w = 8, where the whole table does not fit one CU's LDS).
struct KmerLaunch { uint32_t blocks, threads, passes, cells; size_t lds; };
KmerLaunch kmer_count_geometry(uint32_t w, int num_cus, uint32_t blocks, uint32_t threads);
int launch_kmer_counts(const KmerCountArgs& a, uint32_t w, const KmerLaunch& g, hipStream_t st);
// The dyad tables of gaps gap_lo .. gap_lo + n_gaps - 1 (w = 6 or 8, w + the largest gap <= 16) in one launch of
// `blocks` x `passes` x n_gaps workgroups: workgroup (b, h, z) is workgroup (b, h) of the launch above for the windows whose
// halves lie gap_lo + z positions apart, and adds into a.counts + z * 4^w.
int launch_kmer_counts_gapped(const KmerCountArgs& a, uint32_t w, uint32_t gap_lo, uint32_t n_gaps, const KmerLaunch& g, hipStream_t st);

}  // namespace bamm
