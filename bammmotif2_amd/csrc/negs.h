// SeqGenerator's negative sampler on the device (csrc/negs.hip); reference: /root/reference/src/seq_generator/SeqGenerator.cpp:63-348.
#pragma once
#include "common.h"

namespace bamm {

constexpr uint32_t kNegMaxOrder = 2;                          // the sequence-specific rescaling is written for s = 2 (:112-186)
constexpr uint32_t kNegTable = 84;                            // 4 + 16 + 64 cells of the orders 0..2

struct NegArgs {
    // the resident positives (bamm_seqs) and their exception list of order s
    const uint32_t* words; const uint64_t* word_off; const uint32_t* len; const uint64_t* exc_off; const uint2* exc;
    uint64_t n;
    uint32_t s;                  // order of the sampler's conditionals (-s, 2)
    int generic;                 // --genericNeg: the set's own bars for every positive
    uint64_t m_fold, keep_stride;
    unsigned long long* total_counts;   // [kNegTable] k_neg_counts adds into it
    const float* v;              // [kNegTable] the set's conditionals (host: kmer_frequency's tail)
    const float* bar;            // [kNegTable] their cumulative bars
    float A[kNegMaxOrder + 1];   // pseudo-counts (20, SeqGenerator.cpp:29-32)
    const uint64_t* draw0;       // [n] first draw of positive i: sum over the positives before it of L * m_fold
    const uint32_t* seed_state;  // [34] the generator as srand(42) leaves it
    const uint32_t* pow2;        // [48][31] t^(2^b) mod (t^31 - t^28 - 1)
    const uint64_t* out_word_off;// [n] first output word of positive i's kept negatives
    uint32_t* out_words;
    uint32_t* bad;               // counts the draws the reference leaves undefined (rand() == RAND_MAX at a first base)
};

// Positives beyond BAMM_MAX_SEQ_POSITIONS: their negatives are cut into segments of S positions (a multiple of 16, so that a
// 2-bit output word belongs to one segment), a lane per segment (negs.hip: k_neg_segments).
constexpr uint32_t kNegSegment = 4096;                       // S unless the context's "neg_segment_positions" says otherwise
constexpr uint32_t kNegCountWords = 1024;                     // words of a long positive one wave counts (k_neg_counts_long)

struct NegLongRec {              // one kept negative of a long positive
    uint64_t draw_start;         // its first draw: draw0[n] + f L
    uint64_t out_off;            // its first output word: out_word_off[n] + kept rank * words per negative
    uint32_t L, tab;             // positions; its positive's row of NegLongArgs::bar
};

struct NegLongArgs {
    const uint64_t* long_pos;    // [n_long] the long positives' indices in the set, ascending
    uint64_t n_long;
    const uint64_t* chunk_off;   // [n_long + 1] first counting chunk (kNegCountWords words) of each
    uint64_t n_chunks;
    uint32_t* cnt;               // [n_long][kNegTable] their (k+1)-mer counts (zeroed by the caller)
    float* bar;                  // [n_long][kNegTable] their bars (k_neg_tables)
    const NegLongRec* rec; uint64_t n_rec;
    const uint64_t* seg_off;     // [n_rec + 1] first segment of each kept negative
    uint64_t n_seg;
    uint32_t S;
    unsigned long long* map;     // [n_seg] context -> context over the segment, 16 x 4 bits
    uint32_t* state;             // [34][n_seg] the generator at the segment's first draw
    uint8_t* entry;              // [n_seg] the context the segment starts in (k_neg_entry)
};

int launch_neg_counts(const NegArgs& a, hipStream_t st);      // positives up to BAMM_MAX_SEQ_POSITIONS
int launch_neg_sample(const NegArgs& a, hipStream_t st);
int launch_neg_counts_long(const NegArgs& a, const NegLongArgs& la, hipStream_t st);   // the longer ones
int launch_neg_sample_long(const NegArgs& a, const NegLongArgs& la, hipStream_t st);

}  // namespace bamm
