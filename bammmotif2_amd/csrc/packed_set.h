// A bamm_packed (include/bamm_em.h) on the host: who owns it until the caller does, the one place its seven arrays are
// allocated, and the one place lengths become its header.  negs.cpp builds the sampled negatives' set through these; pack.cpp
// and bamm_seqs_from_codes still allocate by hand (see HISTORY.md).  No HIP here: it compiles with plain g++.
#pragma once
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/bamm_em.h"

namespace bamm {

void set_error(const char* fmt, ...);                         // pack.cpp

// owns a set until release() hands it to the caller of the C ABI (who calls bamm_packed_free)
struct PackedFree { void operator()(bamm_packed* p) const { bamm_packed_free(p); } };
using PackedPtr = std::unique_ptr<bamm_packed, PackedFree>;

// A set of these counts with all seven arrays, zeroed.  Every array has at least one element: the Python views map
// max(count, 1) elements of each.
inline int packed_alloc(uint64_t n_seqs, uint64_t n_words, uint64_t n_exc, PackedPtr* out) {
    PackedPtr p((bamm_packed*)calloc(1, sizeof(bamm_packed)));
    if (p) {
        p->n_seqs = n_seqs; p->n_words = n_words; p->n_exc = n_exc;
        const size_t ne = n_exc ? n_exc : 1;
        p->words = (uint32_t*)calloc(n_words ? n_words : 1, sizeof(uint32_t));
        p->word_off = (uint64_t*)calloc(n_seqs + 1, sizeof(uint64_t));
        p->len = (uint32_t*)calloc(n_seqs ? n_seqs : 1, sizeof(uint32_t));
        p->exc_off = (uint64_t*)calloc(n_seqs + 1, sizeof(uint64_t));
        p->exc_pos = (uint32_t*)calloc(ne, sizeof(uint32_t));
        p->exc_kmer = (uint32_t*)calloc(ne, sizeof(uint32_t));
        p->exc_clean = (uint32_t*)calloc(ne, sizeof(uint32_t));
    }
    if (!p || !p->words || !p->word_off || !p->len || !p->exc_off || !p->exc_pos || !p->exc_kmer || !p->exc_clean) {
        set_error("out of memory");
        return BAMM_ERR_ARG;
    }
    *out = std::move(p);
    return BAMM_OK;
}

// Where the unknown bases of a set built from FASTA codes were: per record the FORWARD positions that held code 0, ascending.
// The exception list cannot tell (it marks every position whose 11-mer is tainted and carries the byte-'N' quirk of the
// reverse strand), so the makers that see the codes (bamm_pack_codes*) note the list beside the
// bamm_packed they return -- the public struct keeps its layout; the note is kept by the packed set's address until
// bamm_packed_free -- and bamm_seqs_upload hands it to the resident set.  Sets packed from kmer_ arrays have none.
// Invariant of the note: every bamm_packed the library hands out is released through bamm_packed_free, which forgets the
// note before the memory goes back (include/bamm_em.h says so).  A struct copied by value has no note (its address differs);
// the library's own makers that do not see codes (pack_impl, packed_alloc) return fresh calloc blocks, whose addresses can
// only repeat one that bamm_packed_free has already forgotten.
struct UnknownList {
    bool single_strand = false;
    std::vector<uint64_t> off;   // [n_seqs + 1]
    std::vector<uint32_t> pos;   // [off[n_seqs]]
};
std::shared_ptr<const UnknownList> unknowns_of_codes(const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, bool single_strand);   // pack.cpp, like the three below
void packed_note_unknowns(const bamm_packed* p, std::shared_ptr<const UnknownList> list);
std::shared_ptr<const UnknownList> packed_unknowns(const bamm_packed* p);                  // null: none noted
void packed_forget_unknowns(const bamm_packed* p);

// What bamm_kmer_counts_gapped and its host twin accept (include/bamm_em.h): w = 6..8, gap_lo <= gap_hi, span w + gap_hi <= 16,
// and a gap above 0 only between equal halves (w even).
inline int kmer_gap_range_ok(const char* who, uint32_t w, uint32_t gap_lo, uint32_t gap_hi) {
    if (w < 6 || w > 8) { set_error("%s: w = %u outside 6..8", who, w); return BAMM_ERR_ARG; }
    if (gap_lo > gap_hi) { set_error("%s: gap_lo = %u above gap_hi = %u", who, gap_lo, gap_hi); return BAMM_ERR_ARG; }
    if (gap_hi > 16u - w) { set_error("%s: w + gap_hi = %u + %u exceeds the span of 16", who, w, gap_hi); return BAMM_ERR_ARG; }
    if ((w & 1u) && gap_hi > 0) { set_error("%s: a gap needs equal halves, w = %u is odd", who, w); return BAMM_ERR_ARG; }
    return BAMM_OK;
}

// The length rule: 16 positions per 32-bit word, every sequence on a word boundary.  From p->n_seqs lengths (`lens` may
// be p->len itself) it fills len, word_off, n_words, total_len, max_len and min_len (0 for an empty set).  exc_off is
// left as it is: all zero as allocated, which is right for a set given by its lengths alone (no exceptions).  On a bare
// header (len and word_off null) it only counts, which tells packed_alloc's caller the words before anything is allocated.
template <class L>
int packed_set_lengths(bamm_packed* p, const L* lens) {
    const bool store = p->word_off != nullptr;
    uint64_t n_words = 0, total = 0;
    uint32_t max_len = 0, min_len = p->n_seqs ? UINT32_MAX : 0;
    for (uint64_t n = 0; n < p->n_seqs; n++) {
        const uint64_t len = lens[n];
        if (len > 0xffffffffull) { set_error("sequence %llu longer than 2^32-1", (unsigned long long)n); return BAMM_ERR_ARG; }
        if (store) { p->len[n] = (uint32_t)len; p->word_off[n] = n_words; }
        n_words += (len + 15) / 16;
        total += len;
        if (len > max_len) max_len = (uint32_t)len;
        if (len < min_len) min_len = (uint32_t)len;
    }
    if (store) p->word_off[p->n_seqs] = n_words;
    p->n_words = n_words; p->total_len = total; p->max_len = max_len; p->min_len = min_len;
    return BAMM_OK;
}

}  // namespace bamm
