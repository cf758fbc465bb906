// bamm_kmer_counts and bamm_kmer_counts_gapped of the C ABI: the exact w-mer table of a resident set, and its dyad tables over
// a range of gaps (csrc/kmer_count.hip), for the de novo seeder.  Host code only.  The host twins, bamm_kmer_counts_host and
// bamm_kmer_counts_gapped_host, are in pack.cpp with the rest of the host-only ABI.

#include "handles.h"
#include "kmer_count.h"

using namespace bamm;

namespace {

// the set's list of unknown forward positions on the device, once (the list itself came with the packed set: packed_set.h)
int unknowns_on_device(bamm_seqs* s) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->d_unk_off) return BAMM_OK;
    const UnknownList& u = *s->unk;
    const uint64_t b = s->unk_begin, first = u.off[b];
    std::vector<uint64_t> off(s->n + 1);
    for (uint64_t n = 0; n <= s->n; n++) off[n] = u.off[b + n] - first;
    DevBlocks made(s->ctx);                                  // the set's once both arrays are in place
    uint64_t* d_off = nullptr;
    uint32_t* d_pos = nullptr;
    int rc = made.upload(&d_off, off.data(), off.size());
    if (!rc) rc = off[s->n] ? made.upload(&d_pos, u.pos.data() + first, off[s->n]) : made.alloc(&d_pos, 1);
    if (rc) return rc;
    if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) { set_error("stream sync failed while uploading the unknown positions"); return BAMM_ERR_HIP; }
    s->mem.adopt(made, d_off); s->mem.adopt(made, d_pos);
    s->d_unk_pos = d_pos;
    s->d_unk_off = d_off;
    return BAMM_OK;
}


// One launch over the set: the contiguous table (gapped == false, n_gaps == 1) or the tables of gaps gap_lo .. gap_lo + n_gaps - 1;
// counts [n_gaps][4^w], n_windows [n_gaps] or null.  `who`: the entry point, for messages.
int count_tables(const char* who, bamm_ctx* c, const bamm_seqs* seqs, uint32_t w, bool gapped, uint32_t gap_lo, uint32_t n_gaps,
                 uint64_t* counts, uint64_t* n_windows) {
    if (seqs->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    if (!seqs->unk) {
        set_error("%s: the set does not say where its unknown bases were (packed from kmer_ arrays, bamm_pack_kmers*, or on the "
                  "device, bamm_seqs_from_codes); upload a set bamm_pack_codes* made", who);
        return BAMM_ERR_UNSUPPORTED;
    }
    bamm_seqs* s = const_cast<bamm_seqs*>(seqs);             // (the device copy of the list is made on first use, under the set's mutex)
    const size_t cells = ipow4(w), all = cells * n_gaps;
    std::fill(counts, counts + all, uint64_t(0));
    if (n_windows) std::fill(n_windows, n_windows + n_gaps, uint64_t(0));
    if (s->n == 0) return BAMM_OK;
    BAMM_HIP(hipSetDevice(c->device));
    int rc = unknowns_on_device(s);
    if (rc) return rc;
    KmerCountArgs a{};
    a.words = s->d_words; a.word_off = s->d_word_off; a.len = s->d_len;
    a.unk_off = s->d_unk_off; a.unk_pos = s->d_unk_pos;
    a.n = s->n;
    a.single_strand = s->unk->single_strand ? 1u : 0u;
    a.seg_words = (c->kmer_segment_positions ? c->kmer_segment_positions : BAMM_MAX_SEQ_POSITIONS) / 16u;
    a.flush_windows = c->kmer_flush_windows ? c->kmer_flush_windows : (1u << 31);
    // records beyond a segment's length: their segments, the positions of overlap (w - 1, or span - 1 <= 15) being the word a lane reads before its own
    std::vector<uint2> items;
    for (uint64_t n = 0; n < s->n; n++) {
        const uint64_t nw = ((uint64_t)s->h_len[n] + 15) / 16;
        if (nw <= a.seg_words) continue;
        for (uint64_t wb = 0; wb < nw; wb += a.seg_words) items.push_back(make_uint2((uint32_t)n, (uint32_t)wb));
    }
    if (items.size() > 0xffffffffull) { set_error("%s: more than 2^32 segments", who); return BAMM_ERR_UNSUPPORTED; }
    a.n_items = (uint32_t)items.size();
    DevBlocks tmp(c);
    uint2* d_items = nullptr;
    unsigned long long* d_counts = nullptr;
    if (!items.empty() && (rc = tmp.upload(&d_items, items.data(), items.size()))) return rc;
    if ((rc = tmp.alloc(&d_counts, all))) return rc;
    a.items = d_items; a.counts = d_counts;
    const KmerLaunch g = kmer_count_geometry(w, c->num_cus, c->blocks, c->threads);
    BAMM_HIP(hipMemsetAsync(d_counts, 0, all * sizeof(unsigned long long), c->stream));
    if ((rc = gapped ? launch_kmer_counts_gapped(a, w, gap_lo, n_gaps, g, c->stream) : launch_kmer_counts(a, w, g, c->stream))) return rc;
    if ((rc = ctx_download(c, counts, d_counts, all * sizeof(uint64_t)))) return rc;   // (through the context's pinned area)
    BAMM_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t z = 0; n_windows && z < n_gaps; z++) {
        uint64_t total = 0;
        for (size_t y = 0; y < cells; y++) total += counts[z * cells + y];
        n_windows[z] = total;
    }
    return BAMM_OK;
}

}  // namespace

extern "C" {

int bamm_kmer_counts(bamm_ctx* c, const bamm_seqs* seqs, uint32_t w, uint64_t* counts, uint64_t* n_windows) {
    if (!c || !seqs || !counts) { set_error("bamm_kmer_counts: null argument"); return BAMM_ERR_ARG; }
    if (w < 6 || w > 8) { set_error("bamm_kmer_counts: w = %u outside 6..8", w); return BAMM_ERR_ARG; }
    return count_tables("bamm_kmer_counts", c, seqs, w, false, 0, 1, counts, n_windows);
}

int bamm_kmer_counts_gapped(bamm_ctx* c, const bamm_seqs* seqs, uint32_t w, uint32_t gap_lo, uint32_t gap_hi, uint64_t* counts,
                            uint64_t* n_windows) {
    if (!c || !seqs || !counts) { set_error("bamm_kmer_counts_gapped: null argument"); return BAMM_ERR_ARG; }
    if (int rc = kmer_gap_range_ok("bamm_kmer_counts_gapped", w, gap_lo, gap_hi)) return rc;
    // (w = 7 comes here with gap 0 only: the contiguous kernel; w = 6 and 8 take the dyad kernel at every gap, 0 included)
    return count_tables("bamm_kmer_counts_gapped", c, seqs, w, (w & 1u) == 0u, gap_lo, gap_hi - gap_lo + 1u, counts, n_windows);
}

}  // extern "C"
