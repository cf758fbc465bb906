// bamm_sample_negatives: the host side of SeqGenerator::sample_bgseqset_by_fold (SeqGenerator.cpp:63-348) on the device
// (csrc/negs.hip), as a sequence of stages over one NegCall.  Host code only.

#include <cstring>
#include <memory>

#include "glibc_rand.h"
#include "handles.h"
#include "neg_layout.h"
#include "negs.h"
#include "packed_set.h"

using namespace bamm;

namespace {

struct NegCall {
    bamm_ctx* c;
    bamm_seqs* pos;
    DevBlocks tmp;                                           // the sampler's buffers: freed before the negatives' resident set is made
    NegArgs a{};
    NegLongArgs la{};
    std::vector<uint64_t> long_pos, chunk_off{0};            // positives beyond the length classes, their counting chunks
    std::vector<unsigned long long> cnt;                     // the set's (k+1)-mer totals
    std::vector<float> v, bar;                               // its conditionals and bars
    NegLayout lay;                                           // output_layout fills it
    std::vector<uint64_t> wo;                                // [n + 1] first output word of positive i's kept negatives
    std::vector<NegLongRec> rec;                             // the long positives' kept negatives and their segments
    std::vector<uint64_t> seg_off{0};
    GlibcRandStream gen;                                     // the generator's seed state and the powers t^(2^b): read by the
    std::vector<uint32_t> pw;                                // uploads until the stream is next synchronised
    NegCall(bamm_ctx* ctx, bamm_seqs* p, const ExcK* exc) : c(ctx), pos(p), tmp(ctx), wo(p->n + 1, 0) {
        a.words = p->d_words; a.word_off = p->d_word_off; a.len = p->d_len; a.exc_off = exc->d_off; a.exc = exc->d_exc;
        a.n = p->n;
        for (uint32_t k = 0; k <= kNegMaxOrder; k++) a.A[k] = 20.0f;        // SeqGenerator.cpp:29-32
    }
    uint32_t table_cells() const { return (uint32_t)bg_size(a.s); }
    static uint64_t words_per(uint64_t L) { return (L + 15) / 16; }   // of one negative (or positive) of L positions
};

// whether this set is the device sampler's to take
int check_supported(const bamm_ctx* c, const bamm_seqs* pos, uint32_t s_order) {
    if (pos->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    // the three declines below are BAMM_ERR_UNSUPPORTED: the CLI samples on the host on exactly that code
    if (s_order != kNegMaxOrder) {
        set_error("the device sampler is written for -s 2 (SeqGenerator.cpp:112-186); other orders run on the host");
        return BAMM_ERR_UNSUPPORTED;
    }
    if (pos->n == 0) { set_error("the device sampler takes non-empty sets"); return BAMM_ERR_UNSUPPORTED; }
    if (!GlibcRandStream::libc_is_this_generator()) {
        set_error("libc's rand() is not the restated glibc generator on this host: the sampler runs on the host, drawing from libc itself");
        return BAMM_ERR_UNSUPPORTED;
    }
    return BAMM_OK;
}

// positives beyond the length classes are counted chunk by chunk and sampled segment by segment (negs.hip)
int long_positives(NegCall& n) {
    NegLongArgs& la = n.la;
    for (uint64_t i = 0; i < n.pos->n; i++)
        if (n.pos->h_len[i] > BAMM_MAX_SEQ_POSITIONS) {
            n.long_pos.push_back(i);
            n.chunk_off.push_back(n.chunk_off.back() + (NegCall::words_per(n.pos->h_len[i]) + kNegCountWords - 1) / kNegCountWords);
        }
    if (n.long_pos.size() > UINT32_MAX) { set_error("bamm_sample_negatives: too many long sequences"); return BAMM_ERR_ARG; }
    la.n_long = n.long_pos.size(); la.n_chunks = n.chunk_off.back();
    la.S = n.c->neg_segment_positions ? n.c->neg_segment_positions / 16u * 16u : kNegSegment;
    if (!la.n_long) return BAMM_OK;
    uint64_t *d_long = nullptr, *d_chunk = nullptr;
    int rc;
    if ((rc = n.tmp.upload(&d_long, n.long_pos.data(), n.long_pos.size())) || (rc = n.tmp.upload(&d_chunk, n.chunk_off.data(), n.chunk_off.size())) ||
        (rc = n.tmp.alloc(&la.cnt, la.n_long * kNegTable)) || (rc = n.tmp.alloc(&la.bar, la.n_long * kNegTable))) return rc;
    la.long_pos = d_long; la.chunk_off = d_chunk;
    if (hipMemsetAsync(la.cnt, 0, la.n_long * kNegTable * sizeof(uint32_t), n.c->stream) != hipSuccess) { set_error("hipMemsetAsync failed"); return BAMM_ERR_HIP; }
    return BAMM_OK;
}

// the counting launches and the set's totals (the tables' device arrays are allocated with them)
int count_kmers(NegCall& n) {
    NegArgs& a = n.a;
    hipStream_t st = n.c->stream;
    const uint32_t tot = n.table_cells();
    int rc;
    if ((rc = n.tmp.alloc(&a.total_counts, tot)) || (rc = n.tmp.alloc(&a.bad, 1))) return rc;
    if (hipMemsetAsync(a.total_counts, 0, tot * sizeof(unsigned long long), st) != hipSuccess || hipMemsetAsync(a.bad, 0, sizeof(uint32_t), st) != hipSuccess) {
        set_error("hipMemsetAsync failed"); return BAMM_ERR_HIP;
    }
    if ((rc = launch_neg_counts(a, st)) || (rc = launch_neg_counts_long(a, n.la, st))) return rc;
    n.cnt.resize(tot);
    if (hipMemcpyAsync(n.cnt.data(), a.total_counts, tot * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        set_error("bamm_sample_negatives: the counting pass failed"); return BAMM_ERR_HIP;
    }
    return BAMM_OK;
}

// the set's conditionals and their bars from the totals: neg_layout.h's, shared with the host sampler
void set_tables(NegCall& n) {
    n.v.assign(n.table_cells(), 0.f); n.bar.assign(n.table_cells(), 0.f);
    neg_set_tables(n.cnt.data(), n.a.s, n.a.A, n.v.data(), n.bar.data(), [](uint32_t k) { return bg_offset(k); });
}

// which negatives are kept and where every positive's draws start (neg_layout.h's, shared with the host sampler), where its
// kept negatives go in the output stream; the long positives' kept negatives and their segments
void output_layout(NegCall& n) {
    const bamm_seqs* pos = n.pos;
    n.lay = NegLayout(pos->n, [pos](uint64_t i) { return pos->h_len[i]; }, n.a.m_fold, n.a.keep_stride);
    for (uint64_t i = 0; i < pos->n; i++) n.wo[i + 1] = n.wo[i] + n.lay.n_kept(i) * NegCall::words_per(pos->h_len[i]);
    for (uint64_t li = 0; li < n.la.n_long; li++) {
        const uint64_t i = n.long_pos[li], L = pos->h_len[i];
        uint64_t rank = 0;
        for (uint64_t f = 0; f < n.lay.m_fold; f++) {
            if (!n.lay.kept(i, f)) continue;
            n.rec.push_back(NegLongRec{n.lay.draw0[i] + f * L, n.wo[i] + rank++ * NegCall::words_per(L), (uint32_t)L, (uint32_t)li});
            n.seg_off.push_back(n.seg_off.back() + (L + n.la.S - 1) / n.la.S);
        }
    }
    n.la.n_rec = n.rec.size(); n.la.n_seg = n.seg_off.back();
}

// the generator as srand(42) leaves it (SeqGenerator.cpp:35) and the powers t^(2^b) the lanes jump ahead with
void generator_tables(NegCall& n) {
    n.gen.seed(42u);
    n.pw.assign(48 * 31, 0);
    uint32_t base[31] = {0, 1}, sq[31];
    for (int b = 0; b < 48; b++) {
        memcpy(n.pw.data() + 31 * b, base, sizeof base);
        GlibcRandStream::poly_mul(base, base, sq);
        memcpy(base, sq, sizeof sq);
    }
}

int upload_tables(NegCall& n) {
    NegArgs& a = n.a;
    NegLongArgs& la = n.la;
    hipStream_t st = n.c->stream;
    const uint64_t np = n.pos->n;
    const uint32_t tot = n.table_cells();
    const std::vector<uint32_t>& pw = n.pw;
    float *d_v = nullptr, *d_bar = nullptr;
    uint64_t *d_draw0 = nullptr, *d_wo = nullptr;
    uint32_t *d_seed = nullptr, *d_pw = nullptr;
    int rc;
    if ((rc = n.tmp.alloc(&d_v, tot)) || (rc = n.tmp.alloc(&d_bar, tot)) || (rc = n.tmp.alloc(&d_draw0, np)) || (rc = n.tmp.alloc(&d_wo, np)) ||
        (rc = n.tmp.alloc(&d_seed, 34)) || (rc = n.tmp.alloc(&d_pw, pw.size())) || (rc = n.tmp.alloc(&a.out_words, n.wo[np]))) return rc;
    hipError_t e = hipMemcpyAsync(d_v, n.v.data(), tot * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_bar, n.bar.data(), tot * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && (ctx_upload(n.c, d_draw0, n.lay.draw0.data(), np * sizeof(uint64_t)) || ctx_upload(n.c, d_wo, n.wo.data(), np * sizeof(uint64_t)))) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipMemcpyAsync(d_seed, n.gen.r, sizeof n.gen.r, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pw, pw.data(), pw.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { set_error("bamm_sample_negatives: upload failed: %s", hipGetErrorString(e)); return BAMM_ERR_HIP; }
    a.v = d_v; a.bar = d_bar; a.draw0 = d_draw0; a.out_word_off = d_wo; a.seed_state = d_seed; a.pow2 = d_pw;
    if (!la.n_seg) return BAMM_OK;
    NegLongRec* d_rec = nullptr;
    uint64_t* d_seg = nullptr;
    if ((rc = n.tmp.upload(&d_rec, n.rec.data(), n.rec.size())) || (rc = n.tmp.upload(&d_seg, n.seg_off.data(), n.seg_off.size())) || (rc = n.tmp.alloc(&la.map, la.n_seg)) ||
        (rc = n.tmp.alloc(&la.state, 34 * la.n_seg)) || (rc = n.tmp.alloc(&la.entry, la.n_seg))) return rc;
    la.rec = d_rec; la.seg_off = d_seg;
    return BAMM_OK;
}

int sample(NegCall& n) {
    int rc;
    if (n.la.n_long < n.pos->n && (rc = launch_neg_sample(n.a, n.c->stream))) return rc;
    return launch_neg_sample_long(n.a, n.la, n.c->stream);
}

// the negatives as a packed set of their own (single strand, no unknown base: no exceptions), and the `bad` count
int download_negatives(NegCall& n, PackedPtr* out, uint32_t* bad) {
    const uint64_t n_words = n.wo[n.pos->n];
    PackedPtr p;
    if (int rc = packed_alloc(n.lay.n_neg(), n_words, 0, &p)) return rc;
    bool ok = true;
    if (n_words) ok = ctx_download(n.c, p->words, n.a.out_words, n_words * sizeof(uint32_t)) == BAMM_OK;
    if (ok) ok = hipMemcpyAsync(bad, n.a.bad, sizeof *bad, hipMemcpyDeviceToHost, n.c->stream) == hipSuccess;
    if (ok) ok = hipStreamSynchronize(n.c->stream) == hipSuccess;
    if (!ok) { set_error("bamm_sample_negatives: the sampling pass failed"); return BAMM_ERR_HIP; }
    for (uint64_t i = 0; i < n.pos->n; i++)
        std::fill(p->len + n.lay.first_kept[i], p->len + n.lay.first_kept[i + 1], n.pos->h_len[i]);
    if (int rc = packed_set_lengths(p.get(), p->len)) return rc;
    *out = std::move(p);
    return BAMM_OK;
}

}  // namespace

extern "C" {

int bamm_sample_negatives(bamm_ctx* c, bamm_seqs* pos, uint32_t s_order, uint64_t m_fold, int generic, uint64_t keep_stride,
                          bamm_packed** packed_out, bamm_seqs** seqs_out) {
    if (!c || !pos || !packed_out || m_fold == 0) { set_error("bamm_sample_negatives: bad argument"); return BAMM_ERR_ARG; }
    *packed_out = nullptr;
    if (seqs_out) *seqs_out = nullptr;
    int rc = check_supported(c, pos, s_order);
    if (rc) return rc;
    BAMM_HIP(hipSetDevice(c->device));
    ExcK* exc = nullptr;
    if ((rc = exceptions_for_order(pos, s_order, &exc))) return rc;
    NegCall n(c, pos, exc);
    n.a.s = s_order; n.a.generic = generic; n.a.m_fold = m_fold; n.a.keep_stride = keep_stride;
    if ((rc = long_positives(n)) || (rc = count_kmers(n))) return rc;
    set_tables(n);
    output_layout(n);
    generator_tables(n);
    if ((rc = upload_tables(n)) || (rc = sample(n))) return rc;
    PackedPtr p;
    uint32_t bad = 0;
    if ((rc = download_negatives(n, &p, &bad))) return rc;
    n.tmp.free_all();                                        // the sampler's buffers go before the negatives' resident set is made
    if (bad) {                                               // rand() == RAND_MAX at a first base: the reference leaves that byte unset
        set_error("a first base drew rand() == RAND_MAX, which the reference leaves undefined: sample this set on the host");
        return BAMM_ERR_UNSUPPORTED;
    }
    if (seqs_out && (rc = bamm_seqs_upload(c, p.get(), 0, p->n_seqs, seqs_out))) return rc;
    *packed_out = p.release();
    return BAMM_OK;
}

int bamm_neg_segment_geometry(uint32_t* segment_positions) {
    if (!segment_positions) { set_error("bamm_neg_segment_geometry: null output"); return BAMM_ERR_ARG; }
    *segment_positions = kNegSegment;
    return BAMM_OK;
}

}  // extern "C"
