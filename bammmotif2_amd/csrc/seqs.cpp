// Resident sequence sets of the C ABI: the 2-bit stream on the device with its length buckets, the per-order exception
// lists and the grouped kernel's per-sequence records built from them, packing on the device (bamm_seqs_from_codes), the
// background counts.  The negative sampler's host side is negs.cpp.  Host code only.

#include <cstdlib>

#include "handles.h"

namespace bamm {

// build (once per order) the list of positions whose kmer_ mod 4^(K+1) differs from what the
// 2-bit stream gives
int exceptions_for_order(bamm_seqs* s, uint32_t K, ExcK** out) {
    std::lock_guard<std::mutex> lock(s->mu);
    auto it = s->exc_by_order.find(K);
    if (it != s->exc_by_order.end()) { *out = &it->second; return BAMM_OK; }
    const uint32_t maskY = (uint32_t)(ipow4(K + 1) - 1);
    ExcK k;
    k.h_off.resize(s->n + 1);
    // two passes over fixed parts of the set, a thread each: counts per sequence (left in h_off[n + 1]) and per part, a scan over
    // the parts, then every part turns its counts into offsets while it fills its stretch of the list -- the same list in the
    // same order as one walk would give, with no pass over a million records on one thread
    const uint32_t parts = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(host_threads_hint(), s->n / 16384 + 1));
    std::vector<uint64_t> part_total(parts + 1, 0);
    auto part_range = [&](uint32_t t, uint64_t& n0, uint64_t& n1) { n0 = s->n * t / parts; n1 = s->n * (t + 1) / parts; };
    auto on_parts = [&](auto&& fn) {
        if (parts == 1) { fn(0u); return; }
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < parts; t++) th.emplace_back([&fn, t] { fn(t); });
        for (auto& x : th) x.join();
    };
    on_parts([&](uint32_t t) {
        uint64_t n0, n1, total = 0;
        part_range(t, n0, n1);
        for (uint64_t n = n0; n < n1; n++) {
            uint64_t c = 0;
            for (uint64_t e = s->h_exc_off[n]; e < s->h_exc_off[n + 1]; e++) c += ((s->h_exc_kmer[e] ^ s->h_exc_clean[e]) & maskY) != 0u;
            k.h_off[n + 1] = c;
            total += c;
        }
        part_total[t + 1] = total;
    });
    for (uint32_t t = 0; t < parts; t++) part_total[t + 1] += part_total[t];
    k.h_ex.resize(part_total[parts]);
    k.h_off[0] = 0;
    on_parts([&](uint32_t t) {
        uint64_t n0, n1;
        part_range(t, n0, n1);
        uint64_t at = part_total[t];
        for (uint64_t n = n0; n < n1; n++) {
            for (uint64_t e = s->h_exc_off[n]; e < s->h_exc_off[n + 1]; e++)
                if (((s->h_exc_kmer[e] ^ s->h_exc_clean[e]) & maskY) != 0u)
                    k.h_ex[at++] = make_uint2(s->h_exc_pos[e], s->h_exc_kmer[e] & maskY);
            k.h_off[n + 1] = at;                              // (was the count: read above, by this thread)
        }
    });
    k.count = k.h_ex.size();
    DevBlocks made(s->ctx);                                  // the set's once the table is complete
    int rc = made.upload(&k.d_off, k.h_off.data(), k.h_off.size());
    if (!rc) rc = made.upload(&k.d_exc, k.h_ex.data(), k.h_ex.size());
    if (rc) return rc;
    if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) {
        set_error("stream sync failed while uploading the exception list");
        return BAMM_ERR_HIP;
    }
    s->mem.adopt(made, k.d_off); s->mem.adopt(made, k.d_exc);
    auto ins = s->exc_by_order.emplace(K, std::move(k));
    *out = &ins.first->second;
    return BAMM_OK;
}

// records of the grouped kernel for group size G (built once per (order, G)): x = first exception
// position | B << 12, y/z/w = exact y of the positions lo-G+1 .. lo+B-1, one bit string of 7-bit fields (10 at K = 3)
int xrec_for_group(bamm_seqs* s, uint32_t K, uint32_t G, ExcK* k, const ExcK::XRec** out) {
    std::lock_guard<std::mutex> lock(s->mu);
    auto it = k->xrec.find(G);
    if (it != k->xrec.end()) { *out = &it->second; return BAMM_OK; }
    const uint32_t maskY = (uint32_t)(ipow4(K + 1) - 1);
    ExcK::XRec x;
    x.h_B.resize(s->n);                                      // every element is written by the loop below
    x.h_lo.resize(s->n);
    RawVec<uint4> xrec(s->n);
    auto stream_y = [&](uint64_t n, int64_t pos) -> uint32_t {      // kmer_ mod 4^(K+1) as the stream alone gives it
        uint32_t y = 0;
        for (uint32_t d = 0; d <= K; d++) {
            const int64_t q = pos - (int64_t)d;
            if (q < 0) break;                                        // implicit A-padding (Sequence.cpp:35-41)
            const uint32_t w = s->h_words[s->h_word_off[n] + (uint64_t)(q >> 4)];
            y |= ((w >> (30u - 2u * (uint32_t)(q & 15))) & 3u) << (2u * d);
        }
        return y;
    };
    host_ranges(s->n, [&](uint64_t n_begin, uint64_t n_end) {
    for (uint64_t n = n_begin; n < n_end; n++) {
        const uint64_t e0 = k->h_off[n], e1 = k->h_off[n + 1];
        x.h_B[n] = 0; x.h_lo[n] = 0; xrec[n] = make_uint4(0, 0, 0, 0);
        if (e0 == e1) continue;
        const uint32_t lo = k->h_ex[e0].x, hi = k->h_ex[e1 - 1].x, L = s->h_len[n];
        const uint32_t hiB = std::min(hi + G - 1u, L - 1u);
        const uint32_t B = hiB - lo + 1u;
        // the record holds 12 seven-bit y fields (Y <= 64), or 9 ten-bit ones at K = 3 (Y = 256)
        const uint32_t max_fields = K == 3u ? 9u : 12u;
        if (B > 8u || B + G - 1u > max_fields || lo >= 4096u) { x.h_B[n] = 255; continue; }
        x.h_B[n] = (uint8_t)B;
        x.h_lo[n] = lo;
        uint32_t w3[3] = {0, 0, 0};
        uint64_t e = e0;
        for (uint32_t i = 0; i < B + G - 1u; i++) {
            const int64_t pos = (int64_t)lo - (int64_t)(G - 1u) + i;
            uint32_t y = maskY + 1u;                                 // no such position
            if (pos >= 0) {
                while (e < e1 && (int64_t)k->h_ex[e].x < pos) e++;
                y = (e < e1 && (int64_t)k->h_ex[e].x == pos) ? k->h_ex[e].y : stream_y(n, pos);
            }
            // the fields form ONE bit string over the three words, 7 bits each (10 at K = 3), field i at bit i * width:
            // a fix lane's consecutive fields are a single funnel shift of two neighbouring words (grouped_kernel.h: xrec_fields)
            const uint32_t bit = (K == 3u ? 10u : 7u) * i, wd = bit >> 5, sh = bit & 31u;
            w3[wd] |= y << sh;
            if (sh + (K == 3u ? 10u : 7u) > 32u) w3[wd + 1u] |= y >> (32u - sh);
        }
        xrec[n] = make_uint4(lo | (B << 12), w3[0], w3[1], w3[2]);
    }
    });
    DevBlocks made(s->ctx);
    int rc = made.upload(&x.d_xrec, xrec.data(), xrec.size());
    if (rc) return rc;
    if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) {
        set_error("stream sync failed while uploading the sequence records");
        return BAMM_ERR_HIP;
    }
    s->mem.adopt(made, x.d_xrec);
    auto ins = k->xrec.emplace(G, std::move(x));
    *out = &ins.first->second;
    return BAMM_OK;
}

}  // namespace bamm

using namespace bamm;

extern "C" {

// device arrays of a whole packed set that its maker already holds in `owner` (bamm_seqs_from_codes): the resident set adopts
// them instead of uploading the host copies again
struct AdoptDev { DevBlocks* owner; uint32_t* words; uint64_t* word_off; uint32_t* len; uint64_t* pos_off; };   // words: 80 words of slack behind the stream

static int seqs_upload_impl(bamm_ctx* c, const bamm_packed* p, uint64_t begin, uint64_t end, bamm_seqs** out, const AdoptDev* have) {
    if (!c || !p || !out || begin > end || end > p->n_seqs) {
        set_error("bamm_seqs_upload: bad argument");
        return BAMM_ERR_ARG;
    }
    if (end - begin > 0xfffffff0ull) { set_error("more than 2^32 sequences per device"); return BAMM_ERR_UNSUPPORTED; }
    BAMM_HIP(hipSetDevice(c->device));
    std::unique_ptr<bamm_seqs> s(new bamm_seqs(c));
    s->n = end - begin;
    const uint64_t w0 = p->word_off[begin], w1 = p->word_off[end];
    std::vector<uint64_t> woff(s->n + 1);
    s->h_len.assign(p->len + begin, p->len + end);
    s->h_pos_off.resize(s->n + 1);
    s->h_exc_off.resize(s->n + 1);
    const uint64_t e0 = p->exc_off[begin], e1 = p->exc_off[end];
    uint64_t pos = 0;
    s->min_len = s->n ? UINT32_MAX : 0;
    for (uint64_t n = 0; n < s->n; n++) {
        woff[n] = p->word_off[begin + n] - w0;
        s->h_pos_off[n] = pos;
        s->h_exc_off[n] = p->exc_off[begin + n] - e0;
        pos += s->h_len[n];
        s->max_len = std::max(s->max_len, s->h_len[n]);
        s->min_len = std::min(s->min_len, s->h_len[n]);
    }
    woff[s->n] = w1 - w0;
    s->h_words.resize(w1 - w0); par_memcpy(s->h_words.data(), p->words + w0, (w1 - w0) * sizeof(uint32_t));
    s->h_word_off = woff;
    s->h_pos_off[s->n] = pos;
    s->h_exc_off[s->n] = e1 - e0;
    s->total_len = pos;
    s->h_exc_pos.resize(e1 - e0); par_memcpy(s->h_exc_pos.data(), p->exc_pos + e0, (e1 - e0) * sizeof(uint32_t));
    s->h_exc_kmer.resize(e1 - e0); par_memcpy(s->h_exc_kmer.data(), p->exc_kmer + e0, (e1 - e0) * sizeof(uint32_t));
    s->h_exc_clean.resize(e1 - e0); par_memcpy(s->h_exc_clean.data(), p->exc_clean + e0, (e1 - e0) * sizeof(uint32_t));

    // length buckets: one kernel instantiation per positions-per-lane class
    // (+ one bucket for the sequences beyond the longest class: long_seq.hip walks those window by window)
    std::vector<std::vector<uint32_t>> members(kNumMClasses + 1);
    for (uint64_t n = 0; n < s->n; n++) {
        const int mc = m_class_for_len(s->h_len[n]);
        members[mc < 0 ? kNumMClasses : mc].push_back((uint32_t)n);
    }
    int rc;
    // 80 zero words of slack: the grouped kernel reads a lane's words without checking the sequence's end
    if (have && begin == 0 && end == p->n_seqs) {
        s->d_words = have->words; s->d_word_off = have->word_off; s->d_len = have->len; s->d_pos_off = have->pos_off;
        for (void* q : {(void*)s->d_words, (void*)s->d_word_off, (void*)s->d_len, (void*)s->d_pos_off}) s->mem.adopt(*have->owner, q);
        BAMM_HIP(hipMemsetAsync(s->d_words + (w1 - w0), 0, 80 * sizeof(uint32_t), c->stream));
    } else {
        if ((rc = s->mem.alloc(&s->d_words, (w1 - w0) + 80))) return rc;
        BAMM_HIP(hipMemsetAsync(s->d_words + (w1 - w0), 0, 80 * sizeof(uint32_t), c->stream));
        if ((rc = ctx_upload(c, s->d_words, p->words + w0, (w1 - w0) * sizeof(uint32_t)))) return rc;
        if ((rc = s->mem.upload(&s->d_word_off, woff.data(), woff.size()))) return rc;
        if ((rc = s->mem.upload(&s->d_len, s->h_len.data(), s->h_len.size()))) return rc;
        if ((rc = s->mem.upload(&s->d_pos_off, s->h_pos_off.data(), s->h_pos_off.size()))) return rc;
    }
    int used = 0;
    for (int mc = 0; mc <= kNumMClasses; mc++) used += !members[mc].empty();
    for (int mc = 0; mc <= kNumMClasses; mc++) {
        if (members[mc].empty()) continue;
        Bucket b;
        b.mclass = mc < kNumMClasses ? mc : kLongClass;
        b.count = (uint32_t)members[mc].size();
        if (mc < kNumMClasses) b.work = (double)b.count * kMClasses[mc];
        else for (uint32_t n : members[mc]) b.work += s->h_len[n] / 8.0;   // ~8x the cost per position of the fast kernels
        s->buckets.push_back(b);
        if (used > 1) {
            if ((rc = s->mem.upload(&s->buckets.back().d_idx, members[mc].data(), members[mc].size()))) return rc;
            s->buckets.back().h_idx = std::move(members[mc]);
        }
    }
    BAMM_HIP(hipStreamSynchronize(c->stream));
    s->hbm_bytes = (w1 - w0) * 4 + (s->n + 1) * 8 * 2 + s->n * 4;
    *out = s.release();
    return BAMM_OK;
}

int bamm_seqs_upload(bamm_ctx* c, const bamm_packed* p, uint64_t begin, uint64_t end, bamm_seqs** out) {
    const int rc = seqs_upload_impl(c, p, begin, end, out, nullptr);
    if (!rc) {                                               // where the set's unknown bases were, if its maker noted it (packed_set.h)
        (*out)->unk = packed_unknowns(p);
        (*out)->unk_begin = begin;
    }
    return rc;
}

// bamm_pack_codes_seeded on the device (csrc/prep.hip), then bamm_seqs_upload: the same packed set, the same resident set
int bamm_seqs_from_codes(bamm_ctx* c, const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int single_strand, uint32_t seed,
                         bamm_packed** packed_out, bamm_seqs** seqs_out) {
    if (!c || !packed_out || (n_seqs && (!codes || !off))) { set_error("bamm_seqs_from_codes: null argument"); return BAMM_ERR_ARG; }
    *packed_out = nullptr;
    if (seqs_out) *seqs_out = nullptr;
    if (n_seqs == 0) {
        int rc0 = bamm_pack_codes_seeded(codes, off, 0, single_strand, seed, packed_out);
        if (!rc0 && seqs_out) rc0 = bamm_seqs_upload(c, *packed_out, 0, 0, seqs_out);
        return rc0;
    }
    for (uint64_t n = 0; n < n_seqs; n++) {
        const uint64_t L0 = off[n + 1] - off[n];
        if ((single_strand ? L0 : 2 * L0 + 1) > 0xffffffffull) { set_error("sequence %llu longer than 2^32-1", (unsigned long long)n); return BAMM_ERR_ARG; }
    }
    BAMM_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const uint64_t n_codes = off[n_seqs] - off[0];
    DevBlocks tmp(c);                                        // everything allocated here is freed on every path out
    int rc;
    uint8_t* d_codes = nullptr;
    uint64_t* d_off = nullptr;
    PrepArgs a{};
    if ((rc = tmp.alloc(&d_codes, n_codes)) || (rc = tmp.alloc(&d_off, n_seqs + 1))) return rc;
    {
        // the records as one contiguous run starting at 0 (off[0] may be anything)
        std::vector<uint64_t> rel(n_seqs + 1);
        for (uint64_t n = 0; n <= n_seqs; n++) rel[n] = off[n] - off[0];
        if (ctx_upload(c, d_codes, codes + off[0], n_codes) != BAMM_OK || ctx_upload(c, d_off, rel.data(), (n_seqs + 1) * sizeof(uint64_t)) != BAMM_OK ||
            hipStreamSynchronize(st) != hipSuccess) { set_error("bamm_seqs_from_codes: upload failed"); return BAMM_ERR_HIP; }
    }
    a.codes = d_codes; a.off = d_off; a.n = n_seqs; a.single_strand = single_strand;
    if ((rc = tmp.alloc(&a.len, n_seqs)) || (rc = tmp.alloc(&a.word_off, n_seqs + 1)) || (rc = tmp.alloc(&a.pos_off, n_seqs + 1)) ||
        (rc = tmp.alloc(&a.zero_off, n_seqs + 1)) || (rc = tmp.alloc(&a.draw_off, n_seqs + 1)) || (rc = tmp.alloc(&a.exc_off, n_seqs + 1))) return rc;
    for (uint64_t* p : {a.word_off, a.pos_off, a.zero_off, a.draw_off, a.exc_off})
        if (hipMemsetAsync(p, 0, sizeof(uint64_t), st) != hipSuccess) { set_error("hipMemsetAsync failed"); return BAMM_ERR_HIP; }
    if ((rc = launch_prep_count(a, st))) return rc;
    for (uint64_t* p : {a.word_off, a.pos_off, a.zero_off, a.draw_off})
        if ((rc = launch_scan_u64(p, n_seqs + 1, st))) return rc;
    uint64_t tot[4] = {0, 0, 0, 0};                          // words, positions, zeros, draws
    {
        uint64_t* src[4] = {a.word_off, a.pos_off, a.zero_off, a.draw_off};
        for (int i = 0; i < 4; i++)
            if (hipMemcpyAsync(&tot[i], src[i] + n_seqs, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess) { set_error("read-back failed"); return BAMM_ERR_HIP; }
        if (hipStreamSynchronize(st) != hipSuccess) { set_error("bamm_seqs_from_codes: the counting pass failed"); return BAMM_ERR_HIP; }
    }
    uint8_t* d_draws = nullptr;
    if ((rc = tmp.alloc(&a.zero_pos, tot[2])) || (rc = tmp.alloc(&d_draws, tot[3]))) return rc;
    if ((rc = launch_prep_zeros(a, st))) return rc;
    {
        // the one serial resource of Sequence::Sequence is libc's rand() stream: the draws are taken on the host (all
        // threads enter the stream by jump-ahead, pack.cpp) while the device lists the zero positions
        std::vector<uint8_t> draws(tot[3] ? tot[3] : 1);
        rand_draws_mod4(seed, tot[3], draws.data());
        if (tot[3] && (ctx_upload(c, d_draws, draws.data(), tot[3]) != BAMM_OK || hipStreamSynchronize(st) != hipSuccess)) {
            set_error("bamm_seqs_from_codes: upload of the draws failed"); return BAMM_ERR_HIP;
        }
    }
    a.draws = d_draws;
    if ((rc = launch_prep_pack(a, false, st)) || (rc = launch_scan_u64(a.exc_off, n_seqs + 1, st))) return rc;
    uint64_t n_exc = 0;
    if (hipMemcpyAsync(&n_exc, a.exc_off + n_seqs, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        set_error("bamm_seqs_from_codes: the exception count failed"); return BAMM_ERR_HIP;
    }
    if ((rc = tmp.alloc(&a.words, tot[0] + 80)) || (rc = tmp.alloc(&a.exc_pos, n_exc)) || (rc = tmp.alloc(&a.exc_kmer, n_exc)) || (rc = tmp.alloc(&a.exc_clean, n_exc))) return rc;
    if ((rc = launch_prep_pack(a, true, st))) return rc;
    // the host's view of the packed set (malloc: bamm_packed_free releases it)
    bamm_packed* p = (bamm_packed*)calloc(1, sizeof(bamm_packed));
    if (!p) { set_error("out of memory"); return BAMM_ERR_ARG; }
    p->n_seqs = n_seqs; p->n_words = tot[0]; p->n_exc = n_exc; p->total_len = tot[1];
    p->words = (uint32_t*)malloc((tot[0] ? tot[0] : 1) * sizeof(uint32_t));
    p->word_off = (uint64_t*)malloc((n_seqs + 1) * sizeof(uint64_t));
    p->len = (uint32_t*)malloc(n_seqs * sizeof(uint32_t));
    p->exc_off = (uint64_t*)malloc((n_seqs + 1) * sizeof(uint64_t));
    p->exc_pos = (uint32_t*)calloc(n_exc ? n_exc : 1, sizeof(uint32_t));
    p->exc_kmer = (uint32_t*)calloc(n_exc ? n_exc : 1, sizeof(uint32_t));
    p->exc_clean = (uint32_t*)calloc(n_exc ? n_exc : 1, sizeof(uint32_t));
    bool ok = p->words && p->word_off && p->len && p->exc_off && p->exc_pos && p->exc_kmer && p->exc_clean;
    auto down = [&](void* dst, const void* src, size_t bytes) { if (ok && bytes) ok = ctx_download(c, dst, src, bytes) == BAMM_OK; };
    down(p->words, a.words, tot[0] * sizeof(uint32_t));
    down(p->word_off, a.word_off, (n_seqs + 1) * sizeof(uint64_t));
    down(p->len, a.len, n_seqs * sizeof(uint32_t));
    down(p->exc_off, a.exc_off, (n_seqs + 1) * sizeof(uint64_t));
    down(p->exc_pos, a.exc_pos, n_exc * sizeof(uint32_t));
    down(p->exc_kmer, a.exc_kmer, n_exc * sizeof(uint32_t));
    down(p->exc_clean, a.exc_clean, n_exc * sizeof(uint32_t));
    if (ok) ok = hipStreamSynchronize(st) == hipSuccess;
    if (!ok) { bamm_packed_free(p); set_error("bamm_seqs_from_codes: the packed set could not be brought back"); return BAMM_ERR_HIP; }
    uint32_t mx = 0, mn = UINT32_MAX;
    for (uint64_t n = 0; n < n_seqs; n++) { mx = std::max(mx, p->len[n]); mn = std::min(mn, p->len[n]); }
    p->max_len = mx; p->min_len = mn;
    if (seqs_out) {
        // the stream, its offsets and the lengths are on the device already: the resident set takes those arrays over
        const AdoptDev have{&tmp, a.words, a.word_off, a.len, a.pos_off};
        if ((rc = seqs_upload_impl(c, p, 0, n_seqs, seqs_out, &have))) { bamm_packed_free(p); return rc; }
    }
    *packed_out = p;
    return BAMM_OK;
}

// BackgroundModel's counting pass over a resident set (BackgroundModel.cpp:26-42), calculateV on the host (:441-473)
int bamm_seqs_bg_model(bamm_ctx* c, bamm_seqs* s, uint32_t K, const float* alpha, float* vbg_out) {
    if (!c || !s || !alpha || !vbg_out || K > BAMM_MAX_ORDER) { set_error("bamm_seqs_bg_model: bad argument"); return BAMM_ERR_ARG; }
    if (s->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    const size_t Y = ipow4(K + 1);
    std::vector<uint64_t> top(Y, 0);
    if (s->n) {
        BAMM_HIP(hipSetDevice(c->device));
        ExcK* exc = nullptr;
        int rc = exceptions_for_order(s, K, &exc);
        if (rc) return rc;
        DevBlocks tmp(c);
        unsigned long long* d_counts = nullptr;
        if ((rc = tmp.alloc(&d_counts, Y))) return rc;
        hipError_t e = hipMemsetAsync(d_counts, 0, Y * sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) rc = launch_bg_counts(s->d_words, s->d_word_off, s->d_len, exc->d_off, exc->d_exc, s->n, K, d_counts,
                                                   (uint32_t)std::max(1, c->num_cus), c->stream);
        if (e == hipSuccess && !rc) e = hipMemcpyAsync(top.data(), d_counts, Y * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && !rc) e = hipStreamSynchronize(c->stream);
        if (rc) return rc;
        if (e != hipSuccess) { set_error("bamm_seqs_bg_model: %s", hipGetErrorString(e)); return BAMM_ERR_HIP; }
    }
    bg_from_top_counts(top.data(), K, alpha, vbg_out);
    return BAMM_OK;
}

int bamm_seqs_destroy(bamm_seqs* s) {
    if (!s) return BAMM_OK;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        if (--s->refs > 0) return BAMM_OK;
    }
    (void)hipSetDevice(s->ctx->device);
    delete s;
    return BAMM_OK;
}

int bamm_seqs_info(const bamm_seqs* s, uint64_t* n_seqs, uint64_t* total_len, uint32_t* max_len, uint64_t* hbm_bytes) {
    if (!s) { set_error("null seqs"); return BAMM_ERR_ARG; }
    if (n_seqs) *n_seqs = s->n;
    if (total_len) *total_len = s->total_len;
    if (max_len) *max_len = s->max_len;
    if (hbm_bytes) *hbm_bytes = s->hbm_bytes;
    return BAMM_OK;
}

}  // extern "C"
