// bamm_fdr: FDR::calculatePR's MOPS branch and FDR::calculatePvalues (FDR.cpp:156-196, :278-333) over window scores that
// never leave the device.  The folds of one motif append their scores (k_score's output, or arrays the caller holds);
// bamm_fdr_statistics sorts both lists in place (occ.hip's radix sort) and runs the peak kernels (fdr.hip); rows and
// p-values are then computed range by range and downloaded through the context's staging area.  Folds that ran on several
// contexts collect on a handle each: bamm_fdr_seal sorts a handle's lists into runs where they lie, bamm_fdr_absorb moves
// them to the handle that computes the statistics, which merges the runs (k_fdr_merge) instead of sorting again.  Host code only.

#include "handles.h"
#include "fdr_rows.h"

using namespace bamm;

namespace {

constexpr uint64_t kFdrMaxScores = 0xffffffffull;            // the sort's index width
constexpr uint64_t kFdrChunkRows = uint64_t(1) << 22;        // rows computed and downloaded at a time: 16 MB per column

const char* list_name(int which) { return which ? "negative" : "positive"; }

// room for `extra` more scores in list `which`: a new block of at least twice the size, the old scores copied across
int fdr_reserve(bamm_fdr* h, int which, uint64_t extra) {
    const uint64_t need = h->n[which] + extra;
    if (need > kFdrMaxScores) {
        set_error("bamm_fdr: %llu %s scores, the limit is 2^32 - 1 = 4294967295", (unsigned long long)need, list_name(which));
        return BAMM_ERR_UNSUPPORTED;
    }
    if (need <= h->cap[which]) return BAMM_OK;
    const uint64_t cap = std::min(kFdrMaxScores, std::max(need, 2 * h->cap[which]));
    float* grown = nullptr;
    if (int rc = scratch_alloc(h->ctx, &grown, (size_t)cap)) return rc;
    if (h->n[which]) {
        const hipError_t e = hipMemcpyAsync(grown, h->d[which], h->n[which] * sizeof(float), hipMemcpyDeviceToDevice, h->ctx->stream);
        if (e != hipSuccess) { scratch_free(h->ctx, grown); set_error("hipMemcpyAsync failed: %s", hipGetErrorString(e)); return BAMM_ERR_HIP; }
    }
    scratch_free(h->ctx, h->d[which]);                       // its next owner is ordered behind the copy on the context's one stream
    h->d[which] = grown;
    h->cap[which] = cap;
    return BAMM_OK;
}

// statistics may still run on a sealed handle; nothing but destroy is left for one that was absorbed
int fdr_open_for_statistics(const bamm_fdr* h, const char* fn) {
    if (!h) { set_error("%s: null argument", fn); return BAMM_ERR_ARG; }
    if (h->done) { set_error("%s: the statistics were computed, the handle accepts no more scores", fn); return BAMM_ERR_STATE; }
    if (h->moved) { set_error("%s: the handle was absorbed by another, it can only be destroyed", fn); return BAMM_ERR_STATE; }
    return BAMM_OK;
}

int fdr_open_for_scores(const bamm_fdr* h, const char* fn) {
    if (int rc = fdr_open_for_statistics(h, fn)) return rc;
    if (h->sealed) { set_error("%s: the handle is sealed, it accepts no more scores", fn); return BAMM_ERR_STATE; }
    return BAMM_OK;
}

// `count` scores now lie behind list `which`: a run of their own, or part of the open piece at its end
void fdr_appended(bamm_fdr* h, int which, uint64_t count, bool run) {
    if (!count) return;
    auto& p = h->pieces[which];
    if (!run && !p.empty() && !p.back().run) p.back().len += count; else p.push_back(bamm_fdr::Piece{count, run});
    h->n[which] += count;
}

// List `which` as ONE ascending run: every open piece sorted where it lies (launch_occ_sort), then the runs merged two by
// two, pass by pass, between the list and the second buffer the sort already took from the pool -- ceil(log2 runs)
// streaming passes; a run without a partner is copied.  The list ends in whichever buffer the last pass wrote.
int fdr_one_run(bamm_fdr* h, int which, DevBlocks& tmp) {
    auto& pieces = h->pieces[which];
    const uint64_t n = h->n[which];
    if (!n || (pieces.size() == 1 && pieces[0].run)) return BAMM_OK;
    bamm_ctx* c = h->ctx;
    hipStream_t st = c->stream;
    int rc;
    DevBlocks sort_tmp(c);                                   // the second buffer goes back to the pool once the launches are queued
    uint32_t* d_alt = nullptr;
    if ((rc = sort_tmp.scratch(&d_alt, (size_t)n))) return rc;
    uint64_t at = 0;
    for (auto& p : pieces) {                                 // ascending, as calculatePvalues wants them; the walk reads from the top
        if (!p.run) {
            uint32_t* d_hist = nullptr;
            const uint32_t len = (uint32_t)p.len, blocks = occ_sort_blocks(len, (uint32_t)std::max(1, c->num_cus));
            if ((rc = tmp.alloc(&d_hist, (size_t)256 * blocks)) || (rc = launch_occ_sort(h->d[which] + at, d_alt, d_hist, len, blocks, st))) return rc;
            p.run = true;
        }
        at += p.len;
    }
    if (pieces.size() == 1) return BAMM_OK;
    uint64_t* d_part = nullptr;
    if ((rc = tmp.alloc(&d_part, (size_t)(n / kFdrStepsPerBlock + 2)))) return rc;
    float *src = h->d[which], *dst = reinterpret_cast<float*>(d_alt);
    std::vector<uint64_t> len, next;
    for (const auto& p : pieces) len.push_back(p.len);
    while (len.size() > 1) {
        next.clear();
        at = 0;
        for (size_t i = 0; i < len.size(); i += 2) {
            const uint64_t both = len[i] + (i + 1 < len.size() ? len[i + 1] : 0);
            if (i + 1 < len.size()) {
                if ((rc = launch_fdr_merge(FdrMergeArgs{src + at, src + at + len[i], len[i], len[i + 1], dst + at, d_part}, st))) return rc;
            } else {
                BAMM_HIP(hipMemcpyAsync(dst + at, src + at, both * sizeof(float), hipMemcpyDeviceToDevice, st));
            }
            next.push_back(both);
            at += both;
        }
        std::swap(src, dst);
        len.swap(next);
    }
    if (src != h->d[which]) {                                // the buffers change roles: the list's old block goes back to the pool
        sort_tmp.keep(d_alt);
        scratch_free(c, h->d[which]);
        h->d[which] = src;
        h->cap[which] = n;
    }
    pieces.assign(1, bamm_fdr::Piece{n, true});
    return BAMM_OK;
}

// `n` floats from one context's device to another's that it cannot reach directly: through the two pinned staging areas
// (ctx_download / ctx_upload), a chunk at a time; the hop between them is touched by the host's memcpy only
int fdr_relay(bamm_ctx* dc, float* to, bamm_ctx* sc, const float* from, uint64_t n) {
    std::vector<float> hop((size_t)std::min(n, kFdrChunkRows));
    for (uint64_t at = 0; at < n; at += hop.size()) {
        const size_t bytes = (size_t)std::min<uint64_t>(hop.size(), n - at) * sizeof(float);
        int rc;
        BAMM_HIP(hipSetDevice(sc->device));
        if ((rc = ctx_download(sc, hop.data(), from + at, bytes))) return rc;
        BAMM_HIP(hipStreamSynchronize(sc->stream));          // a short tail is only enqueued
        BAMM_HIP(hipSetDevice(dc->device));
        if ((rc = ctx_upload(dc, to + at, hop.data(), bytes))) return rc;
    }
    return BAMM_OK;
}

// an event on a context's stream that other streams wait for; destroyed with its owner (the runtime keeps what is enqueued)
struct StreamMark {
    hipEvent_t ev = nullptr;
    ~StreamMark() { if (ev) (void)hipEventDestroy(ev); }
    // everything enqueued on `waiter`'s stream from now on runs behind what `of`'s stream holds now
    int order(bamm_ctx* waiter, bamm_ctx* of) {
        BAMM_HIP(hipSetDevice(of->device));
        BAMM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        BAMM_HIP(hipEventRecord(ev, of->stream));
        BAMM_HIP(hipSetDevice(waiter->device));
        BAMM_HIP(hipStreamWaitEvent(waiter->stream, ev, 0));
        return BAMM_OK;
    }
};

int fdr_range(const bamm_fdr* h, const char* fn, uint64_t begin, uint64_t end, uint64_t n, const char* what) {
    if (!h) { set_error("%s: null argument", fn); return BAMM_ERR_ARG; }
    if (!h->done) { set_error("%s before bamm_fdr_statistics", fn); return BAMM_ERR_STATE; }
    if (begin > end || end > n) {
        set_error("%s: [%llu, %llu) is outside the %llu %s", fn, (unsigned long long)begin, (unsigned long long)end, (unsigned long long)n, what);
        return BAMM_ERR_ARG;
    }
    return BAMM_OK;
}

}  // namespace

extern "C" {

int bamm_fdr_create(bamm_ctx* c, bamm_fdr** out) {
    if (!c || !out) { set_error("bamm_fdr_create: null argument"); return BAMM_ERR_ARG; }
    *out = new bamm_fdr;
    (*out)->ctx = c;
    return BAMM_OK;
}

int bamm_fdr_geometry(uint32_t* steps_per_thread, uint32_t* steps_per_block) {
    if (steps_per_thread) *steps_per_thread = kFdrStepsPerThread;
    if (steps_per_block) *steps_per_block = kFdrStepsPerBlock;
    return BAMM_OK;
}

int bamm_fdr_add_set(bamm_fdr* h, int negative, bamm_seqs* set, const uint8_t* seq_mask, uint32_t K, uint32_t W, uint32_t bg_order,
                     const float* v, const float* vbg) {
    if (int rc = fdr_open_for_scores(h, "bamm_fdr_add_set")) return rc;
    if (!set || !v || !vbg) { set_error("bamm_fdr_add_set: null argument"); return BAMM_ERR_ARG; }
    if (K > BAMM_MAX_ORDER || W == 0) { set_error("bamm_fdr_add_set: bad K/W"); return BAMM_ERR_ARG; }
    if (set->ctx != h->ctx) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    if (set->n && set->min_len < W) { set_error("a sequence is shorter than the motif (W=%u)", W); return BAMM_ERR_ARG; }
    const int which = negative ? 1 : 0;
    bamm_ctx* c = h->ctx;
    uint64_t total = 0, n_sel = 0;
    for (uint64_t n = 0; n < set->n; n++)
        if (!seq_mask || seq_mask[n]) { total += set->h_len[n] - W + 1; n_sel++; }
    if (!total) return BAMM_OK;
    BAMM_HIP(hipSetDevice(c->device));
    if (int rc = fdr_reserve(h, which, total)) return rc;    // refuses a list beyond the sort's index width before anything is scored
    DevBlocks tmp(c);
    DeviceScores sc;
    int rc = score_on_device(c, set, seq_mask, K, W, bg_order, v, vbg, kWantMops, kPooledMops, tmp, &sc);
    if (rc) return rc;
    float* dst = h->d[which] + h->n[which];
    if (!seq_mask) {
        BAMM_HIP(hipMemcpyAsync(dst, sc.mops, total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    } else {                                                 // the selected sequences' windows, packed
        std::vector<FdrSeg> seg;
        seg.reserve((size_t)n_sel);
        uint64_t at = 0;
        for (uint64_t n = 0; n < set->n; n++) {
            if (!seq_mask[n]) continue;
            const uint32_t len = set->h_len[n] - W + 1;
            seg.push_back(FdrSeg{sc.moff[n], at, len, 0u});
            at += len;
        }
        FdrSeg* d_seg = nullptr;
        if ((rc = tmp.upload(&d_seg, seg.data(), seg.size()))) return rc;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((seg.size() + 3) / 4, (uint64_t)std::max(1, c->num_cus) * 8u);
        if ((rc = launch_fdr_gather(sc.mops, dst, d_seg, (uint32_t)seg.size(), blocks, c->stream))) return rc;
    }
    fdr_appended(h, which, total, false);
    return BAMM_OK;
}

int bamm_fdr_add_scores(bamm_fdr* h, int negative, const float* scores, uint64_t n) {
    if (int rc = fdr_open_for_scores(h, "bamm_fdr_add_scores")) return rc;
    if (!scores && n) { set_error("bamm_fdr_add_scores: null argument"); return BAMM_ERR_ARG; }
    if (!n) return BAMM_OK;
    const int which = negative ? 1 : 0;
    BAMM_HIP(hipSetDevice(h->ctx->device));
    int rc;
    if ((rc = fdr_reserve(h, which, n)) || (rc = ctx_upload(h->ctx, h->d[which] + h->n[which], scores, n * sizeof(float)))) return rc;
    fdr_appended(h, which, n, false);
    return BAMM_OK;
}

int bamm_fdr_seal(bamm_fdr* h) {
    if (!h) { set_error("bamm_fdr_seal: null argument"); return BAMM_ERR_ARG; }
    if (h->done) { set_error("bamm_fdr_seal: the handle is past bamm_fdr_statistics"); return BAMM_ERR_ARG; }
    if (h->moved) { set_error("bamm_fdr_seal: the handle was absorbed by another, it can only be destroyed"); return BAMM_ERR_ARG; }
    if (h->sealed) return BAMM_OK;
    bamm_ctx* c = h->ctx;
    BAMM_HIP(hipSetDevice(c->device));
    int rc;
    {
        DevBlocks tmp(c);
        if ((rc = fdr_one_run(h, 0, tmp)) || (rc = fdr_one_run(h, 1, tmp))) return rc;
        BAMM_HIP(hipStreamSynchronize(c->stream));           // the runs are in place when the call returns
    }
    h->sealed = true;
    return BAMM_OK;
}

int bamm_fdr_absorb(bamm_fdr* dst, bamm_fdr* src) {
    if (!dst || !src) { set_error("bamm_fdr_absorb: null argument"); return BAMM_ERR_ARG; }
    if (dst == src) { set_error("bamm_fdr_absorb: a handle cannot absorb itself"); return BAMM_ERR_ARG; }
    for (const bamm_fdr* h : {dst, src}) {
        const char* who = h == dst ? "destination" : "source";
        if (h->done) { set_error("bamm_fdr_absorb: the %s is past bamm_fdr_statistics", who); return BAMM_ERR_ARG; }
        if (h->moved) { set_error("bamm_fdr_absorb: the %s was absorbed by another handle, it can only be destroyed", who); return BAMM_ERR_ARG; }
    }
    if (dst->sealed) { set_error("bamm_fdr_absorb: the destination is sealed, it accepts no more scores"); return BAMM_ERR_ARG; }
    for (int which = 0; which < 2; which++)
        if (dst->n[which] + src->n[which] > kFdrMaxScores) {
            set_error("bamm_fdr_absorb: %llu %s scores, the limit is 2^32 - 1 = 4294967295",
                      (unsigned long long)(dst->n[which] + src->n[which]), list_name(which));
            return BAMM_ERR_ARG;
        }
    bamm_ctx *dc = dst->ctx, *sc = src->ctx;
    const bool same_ctx = dc == sc, same_device = dc->device == sc->device;
    int direct = 1;                                          // the copy engine reaches src's memory from dst's device
    if (!same_device) BAMM_HIP(hipDeviceCanAccessPeer(&direct, dc->device, sc->device));
    // a list that arrives on its own context at an empty one brings its block along: nothing is copied
    auto takes_block = [&](int which) { return same_ctx && !dst->n[which]; };
    const bool copies = (src->n[0] && !takes_block(0)) || (src->n[1] && !takes_block(1));
    const bool ordered = copies && !same_ctx && direct;      // same context: one stream; staged: ctx_download waits for src's stream
    StreamMark filled, copied;
    int rc;
    if (ordered && (rc = filled.order(dc, sc))) return rc;
    BAMM_HIP(hipSetDevice(dc->device));
    for (int which = 0; which < 2; which++) {
        const uint64_t n = src->n[which];
        if (!n) continue;
        if (takes_block(which)) {
            scratch_free(dc, dst->d[which]);
            dst->d[which] = src->d[which]; dst->cap[which] = src->cap[which];
            src->d[which] = nullptr;
        } else {
            if ((rc = fdr_reserve(dst, which, n))) return rc;
            float* to = dst->d[which] + dst->n[which];
            if (same_device) BAMM_HIP(hipMemcpyAsync(to, src->d[which], n * sizeof(float), hipMemcpyDeviceToDevice, dc->stream));
            else if (direct) BAMM_HIP(hipMemcpyPeerAsync(to, dc->device, src->d[which], sc->device, n * sizeof(float), dc->stream));
            else if ((rc = fdr_relay(dc, to, sc, src->d[which], n))) return rc;
        }
        for (const auto& p : src->pieces[which]) fdr_appended(dst, which, p.len, p.run);
    }
    // src's blocks go back to its context's pool: their next owner there is ordered behind dst's copies
    if (ordered && (rc = copied.order(sc, dc))) return rc;
    (void)hipSetDevice(sc->device);
    for (int which = 0; which < 2; which++) {
        scratch_free(sc, src->d[which]);
        src->d[which] = nullptr;
        src->n[which] = src->cap[which] = 0;
        src->pieces[which].clear();
    }
    src->moved = true;
    return BAMM_OK;
}

int bamm_fdr_statistics(bamm_fdr* h, uint64_t posN, uint64_t negN, int with_pvalues) {
    if (int rc = fdr_open_for_statistics(h, "bamm_fdr_statistics")) return rc;
    const uint64_t total = h->n[0] + h->n[1];
    if (!total) { set_error("bamm_fdr_statistics: no score was added"); return BAMM_ERR_STATE; }
    bamm_ctx* c = h->ctx;
    BAMM_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc;
    DevBlocks tmp(c);
    if ((rc = fdr_one_run(h, 0, tmp)) || (rc = fdr_one_run(h, 1, tmp))) return rc;
    FdrWalkArgs& w = h->walk;
    w.pos = h->d[0]; w.neg = h->d[1]; w.n_pos = h->n[0]; w.n_neg = h->n[1];
    w.m_fold = fdr_mfold(posN, negN);
    w.n_blocks = (total + kFdrStepsPerBlock - 1) / kFdrStepsPerBlock;
    if ((rc = scratch_alloc(c, &w.part, (size_t)w.n_blocks + 1)) || (rc = scratch_alloc(c, &w.block_max, (size_t)w.n_blocks)) ||
        (rc = dev_alloc(&w.peak, 1))) return rc;
    BAMM_HIP(hipMemsetAsync(w.peak, 0, sizeof(FdrPeak), st));
    FdrPeak peak{};
    if ((rc = launch_fdr_peak(w, st)) || (rc = ctx_download(c, &peak, w.peak, sizeof peak))) return rc;
    BAMM_HIP(hipStreamSynchronize(st));
    const uint64_t idx_max = peak.last_eq ? peak.last_eq - 1 : posN + negN;   // FDR.cpp:164: sequence counts, not window counts
    h->posN = posN; h->negN = negN;
    h->e_tp = peak.e_tp;
    h->n_rows = std::min(idx_max, total);
    h->with_pvalues = with_pvalues != 0;
    h->done = true;
    return BAMM_OK;
}

int bamm_fdr_info(const bamm_fdr* h, uint64_t* n_pos, uint64_t* n_neg, uint64_t* n_rows, float* e_tp, float* occ_mult) {
    if (!h) { set_error("bamm_fdr_info: null argument"); return BAMM_ERR_ARG; }
    if (n_pos) *n_pos = h->n[0];
    if (n_neg) *n_neg = h->n[1];
    if (n_rows) *n_rows = h->n_rows;
    if (e_tp) *e_tp = h->e_tp;
    if (occ_mult) *occ_mult = h->done ? h->e_tp / (float)h->posN : 0.0f;   // FDR.cpp:195
    return BAMM_OK;
}

int bamm_fdr_rows(bamm_fdr* h, uint64_t begin, uint64_t end, float* tp, float* fp, float* fdr, float* rec) {
    if (int rc = fdr_range(h, "bamm_fdr_rows", begin, end, h ? h->n_rows : 0, "rows")) return rc;
    bamm_ctx* c = h->ctx;
    BAMM_HIP(hipSetDevice(c->device));
    float* host[4] = {tp, fp, fdr, rec};
    float* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBlocks tmp(c);
    int rc;
    const uint64_t chunk = std::min(kFdrChunkRows, end - begin);
    for (int k = 0; k < 4; k++)
        if (host[k] && chunk && (rc = tmp.scratch(&dev[k], (size_t)chunk))) return rc;
    for (uint64_t at = begin; at < end; at += chunk) {
        const uint64_t stop = std::min(end, at + chunk);
        if ((rc = launch_fdr_rows(h->walk, at, stop, h->e_tp, dev[0], dev[1], dev[2], dev[3], c->stream))) return rc;
        for (int k = 0; k < 4; k++)
            if (host[k] && (rc = ctx_download(c, host[k] + (at - begin), dev[k], (stop - at) * sizeof(float)))) return rc;
        BAMM_HIP(hipStreamSynchronize(c->stream));           // the next chunk overwrites the device buffers
    }
    return BAMM_OK;
}

int bamm_fdr_pvalues(bamm_fdr* h, uint64_t begin, uint64_t end, float* p) {
    if (int rc = fdr_range(h, "bamm_fdr_pvalues", begin, end, h ? h->n[0] : 0, "positive scores")) return rc;
    if (!h->with_pvalues) { set_error("bamm_fdr_pvalues: bamm_fdr_statistics was called without with_pvalues"); return BAMM_ERR_STATE; }
    if (!p && end > begin) { set_error("bamm_fdr_pvalues: null argument"); return BAMM_ERR_ARG; }
    bamm_ctx* c = h->ctx;
    BAMM_HIP(hipSetDevice(c->device));
    DevBlocks tmp(c);
    float* d_p = nullptr;
    int rc;
    const uint64_t chunk = std::min(kFdrChunkRows, end - begin);
    if (chunk && (rc = tmp.scratch(&d_p, (size_t)chunk))) return rc;
    for (uint64_t at = begin; at < end; at += chunk) {
        const uint64_t stop = std::min(end, at + chunk);
        if ((rc = launch_fdr_pvalues(h->d[0], h->d[1], h->n[1], at, stop, d_p, c->stream)) ||
            (rc = ctx_download(c, p + (at - begin), d_p, (stop - at) * sizeof(float)))) return rc;
        BAMM_HIP(hipStreamSynchronize(c->stream));
    }
    return BAMM_OK;
}

int bamm_fdr_destroy(bamm_fdr* h) {
    if (!h) return BAMM_OK;
    (void)hipSetDevice(h->ctx->device);
    for (void* p : {(void*)h->d[0], (void*)h->d[1], (void*)h->walk.part, (void*)h->walk.block_max, (void*)h->walk.peak}) scratch_free(h->ctx, p);
    delete h;
    return BAMM_OK;
}

}  // extern "C"
