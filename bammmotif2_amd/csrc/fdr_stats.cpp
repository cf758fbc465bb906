// bamm_fdr: FDR::calculatePR's MOPS branch and FDR::calculatePvalues (FDR.cpp:156-196, :278-333) over window scores that
// never leave the device.  The folds of one motif append their scores (k_score's output, or arrays the caller holds);
// bamm_fdr_statistics sorts both lists in place (occ.hip's radix sort) and runs the peak kernels (fdr.hip); rows and
// p-values are then computed range by range and downloaded through the context's staging area.  Host code only.

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

int fdr_open_for_scores(const bamm_fdr* h, const char* fn) {
    if (!h) { set_error("%s: null argument", fn); return BAMM_ERR_ARG; }
    if (h->done) { set_error("%s: the statistics were computed, the handle accepts no more scores", fn); return BAMM_ERR_STATE; }
    return BAMM_OK;
}

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
    DevTemps tmp(c);
    DeviceScores sc;
    int rc = score_on_device(c, set, seq_mask, K, W, bg_order, v, vbg, true, true, tmp, &sc);
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
    h->n[which] += total;
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
    h->n[which] += n;
    return BAMM_OK;
}

int bamm_fdr_statistics(bamm_fdr* h, uint64_t posN, uint64_t negN, int with_pvalues) {
    if (int rc = fdr_open_for_scores(h, "bamm_fdr_statistics")) return rc;
    const uint64_t total = h->n[0] + h->n[1];
    if (!total) { set_error("bamm_fdr_statistics: no score was added"); return BAMM_ERR_STATE; }
    bamm_ctx* c = h->ctx;
    BAMM_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc;
    DevTemps tmp(c);
    for (int which = 0; which < 2; which++) {                // ascending, as calculatePvalues wants them; the walk reads from the top
        if (!h->n[which]) continue;
        DevTemps sort_tmp(c);                                // the second buffer goes back to the pool once the launches are queued
        uint32_t *d_alt = nullptr, *d_hist = nullptr;
        const uint32_t n = (uint32_t)h->n[which], blocks = occ_sort_blocks(n, (uint32_t)std::max(1, c->num_cus));
        if ((rc = sort_tmp.scratch(&d_alt, (size_t)n)) || (rc = tmp.alloc(&d_hist, (size_t)256 * blocks)) ||
            (rc = launch_occ_sort(h->d[which], d_alt, d_hist, n, blocks, st))) return rc;
    }
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
    DevTemps tmp(c);
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
    DevTemps tmp(c);
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
