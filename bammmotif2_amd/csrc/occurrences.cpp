// bamm_occurrences: ScoreSeqSet::calcPvalues + the cut of ScoreSeqSet::write (seq_scoring/ScoreSeqSet.cpp:70-126,
// :245-291) over two resident sets.  Scores, the sorted negatives and the ranking stay on the device (occ.hip); the
// host sees nTop + 1 negative scores, a counter and the candidate windows, and evaluates the reference's formula on
// those with the function the host path uses (occ_pvalue.h).  Host code only.

#include "handles.h"
#include "occ_pvalue.h"

using namespace bamm;

struct bamm_occ {
    std::vector<uint64_t> seq, fp;
    std::vector<uint32_t> pos;
    std::vector<float> score, p, e;
    OccScalars sc;
    uint64_t n_candidates = 0;
};

extern "C" {

int bamm_occurrences(bamm_ctx* c, bamm_seqs* positives, bamm_seqs* negatives, uint32_t K, uint32_t W, uint32_t bg_order,
                     const float* v, const float* vbg, float p_cutoff, bamm_occ** out) {
    if (!c || !positives || !negatives || !v || !vbg || !out) { set_error("bamm_occurrences: null argument"); return BAMM_ERR_ARG; }
    *out = nullptr;
    if (K > BAMM_MAX_ORDER || W == 0) { set_error("bamm_occurrences: bad K/W"); return BAMM_ERR_ARG; }
    if (positives->ctx != c || negatives->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    if ((positives->n && positives->min_len < W) || (negatives->n && negatives->min_len < W)) {
        set_error("a sequence is shorter than the motif (W=%u)", W);
        return BAMM_ERR_ARG;
    }
    uint64_t negN = 0;
    for (uint64_t n = 0; n < negatives->n; n++) negN += negatives->h_len[n] - W + 1;
    if (negN == 0) { set_error("bamm_occurrences: the negative set is empty"); return BAMM_ERR_ARG; }
    if (negN > 2147483647ull) {                              // ScoreSeqSet.cpp:87 computes nTop from (int)negN
        set_error("bamm_occurrences: %llu negative windows, the limit is 2^31 - 1 = 2147483647", (unsigned long long)negN);
        return BAMM_ERR_UNSUPPORTED;
    }
    BAMM_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::unique_ptr<bamm_occ> res(new bamm_occ);
    int rc;

    // negatives: score, sort in place, fetch the lowest nTop + 1 (the scorer's per-sequence maxima are outputs its kernels
    // write unconditionally: a few bytes per sequence nobody reads here)
    DevBlocks tmp(c);
    DeviceScores neg;
    if ((rc = score_on_device(c, negatives, nullptr, K, W, bg_order, v, vbg, kWantMops, kPooledMops, tmp, &neg))) return rc;
    {
        // the sort's second buffer goes back to the pool as soon as the launches are queued: whoever takes it next (the
        // positives' scores below) is ordered behind them on the context's one stream.  The small histogram table is a
        // plain allocation and lives to the end of the call -- freeing it here would synchronise the device (as freeing a
        // second buffer below the pool's 4 MB does: a set that small has nothing to overlap with).
        DevBlocks sort_tmp(c);
        uint32_t *d_alt = nullptr, *d_hist = nullptr;
        const uint32_t blocks = occ_sort_blocks((uint32_t)negN, (uint32_t)std::max(1, c->num_cus));
        if ((rc = sort_tmp.scratch(&d_alt, (size_t)negN)) || (rc = tmp.alloc(&d_hist, (size_t)256 * blocks)) ||
            (rc = launch_occ_sort(neg.mops, d_alt, d_hist, (uint32_t)negN, blocks, st))) return rc;
    }
    const size_t nTop = occ_ntop((size_t)negN);
    std::vector<float> lowest(nTop + 1);
    if ((rc = ctx_download(c, lowest.data(), neg.mops, lowest.size() * sizeof(float)))) return rc;
    BAMM_HIP(hipStreamSynchronize(st));
    res->sc = occ_scalars(lowest.data(), (size_t)negN);

    // positives: score, rank against the sorted negatives, keep the candidates
    std::vector<OccCand> cand;
    DeviceScores pos;
    pos.moff.assign(1, 0);
    if (positives->n) {
        if ((rc = score_on_device(c, positives, nullptr, K, W, bg_order, v, vbg, kWantMops, kPooledMops, tmp, &pos))) return rc;
        const uint64_t n_pos = pos.moff[positives->n];
        OccRankArgs a{};
        a.pos = pos.mops; a.n_pos = n_pos; a.neg = neg.mops; a.n_neg = (uint32_t)negN; a.p_cutoff = p_cutoff;
        a.expf_branch = fabs(res->sc.lambda) > kOccEps ? 1u : 0u;
        if ((rc = tmp.alloc(&a.count, 1))) return rc;
        const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_pos + 255) / 256, (uint64_t)std::max(1, c->num_cus) * 16u));
        unsigned long long found = 0;
        a.cap = std::min<uint64_t>(n_pos, std::max<uint64_t>(65536, n_pos / 256));
        for (int attempt = 0; attempt < 2; attempt++) {      // the list is sized by guess; a launch that counts more runs again with room for all
            DevBlocks list_tmp(c);
            if ((rc = list_tmp.scratch(&a.out, (size_t)a.cap))) return rc;
            BAMM_HIP(hipMemsetAsync(a.count, 0, sizeof(unsigned long long), st));
            if ((rc = launch_occ_rank(a, blocks, st)) || (rc = ctx_download(c, &found, a.count, sizeof found))) return rc;
            BAMM_HIP(hipStreamSynchronize(st));
            if (found <= a.cap) {
                cand.resize((size_t)found);
                if ((rc = ctx_download(c, cand.data(), a.out, cand.size() * sizeof(OccCand)))) return rc;
                BAMM_HIP(hipStreamSynchronize(st));
                break;
            }
            if (attempt == 1) { set_error("bamm_occurrences: the candidate count changed between two launches"); return BAMM_ERR_STATE; }
            a.cap = found;
        }
    }
    res->n_candidates = cand.size();
    std::sort(cand.begin(), cand.end(), [](const OccCand& x, const OccCand& y) { return x.window < y.window; });
    const float posN = (float)positives->n;
    uint64_t seq = 0;
    for (const OccCand& k : cand) {
        const float p = occ_window_pvalue(k.score, (size_t)k.fp, k.higher, k.lower, res->sc);
        if (!(p < p_cutoff)) continue;
        while (pos.moff[seq + 1] <= k.window) seq++;         // candidates ascend
        res->seq.push_back(seq);
        res->pos.push_back((uint32_t)(k.window - pos.moff[seq]));
        res->score.push_back(k.score);
        res->fp.push_back(k.fp);
        res->p.push_back(p);
        res->e.push_back(p * posN);
    }
    *out = res.release();
    return BAMM_OK;
}

int bamm_occ_info(const bamm_occ* o, uint64_t* n_hits, uint64_t* n_neg_scores, uint32_t* n_top, float* s_ntop, float* lambda,
                  uint64_t* n_candidates) {
    if (!o) { set_error("bamm_occ_info: null argument"); return BAMM_ERR_ARG; }
    if (n_hits) *n_hits = o->p.size();
    if (n_neg_scores) *n_neg_scores = o->sc.negN;
    if (n_top) *n_top = (uint32_t)o->sc.nTop;
    if (s_ntop) *s_ntop = o->sc.S_ntop;
    if (lambda) *lambda = o->sc.lambda;
    if (n_candidates) *n_candidates = o->n_candidates;
    return BAMM_OK;
}

int bamm_occ_get(const bamm_occ* o, uint64_t* seq, uint32_t* pos, float* score, uint64_t* fp, float* p, float* e, uint64_t cap) {
    if (!o) { set_error("bamm_occ_get: null argument"); return BAMM_ERR_ARG; }
    const size_t n = o->p.size();
    if (cap < n) { set_error("bamm_occ_get: room for %llu hits, the result holds %zu", (unsigned long long)cap, n); return BAMM_ERR_ARG; }
    if (seq) std::copy(o->seq.begin(), o->seq.end(), seq);
    if (pos) std::copy(o->pos.begin(), o->pos.end(), pos);
    if (score) std::copy(o->score.begin(), o->score.end(), score);
    if (fp) std::copy(o->fp.begin(), o->fp.end(), fp);
    if (p) std::copy(o->p.begin(), o->p.end(), p);
    if (e) std::copy(o->e.begin(), o->e.end(), e);
    return BAMM_OK;
}

int bamm_occ_destroy(bamm_occ* o) {
    delete o;
    return BAMM_OK;
}

}  // extern "C"
