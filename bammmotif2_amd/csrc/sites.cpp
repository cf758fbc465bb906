// bamm_em_sites: the windows with r >= cut-off (the rows of EM::write's .positions, EM.cpp:577-601) and every
// sequence's best window (GibbsSampling.cpp:105-116), taken from the dense r where it lies on the device (sites.hip).
// The host sees three words per sequence and 12 bytes per site; no window-sized array crosses.  Host code only.

#include <cmath>

#include "handles.h"

using namespace bamm;

struct bamm_sites {
    std::vector<uint64_t> seq;
    std::vector<uint32_t> pos, z, count;
    std::vector<float> r, r_best;
};

namespace {

// dense r the call keeps on the device at a time unless "sites_chunk_positions" says otherwise: 512 MiB, a third of
// the 401 M positions of 1M x 200 bp on both strands (getR's scratch for that set is 1.6 GB)
constexpr uint64_t kSitesChunkPositions = uint64_t(1) << 27;

template <class T>
int download_array(bamm_ctx* c, std::vector<T>& dst, const T* src_dev, size_t count) {
    dst.resize(count);
    if (!count) return BAMM_OK;
    return ctx_download(c, dst.data(), src_dev, count * sizeof(T));
}

}  // namespace

extern "C" {

int bamm_em_sites(bamm_em* em, uint64_t begin, uint64_t end, float cutoff, bamm_sites** out) {
    if (!em || !out || begin > end || end > em->seqs->n) { set_error("bamm_em_sites: bad range"); return BAMM_ERR_ARG; }
    *out = nullptr;
    if (std::isnan(cutoff)) { set_error("bamm_em_sites: the cut-off is not a number"); return BAMM_ERR_ARG; }
    bamm_seqs* s = em->seqs;
    bamm_ctx* c = em->ctx;
    std::unique_ptr<bamm_sites> res(new bamm_sites);
    const uint64_t n = end - begin;
    if (n == 0) { *out = res.release(); return BAMM_OK; }
    BAMM_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc;

    DevBlocks tmp(c);
    uint32_t *d_count = nullptr, *d_z = nullptr;
    float* d_best = nullptr;
    unsigned long long *d_offset = nullptr, *d_total = nullptr;
    if ((rc = tmp.scratch(&d_count, (size_t)n)) || (rc = tmp.scratch(&d_z, (size_t)n)) || (rc = tmp.scratch(&d_best, (size_t)n)) ||
        (rc = tmp.scratch(&d_offset, (size_t)n)) || (rc = tmp.alloc(&d_total, 1))) return rc;

    // r that spans the whole set already (EM::mask's, the sliced path's state) is walked in one go; a range the fused
    // kernels fill goes in chunks of whole sequences of at most `budget` positions, a longer sequence alone
    const bool resident_r = em->mask_done || em->sliced;
    const uint64_t budget = c->sites_chunk_positions ? c->sites_chunk_positions : kSitesChunkPositions;
    const uint32_t max_blocks = (uint32_t)std::max(1, c->num_cus) * 8u;
    unsigned long long found = 0;                            // sites of the chunks so far
    std::vector<SiteRec> rec;
    for (uint64_t cb = begin; cb < end;) {
        uint64_t ce = cb + 1;
        if (resident_r) ce = end;
        else while (ce < end && s->h_pos_off[ce + 1] - s->h_pos_off[cb] <= budget) ce++;
        DevBlocks chunk_tmp(c);                              // the chunk's r and its records go back to the pool behind it
        DenseR dr;
        if ((rc = dense_r_on_device(em, cb, ce, chunk_tmp, &dr))) return rc;
        SitesArgs a{};
        a.r = dr.r; a.r_base = dr.base; a.slot_layout = dr.slot_layout ? 1u : 0u;
        a.pos_off = s->d_pos_off; a.len = s->d_len;
        a.seq_begin = (uint32_t)cb; a.n_seqs = (uint32_t)(ce - cb); a.out_begin = (uint32_t)begin;
        a.W = em->prm.W; a.cutoff = cutoff;
        a.count = d_count; a.z = d_z; a.r_best = d_best; a.offset = d_offset;
        const uint32_t blocks = std::min<uint32_t>(max_blocks, (a.n_seqs + 3u) / 4u);
        unsigned long long total = 0;
        if ((rc = launch_sites_count(a, blocks, st)) ||
            (rc = launch_sites_scan(d_count + (cb - begin), d_offset + (cb - begin), a.n_seqs, found, d_total, st)) ||
            (rc = ctx_download(c, &total, d_total, sizeof total))) return rc;
        BAMM_HIP(hipStreamSynchronize(st));
        const unsigned long long fresh = total - found;
        if (fresh) {
            a.out_base = found; a.out_cap = fresh;
            if ((rc = chunk_tmp.scratch(&a.out, (size_t)fresh)) || (rc = launch_sites_write(a, blocks, st))) return rc;
            rec.resize((size_t)total);
            if ((rc = ctx_download(c, rec.data() + found, a.out, (size_t)fresh * sizeof(SiteRec)))) return rc;
            BAMM_HIP(hipStreamSynchronize(st));
        }
        found = total;
        cb = ce;
    }
    if ((rc = download_array(c, res->count, d_count, (size_t)n)) || (rc = download_array(c, res->z, d_z, (size_t)n)) ||
        (rc = download_array(c, res->r_best, d_best, (size_t)n))) return rc;
    BAMM_HIP(hipStreamSynchronize(st));
    res->seq.resize(rec.size()); res->pos.resize(rec.size()); res->r.resize(rec.size());
    host_ranges(rec.size(), [&](uint64_t b, uint64_t e) {
        for (uint64_t i = b; i < e; i++) { res->seq[i] = rec[i].seq; res->pos[i] = rec[i].pos; res->r[i] = rec[i].r; }
    });
    *out = res.release();
    return BAMM_OK;
}

int bamm_sites_info(const bamm_sites* s, uint64_t* n_sites, uint64_t* n_seqs) {
    if (!s) { set_error("bamm_sites_info: null argument"); return BAMM_ERR_ARG; }
    if (n_sites) *n_sites = s->r.size();
    if (n_seqs) *n_seqs = s->z.size();
    return BAMM_OK;
}

int bamm_sites_get(const bamm_sites* s, uint64_t* seq, uint32_t* pos, float* r, uint64_t cap) {
    if (!s) { set_error("bamm_sites_get: null argument"); return BAMM_ERR_ARG; }
    if (cap < s->r.size()) { set_error("bamm_sites_get: room for %llu sites, the result holds %zu", (unsigned long long)cap, s->r.size()); return BAMM_ERR_ARG; }
    if (seq) std::copy(s->seq.begin(), s->seq.end(), seq);
    if (pos) std::copy(s->pos.begin(), s->pos.end(), pos);
    if (r) std::copy(s->r.begin(), s->r.end(), r);
    return BAMM_OK;
}

int bamm_sites_best(const bamm_sites* s, uint32_t* z, float* r_best, uint32_t* count, uint64_t cap) {
    if (!s) { set_error("bamm_sites_best: null argument"); return BAMM_ERR_ARG; }
    if (cap < s->z.size()) { set_error("bamm_sites_best: room for %llu sequences, the result holds %zu", (unsigned long long)cap, s->z.size()); return BAMM_ERR_ARG; }
    if (z) std::copy(s->z.begin(), s->z.end(), z);
    if (r_best) std::copy(s->r_best.begin(), s->r_best.end(), r_best);
    if (count) std::copy(s->count.begin(), s->count.end(), count);
    return BAMM_OK;
}

int bamm_sites_destroy(bamm_sites* s) {
    delete s;
    return BAMM_OK;
}

}  // extern "C"
