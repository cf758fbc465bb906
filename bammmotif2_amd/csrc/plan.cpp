// The launch plan of an EM handle (bamm_em_create): the column slices of tables beyond the fused kernel's LDS, the
// split of every length bucket into grouped-column and per-column launches, the blocks of each launch, the launch that
// carries the fused update and the sliced path's lists; the launch geometry of EM::mask.  Host code only.

#include <atomic>
#include <climits>
#include <cmath>
#include <functional>
#include <map>

#include "handles.h"

namespace bamm {

namespace {

constexpr size_t kLds = 160 * 1024;

// Make the kernel(s) one bucket's passes launch ready ahead of the first pass: the HIP runtime loads a translation unit's
// code object on the first use of any kernel in it (0.8 ms for the mixed-row kernels, 8-14 ms for the 4 MB units), which
// otherwise lands in the handle's first pass.  Runs on a thread of its own beside bamm_em_create's host work.
int prime_bucket(bamm_ctx* c, const bamm_em_params& prm, uint32_t Y, bool sliced, const EmBucket& eb) {
    if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice failed"); return BAMM_ERR_HIP; }
    // (no handle here -- bamm_em_create may have failed and deleted it by now -- so only the shape of pass_args)
    EmKernelArgs a = shape_args(prm, Y);
    if (eb.mclass == kLongClass) return prime_long_bucket(eb, a, c->stream);
    const uint32_t threads = bucket_threads(c, eb);
    EmLaunch what;
    if (sliced || !eb.grouped) {                             // k_em_seq, the slices and the list walk share kernels.hip
        a.logC = 0;
        return launch_em_seq(eb.mclass, what.accum, what.write_r, a, kPrimeOnly, threads, c->stream);
    }
    what.accum = true;
    GrpKernelArgs ga{};
    ga.e = a;
    if (!grp_geometry(prm.K, prm.W, eb.G, kMClasses[eb.mclass], threads / 64u, true, eb.logc, eb.layout, &ga.g)) return BAMM_OK;   // (the launch reports it)
    if (eb.layout & 8u)                                      // mixed rows: the builder of the lane records is the handle's first launch
        if (int rc = launch_mix_records(eb.mclass, SeqView{}, nullptr, prm.W, ga.g.T, ga.g.mixB, 0u, 0, nullptr, kPrimeOnly, c->stream)) return rc;
    return launch_em_grp(eb.mclass, what.accum, what.write_r, ga, kPrimeOnly, threads, c->stream);
}

}  // namespace

uint32_t default_threads(const bamm_ctx* c, int mclass) {
    uint32_t t = c->threads ? c->threads : max_threads_for_mclass(mclass);
    return std::min(t, max_threads_for_mclass(mclass));
}

// block size of one launch: the grouped kernel's longer length classes are built for fewer waves
uint32_t bucket_threads(const bamm_ctx* c, const EmBucket& b) {
    if (b.mclass == kLongClass) return 256u;
    const uint32_t t = default_threads(c, b.mclass);
    return b.grouped ? std::min(t, grp_max_threads(kMClasses[b.mclass])) : t;
}

uint32_t default_blocks(const bamm_ctx* c, uint32_t threads) {
    if (c->blocks) return c->blocks;
    const uint32_t cus = c->num_cus > 0 ? (uint32_t)c->num_cus : 256u;
    return cus * std::max(1u, 2048u / threads);       // fill 32 waves per CU
}

bool plan_slices(bamm_em* em) {
    const bamm_em_params* prm = &em->prm;
    const bamm_ctx* c = em->ctx;
    const uint32_t Y = em->Y;
    bool sliced = em_lds_bytes(prm->W, Y, true, 0, 0) > kLds;
    uint32_t e_cols = 0, m_cols = 0;
    // orders 7..10 (kmer_ spans 11 bases, Sequence.cpp:37): not even one column of the odds / count tables (4^(K+1) rows)
    // fits the 160 KiB of a CU.  Those models run with their tables in global memory (long_seq.hip: every window
    // multiplies its W odds straight from the table, the fixed-point addends go straight into the pass's
    // accumulator) -- the same integers, written for coverage, not speed.
    bool global_tables = false;
    if (sliced) {
        while (e_cols < prm->W && e_slice_lds_bytes(e_cols + 1, Y) <= kLds) e_cols++;
        while (m_cols < prm->W && m_slice_lds_bytes(m_cols + 1, Y, 0) <= kLds) m_cols++;
        if (e_cols == 0 || m_cols == 0) { global_tables = true; sliced = false; }
    }
    em->sliced = sliced;
    if (sliced) {
        auto cut = [&](uint32_t max_cols, std::vector<std::pair<uint32_t, uint32_t>>& out) {
            const uint32_t n = (prm->W + max_cols - 1) / max_cols, per = (prm->W + n - 1) / n;
            for (uint32_t j = 0; j < prm->W; j += per) out.emplace_back(j, std::min(prm->W, j + per));
            return per;
        };
        cut(e_cols, em->e_slices);
        em->e_fused = em_lds_bytes(prm->W, Y, false, 0, 0) <= kLds && c->use_e_fused;
        // sparse M-slices: room for a list of 256 windows + the y of every position per wave (8 waves per
        // block at the longest length class) is taken off the column budget when that costs no extra slice
        int mc_max = 0;                                      // longest length class present (the long bucket has no class)
        for (auto& b : em->seqs->buckets) mc_max = std::max(mc_max, b.mclass);
        const int Mmax = kMClasses[mc_max];
        const uint32_t waves = max_threads_for_mclass(mc_max) / 64u;
        const size_t scratch = !c->use_sparse ? 0 : m_slice_wave_bytes(Mmax, 256) * waves;
        uint32_t m_cols_sparse = 0;
        while (scratch && m_cols_sparse < prm->W && m_slice_lds_bytes(m_cols_sparse + 1, Y, 0) + scratch <= kLds) m_cols_sparse++;
        // ... and when it would, the widest slices stay and every bucket takes the longest list that still
        // fits beside them (run_accumulate): at k=4, W=30 a 128-entry list next to the 120 KB count slice
        // is worth 20 % of the iteration
        const bool roomy = m_cols_sparse && (prm->W + m_cols_sparse - 1) / m_cols_sparse == (prm->W + m_cols - 1) / m_cols;
        if (roomy) m_cols = m_cols_sparse;
        if (scratch) em->m_slice_cap = 256;
        const uint32_t per_m = cut(m_cols, em->m_slices);
        const size_t used = roomy ? scratch : std::min(scratch, kLds - std::min(kLds, m_slice_lds_bytes(per_m, Y, 0)));
        while (em->m_slice_logc < 4 && m_slice_lds_bytes(per_m, Y, em->m_slice_logc + 1) + used <= kLds) em->m_slice_logc++;
    }
    return global_tables;
}

namespace {

// What the stages of plan_launches share.  The code objects of the kernels the handle will launch are loaded beside the
// host work (prime_bucket, on a thread of its own), each as soon as the plan names the kernel.
struct Planning {
    bamm_em* em;
    Primers& primers;
    bool uploads_pending = false;                            // index lists / tile offsets were uploaded: one synchronisation at the end
    void prime(const EmBucket& eb) {
        primers.t.emplace_back([c = em->ctx, prm = em->prm, Y = em->Y, sliced = em->sliced, eb] { (void)prime_bucket(c, prm, Y, sliced, eb); });
    }
};

// Stage 1, a bucket beyond the length classes (or any bucket of a handle whose tables stay in global memory): one launch of
// long_seq.hip, or of em_tiles.hip.  Decides tiled or window by window; a tiled bucket uploads its tile offsets and allocates
// the tiles' and records' normalisers.
int plan_long_bucket(Planning& pl, const Bucket& b, bool global_tables, EmBucket* out) {
    bamm_em* em = pl.em;
    const uint32_t W = em->prm.W;
    EmBucket eb;
    eb.mclass = kLongClass; eb.count = b.count; eb.d_idx = b.d_idx;
    eb.work = b.mclass == kLongClass ? b.work : (double)b.count * kMClasses[b.mclass];
    // Tile by tile (em_tiles.hip) while the odds and count tables fit one CU's LDS unsliced and W leaves a tile a
    // stride: sliced handles (their slot layout), tables in global memory (which send short sequences here too) and
    // "em_tiles" = 0 stay window by window.  The tiles of EVERY sequence, mask or not: getR runs without the mask.
    if (b.mclass == kLongClass && !global_tables && !em->sliced && em->ctx->use_em_tiles && em_tile_geometry(W, nullptr, &eb.tile_stride)) {
        std::vector<uint32_t> toff((size_t)b.count + 1, 0u);
        uint64_t tiles = 0;
        for (uint32_t t = 0; t < b.count; t++) {
            const uint64_t seq = b.h_idx.empty() ? t : b.h_idx[t];
            tiles += ((uint64_t)em->seqs->h_len[seq] - W + eb.tile_stride) / eb.tile_stride;
            toff[t + 1] = (uint32_t)std::min<uint64_t>(tiles, UINT32_MAX);
        }
        if (tiles != 0 && tiles <= UINT32_MAX) {             // (more tiles than a launch indexes: window by window)
            uint32_t* d_toff = nullptr;
            int rc;
            if ((rc = em->mem.upload(&d_toff, toff.data(), toff.size())) || (rc = em->mem.alloc(&eb.d_tile_z, (size_t)tiles)) ||
                (rc = em->mem.alloc(&eb.d_rec_invz, (size_t)b.count))) return rc;
            pl.uploads_pending = true;
            eb.tiled = true; eb.n_tiles = (uint32_t)tiles; eb.d_tile_off = d_toff;
        }
    }
    *out = eb;
    return BAMM_OK;
}

// `ids` as a launch's index list on the device (owned by the handle)
int upload_ids(Planning& pl, const std::vector<uint32_t>& ids, EmBucket* eb) {
    uint32_t* d = nullptr;
    if (int rc = pl.em->mem.upload(&d, ids.data(), ids.size())) return rc;
    pl.uploads_pending = true;
    eb->count = (uint32_t)ids.size(); eb->d_idx = d;
    return BAMM_OK;
}

// Stage 2, one length class: the sequences the grouped-column kernel takes (no exception, or all of them within its
// virtual rows) and the rest, appended to `out` as one or two launches.  Decides group size / copies / layout (grp_plan);
// uploads the index lists of a split class and, for mixed rows, allocates and builds (one launch) the lane records.
int plan_class_split(Planning& pl, const Bucket& b, bool want_grouped, uint64_t plan_n, std::vector<EmBucket>& out) {
    bamm_em* em = pl.em;
    bamm_seqs* seqs = em->seqs;
    const bamm_ctx* c = em->ctx;
    const uint32_t K = em->prm.K, W = em->prm.W;
    const int Mcls = kMClasses[b.mclass];
    const uint32_t waves = std::min(default_threads(c, b.mclass), grp_max_threads(Mcls)) / 64u;   // of the grouped kernel
    auto seq_at = [&](uint64_t i) { return b.d_idx ? b.h_idx[i] : (uint32_t)i; };
    int rc;
    // do most sequences of this bucket carry exceptions (a double-stranded set: all of them)?
    std::atomic<size_t> with_exc{0};
    host_ranges(b.count, [&](uint64_t i0, uint64_t i1) {
        size_t cnt = 0;
        for (uint64_t i = i0; i < i1; i++) cnt += em->exc->h_off[seq_at(i) + 1] != em->exc->h_off[seq_at(i)];
        with_exc.fetch_add(cnt, std::memory_order_relaxed);
    });
    GrpGeom gg{};
    uint32_t glogc = 0, gG = 0, glayout = 0;
    std::vector<uint32_t> no;
    if (want_grouped && grp_supported_class(Mcls, K) &&
        grp_plan(K, W, Mcls, waves, 2 * with_exc.load() > b.count, plan_n * (uint64_t)Mcls >= 40000ull * 7ull, c->group_size, c->group_layout, &gG, &glogc, &glayout) &&
        grp_geometry(K, W, gG, Mcls, waves, true, glogc, glayout, &gg)) {
        EmBucket eb;
        eb.mclass = b.mclass; eb.grouped = true; eb.logc = glogc; eb.G = gG; eb.layout = glayout;
        pl.prime(eb);
        const ExcK::XRec* xr = nullptr;
        if ((rc = xrec_for_group(seqs, K, gG, em->exc, &xr))) return rc;
        eb.d_xrec = xr->d_xrec;
        // exceptions within the virtual rows for them, and clear of the rows for the LW1 edge
        auto capable = [&](uint32_t n) {
            const uint32_t B = xr->h_B[n];
            return B == 0u || (B <= gg.Bj && (gg.np != 0u || xr->h_lo[n] + B + gg.G <= seqs->h_len[n] - W + 1u));
        };
        std::atomic<bool> all_capable{true};
        host_ranges(b.count, [&](uint64_t i0, uint64_t i1) {
            for (uint64_t i = i0; i < i1 && all_capable.load(std::memory_order_relaxed); i++)
                if (!capable(seq_at(i))) all_capable.store(false, std::memory_order_relaxed);
        });
        const bool all = all_capable.load();
        // Mixed rows: a sequence RUNS in the shortest class whose 64 M slots reach all of its rows that are not neutral when
        // the windows are anchored at their start (mixed_kernel.h, ANCH; "mix_anchor" = 0: never) -- 200 bp on both strands
        // at W = 20 in class 6 instead of 7 -- if that class is shorter than the bucket's and k_em_mix is built for it; else
        // in the bucket's class, end-anchored as ever.  The rule reads (L, W) only, so every shard of a set takes the same
        // kernel for the same sequence.  The bucket itself stays classed by L: the scorer and the other kernels read it.
        int anch_class[kNumMClasses];                        // per span in units of 64 slots: the class to run in, or the bucket's
        const bool mixed = (glayout & 8u) != 0u;
        auto run_class = [&](uint32_t n) {
            if (!mixed || !c->use_mix_anchor) return b.mclass;
            const uint32_t need = (mix_anchor_span(seqs->h_len[n], W, gg.mixB) + 63u) / 64u;
            return need < (uint32_t)kNumMClasses ? anch_class[need] : b.mclass;
        };
        if (mixed) {
            for (int need = 0; need < kNumMClasses; need++) {
                anch_class[need] = b.mclass;
                for (int ci = 3; ci <= 8 && ci < b.mclass; ci++) {           // the classes launch_mix has
                    if (kMClasses[ci] < need) continue;
                    GrpGeom g2{};
                    const uint32_t w2 = std::min(default_threads(c, ci), grp_max_threads(kMClasses[ci])) / 64u;
                    if (mix_geometry(K, W, kMClasses[ci], w2, true, &g2)) anch_class[need] = ci;
                    break;
                }
            }
        }
        std::atomic<int> cls_lo{INT_MAX}, cls_hi{-1};
        host_ranges(b.count, [&](uint64_t i0, uint64_t i1) {
            int lo = INT_MAX, hi = -1;
            for (uint64_t i = i0; i < i1; i++) {
                if (!all && !capable(seq_at(i))) continue;
                const int rcl = run_class(seq_at(i));
                lo = std::min(lo, rcl); hi = std::max(hi, rcl);
            }
            for (int cur = cls_lo.load(); lo < cur && !cls_lo.compare_exchange_weak(cur, lo);) {}
            for (int cur = cls_hi.load(); hi > cur && !cls_hi.compare_exchange_weak(cur, hi);) {}
        });
        // one launch per class run, the bucket's own first: the whole bucket as it stands when nothing splits it, else index lists
        std::map<int, std::vector<uint32_t>, std::greater<int>> parts;
        const bool whole = all && cls_lo.load() == cls_hi.load() && cls_hi.load() >= 0;
        if (whole) parts[cls_lo.load()];
        else
            for (uint32_t i = 0; i < b.count; i++) {
                if (all || capable(seq_at(i))) parts[run_class(seq_at(i))].push_back(seq_at(i));
                else no.push_back(seq_at(i));
            }
        for (auto& part : parts) {
            EmBucket pb = eb;
            pb.mclass = part.first;
            const int Mrun = kMClasses[pb.mclass];
            const bool anchored = pb.mclass != b.mclass;
            if (anchored) pb.layout |= kMixAnchorBit;
            if (whole) { pb.count = b.count; pb.d_idx = b.d_idx; }
            else if ((rc = upload_ids(pl, part.second, &pb))) return rc;
            if (mixed && pb.count) {
                // mixed rows: every lane's stream window and fix-lane codes per launch slot of this launch, derived once
                // here instead of in every pass (lane_records.h; 512 bytes per sequence, set-sized: from the scratch pool);
                // the accumulating layout of the class run: its resident columns decide what a fix lane has left to log
                GrpGeom gr = gg;
                if (anchored && !grp_geometry(K, W, gG, Mrun, bucket_threads(c, pb) / 64u, true, glogc, glayout, &gr)) {
                    set_error("mixed rows: no geometry for the start-anchored class %d", Mrun);
                    return BAMM_ERR_UNSUPPORTED;
                }
                uint2* rec = nullptr;
                if ((rc = em->mem.scratch(&rec, (size_t)pb.count * 64u))) return rc;
                if ((rc = launch_mix_records(pb.mclass, make_view(seqs, em->exc, pb.d_idx, pb.count, nullptr), xr->d_xrec, W, gr.T, gr.mixB,
                                             mix_resident_cols(gr), anchored ? mix_anchor_frame(gr.mixB) : 0, rec,
                                             (uint32_t)std::max(1, c->num_cus), c->stream))) return rc;
                pb.d_lane_rec = rec;
            }
            pb.work = (double)pb.count * Mrun * 0.6;         // grouped passes cost about 60 % per sequence
            if (pb.count) out.push_back(pb);
        }
        if (all) return BAMM_OK;
    }
    EmBucket eb;
    eb.mclass = b.mclass;
    if (no.empty()) { eb.count = b.count; eb.d_idx = b.d_idx; }
    else if ((rc = upload_ids(pl, no, &eb))) return rc;
    eb.work = (double)eb.count * Mcls;
    out.push_back(eb);
    pl.prime(eb);
    return BAMM_OK;
}

// Stage 3, every launch: its blocks (split over the launches in proportion to their work) and, for the per-column kernel,
// the copies of the count table and the sparse M-step's scratch.  Decides only; fills the EmBuckets and total_blocks.
void plan_launch_sizes(bamm_em* em) {
    const bamm_ctx* c = em->ctx;
    const uint32_t W = em->prm.W, Y = em->Y;
    const bool sliced = em->sliced;
    double total_work = 0;
    for (auto& b : em->ebuckets) total_work += b.work;
    em->total_blocks = 0;
    for (auto& b : em->ebuckets) {
        if (b.mclass == kLongClass) {                        // a workgroup per sequence
            b.blocks = std::min(b.count, (uint32_t)std::max(1, c->num_cus) * 8u);
            em->total_blocks += b.blocks;
            continue;
        }
        const uint32_t threads = bucket_threads(c, b);
        // 16 waves per CU saturate the LDS pipe (tools/lds_bench2.hip); the LDS left over goes
        // into private copies of the count table
        const uint32_t blocks_per_cu = sliced ? 1u : std::max(1u, 1024u / threads);
        if (!b.grouped) {
            // sparse M-step scratch (per wave) competes with the private copies for LDS; it is only
            // enabled when at least 4 copies survive next to it
            const int Mcls = kMClasses[b.mclass];
            size_t scratch = sliced ? 0 : sparse_wave_bytes(Mcls) * (threads / 64u);
            uint32_t cap = sliced ? 0u : sparse_cap_for(Mcls);
            if (!c->use_sparse) { cap = 0; scratch = 0; }
            if (cap && (em_lds_bytes(W, Y, true, 0, scratch) > kLds / blocks_per_cu ||
                        pick_log_copies(W, Y, blocks_per_cu, scratch) + 1 < pick_log_copies(W, Y, blocks_per_cu, 0))) {
                cap = 0;
                scratch = 0;
            }
            b.sparse_cap = cap;
            b.sparse_bytes = (uint32_t)(cap ? sparse_wave_bytes(Mcls) : 0);
            b.logc = sliced ? 0u : pick_log_copies(W, Y, blocks_per_cu, scratch);
        }
        const uint32_t per_cu = b.grouped ? 1u : blocks_per_cu;
        const uint32_t all = c->blocks ? c->blocks : (uint32_t)std::max(1, c->num_cus) * per_cu;
        uint32_t nb = (uint32_t)std::max(1.0, std::floor(all * (b.work / total_work) + 0.5));
        const uint32_t waves_per_block = threads / 64u;
        nb = std::min(nb, (b.count + waves_per_block - 1) / waves_per_block);
        nb = std::max(nb, 1u);
        b.blocks = nb;
        em->total_blocks += nb;
    }
}

// Stage 4, fused updates (update_kernel.h): inside iterate() / optimize() the model update of pass p runs in the block
// prologue of pass p+1's FIRST launch -- a grouped kernel whose count tables leave room for the update's scratch.  Decides
// which launch that is, moves it to the front and allocates every block's copy of the odds table.
int plan_fused_update(bamm_em* em) {
    const uint32_t K = em->prm.K, W = em->prm.W, Y = em->Y;
    if (em->sliced || !em->ctx->use_fused_update || !update_fits_lds(K, W) || K > 2u) return BAMM_OK;
    size_t best = em->ebuckets.size();
    for (size_t i = 0; i < em->ebuckets.size(); i++)
        if (em->ebuckets[i].grouped && kMClasses[em->ebuckets[i].mclass] <= BAMM_FUSE_MAX_M &&   // the classes built with the fused prologue
            (best == em->ebuckets.size() || em->ebuckets[i].count > em->ebuckets[best].count)) best = i;
    if (best == em->ebuckets.size()) return BAMM_OK;
    std::swap(em->ebuckets[0], em->ebuckets[best]);
    const EmBucket& eb = em->ebuckets[0];
    GrpGeom g{};
    if (!grp_geometry(K, W, eb.G, kMClasses[eb.mclass], bucket_threads(em->ctx, eb) / 64u, true, eb.logc, eb.layout, &g)) return BAMM_OK;
    const uint32_t need = (uint32_t)update_lds_bytes(K, W);
    const uint32_t s1_bytes = (W * (Y + 1u) * 4u + 15u) & ~15u;
    // mixed rows: behind the staged single-column table, inside the count tables; uniform rows: the count table
    const uint32_t off = (eb.layout & 8u) ? g.off_s1 + s1_bytes : g.off_ng;
    const uint32_t end = (eb.layout & 8u) ? g.off_wave : g.off_n1;
    if (off + need > end) return BAMM_OK;
    em->fusable = true;
    em->fuse_upd_off = off;
    return em->mem.alloc(&em->d_s_block, (size_t)eb.blocks * W * (Y + 1u));
}

// Stage 5, the sliced path with k_em_seq as its E pass: compacted lists between the E pass and the M slices, and the
// choice per pass between them and dense r.  Allocates the lists and the two counters; decides the threshold.
int plan_lists(bamm_em* em, const uint8_t* seq_mask) {
    const bamm_ctx* c = em->ctx;
    bamm_seqs* seqs = em->seqs;
    hipStream_t st = c->stream;
    if (!em->sliced || !em->e_fused || !c->use_e_list) return BAMM_OK;
    int rc;
    if ((rc = em->mem.scratch(&em->d_list_r, (size_t)seqs->total_len)) || (rc = em->mem.scratch(&em->d_list_p, (size_t)seqs->total_len)) ||
        (rc = em->mem.alloc(&em->d_list_n, (size_t)seqs->n))) return rc;
    if (hipMemsetAsync(em->d_list_n, 0, (seqs->n ? seqs->n : 1) * sizeof(uint32_t), st) != hipSuccess) { set_error("hipMemsetAsync failed"); return BAMM_ERR_HIP; }
    // lists or dense r, per pass: the first pass of a handle takes the dense flavour (nothing is known yet: the
    // counter starts saturated), later ones lists once fewer than list_threshold_pct of the windows are non-zero
    if ((rc = em->mem.alloc(&em->d_nnz, 2))) return rc;
    const unsigned long long start[2] = {~0ull, 0ull};
    if (hipMemcpyAsync(em->d_nnz, start, sizeof start, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("hipMemcpyAsync failed"); return BAMM_ERR_HIP; }
    unsigned long long windows = 0;
    for (uint64_t n = 0; n < seqs->n; n++) windows += seqs->h_len[n] - em->prm.W + 1u;
    if (seq_mask && seqs->n) windows = (unsigned long long)((double)windows * (double)em->n_active / (double)seqs->n);
    em->nnz_limit = windows / 100u * c->list_threshold_pct;
    em->adaptive_lists = c->use_adaptive_lists;
    return BAMM_OK;
}

}  // namespace

int plan_launches(bamm_em* em, bool global_tables, const uint8_t* seq_mask, Primers& primers) {
    const bamm_em_params* prm = &em->prm;
    Planning pl{em, primers};
    int rc = BAMM_OK;
    const bool want_grouped = !em->sliced && prm->K <= 3u && em->ctx->use_grouped;
    // A shard of a sharded set plans its kernels as the whole set would: which rows a sequence is multiplied through
    // (mixed or uniform) decides the last bit of its responsibilities, so the choice follows the GLOBAL size the caller
    // names (n_seqs_bound / n_seqs_global; this shard's own count when it names neither) and nothing about the shard:
    // every length class of a set of `plan_n` sequences is planned as a launch of that many (a class that holds a small
    // part of a large set pays the larger tables' few microseconds per launch; an estimate of the class's global share
    // from this shard's own mix of lengths could differ between ranks next to the threshold).  The other input of the
    // plan, whether most sequences of a class carry exceptions, is the shard's own: a property of the data that holds
    // for every shard alike on double-stranded sets (each sequence has its strand junction) and on clean single-stranded ones.
    const uint64_t plan_n = std::max<uint64_t>(std::max<uint64_t>(prm->n_seqs_bound, prm->n_seqs_global), em->seqs->n);
    for (auto& b : em->seqs->buckets) {                      // the launches of one pass, in the order of the set's buckets
        if (b.mclass == kLongClass || global_tables) {       // beyond the length classes / tables beyond LDS
            EmBucket eb;
            if ((rc = plan_long_bucket(pl, b, global_tables, &eb))) return rc;
            em->ebuckets.push_back(eb);
            pl.prime(eb);
        } else if ((rc = plan_class_split(pl, b, want_grouped, plan_n, em->ebuckets))) return rc;
    }
    plan_launch_sizes(em);
    if ((rc = plan_fused_update(em)) || (rc = plan_lists(em, seq_mask))) return rc;
    // index lists and tile offsets are on the device before the plan is handed out (nothing above reads device memory)
    if (pl.uploads_pending && hipStreamSynchronize(em->ctx->stream) != hipSuccess) { set_error("stream sync failed"); return BAMM_ERR_HIP; }
    return BAMM_OK;
}

uint32_t MaskPlan::waves_for(size_t table) const {
    return wave_global ? 4u : (uint32_t)std::max<size_t>(1, std::min<size_t>(4, (kLds - table) / wave_bytes));
}

MaskPlan mask_plan(uint32_t W, uint32_t Y, uint32_t max_len, uint64_t n_seqs, size_t cells, int num_cus) {
    auto round16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t s_bytes = round16((size_t)W * (Y + 1) * sizeof(float));
    MaskPlan p{};
    p.direct = round16((size_t)Y * 8) > kLds;
    p.wave_global = p.direct || mask_wave_bytes(max_len, false) + round16((size_t)Y * 8) > kLds || max_len > 65535u;
    p.wave_bytes = mask_wave_bytes(max_len, p.wave_global);
    p.s_in_lds = s_bytes <= 64 * 1024 && (p.wave_global || s_bytes + p.wave_bytes <= kLds);
    p.e_table = p.s_in_lds ? s_bytes : 0;
    p.m_cols = p.direct ? W : (uint32_t)std::min<size_t>(W, (p.wave_global ? kLds / 2 : std::min(kLds / 2, kLds - p.wave_bytes)) / ((size_t)Y * 8));
    p.m_cols = std::max(1u, p.m_cols);
    p.m_table = p.direct ? 0 : round16((size_t)p.m_cols * Y * 8);
    p.init_table = (uint32_t)round16((size_t)W * 4 * sizeof(float));
    p.e_waves = p.waves_for(p.e_table); p.m_waves = p.waves_for(p.m_table);
    // 16 waves per CU (as the fused kernel), but no more partial tables than 64 MiB worth
    // (arrays in global memory: at most 2048 waves' worth of them)
    // ... and no more than 8 GiB of them: a launch has at most cus * 8 blocks of 4 waves
    p.cus = p.wave_global ? (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min(64u, (uint32_t)std::max(1, num_cus)), ((size_t)8 << 30) / (32 * p.wave_bytes)))
                          : (uint32_t)std::max(1, num_cus);
    const uint32_t per_cu = std::max(1u, 16u / std::min(p.e_waves, p.m_waves));
    const uint32_t cap_blocks = p.direct ? p.cus * 8u        // no partial tables at all
                                         : (uint32_t)std::max<size_t>(p.cus, std::min<size_t>((size_t)p.cus * per_cu, ((size_t)64 << 20) / (cells * 8)));
    p.mblocks = std::max(1u, std::min(((uint32_t)n_seqs + std::min(p.e_waves, p.m_waves) - 1) / std::min(p.e_waves, p.m_waves), cap_blocks));
    // every launch has at most cus * 8 blocks of 4 waves
    p.wave_scratch_bytes = p.wave_global ? (size_t)std::max(p.cus * 8u, p.mblocks) * 4u * p.wave_bytes : 0;
    return p;
}

}  // namespace bamm

extern "C" int bamm_mask_plan(uint32_t W, uint32_t Y, uint32_t max_len, uint64_t n_seqs, uint64_t cells, int num_cus, uint64_t* out) {
    if (!out || !W || !Y || !cells) { bamm::set_error("bamm_mask_plan: bad argument"); return BAMM_ERR_ARG; }
    const bamm::MaskPlan p = bamm::mask_plan(W, Y, max_len, n_seqs, (size_t)cells, num_cus);
    const uint64_t v[13] = {p.direct, p.wave_global, p.wave_bytes, p.s_in_lds, p.e_table, p.m_cols, p.m_table, p.init_table,
                            p.e_waves, p.m_waves, p.cus, p.mblocks, p.wave_scratch_bytes};
    std::copy(v, v + 13, out);
    return BAMM_OK;
}
