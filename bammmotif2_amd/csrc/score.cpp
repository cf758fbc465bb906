// The scorer of the C ABI: the seed model's counts from a PWM (Motif::initFromPWM) and the log-odds scores of a model
// over a resident set (ScoreSeqSet::calcLogOdds).  Host code only.

#include <climits>
#include <cmath>

#include "handles.h"

using namespace bamm;

namespace bamm {

namespace {

// The scorer a length bucket takes: k_score while a sequence fits one wavefront's registers, beyond that the same chain
// tile by tile (both in scorer.hip, one chain, the log-odds table in LDS), and the window-by-window scorer (long_seq.hip),
// which reads the table from global memory, for tables beyond the LDS of a CU (K = 4 from W = 40, K = 5 from W = 10, K = 6
// from W = 3), for widths that leave a tile no stride, and for long sequences under bamm_ctx_set_tuning("score_tiles", 0).
// Under bamm_ctx_set_tuning("score_slices", 1) a table beyond the LDS of which at least one column fits (orders up to 6)
// takes the first two instead, a slice of columns per launch (score_slices: 1 = the table fits whole).
enum class ScoreRoute { kWave, kTiles, kWindows };
constexpr size_t kScoreLdsBytes = 160u * 1024u;
// the slices of columns the LDS kernels take the table in: 1 = whole, 0 = it stays in global memory
uint32_t score_slices(const bamm_ctx* c, uint32_t K, uint32_t W, uint32_t* columns_per_slice) {
    uint32_t cps = W, S = 1;
    if ((size_t)W * (ipow4(K + 1) + 1) * sizeof(float) > kScoreLdsBytes && !(c->use_score_slices && score_slice_geometry(K, W, &cps, &S)))
        return 0;
    if (columns_per_slice) *columns_per_slice = cps;
    return S;
}
ScoreRoute score_route(const bamm_ctx* c, const Bucket& bk, uint32_t K, uint32_t W) {
    if (!score_slices(c, K, W, nullptr)) return ScoreRoute::kWindows;
    if (bk.mclass != kLongClass) return ScoreRoute::kWave;
    return c->use_score_tiles && score_tile_geometry(W, nullptr, nullptr) ? ScoreRoute::kTiles : ScoreRoute::kWindows;
}

// prefix sums of the tile counts of a long bucket's sequences, ceil((L - W + 1) / stride) each and none for a sequence the
// mask leaves out: one entry per long sequence, nothing proportional to their length.  Returns the number of tiles.
uint64_t bucket_tiles(const bamm_seqs* s, const Bucket& bk, const uint8_t* seq_mask, uint32_t W, uint32_t stride,
                      std::vector<uint32_t>* off) {
    uint64_t tiles = 0;
    if (off) off->assign((size_t)bk.count + 1, 0u);
    for (uint32_t t = 0; t < bk.count; t++) {
        const uint64_t seq = bk.h_idx.empty() ? t : bk.h_idx[t];
        if (!seq_mask || seq_mask[seq]) tiles += ((uint64_t)s->h_len[seq] - W + stride) / stride;
        if (off) (*off)[t + 1] = (uint32_t)std::min<uint64_t>(tiles, UINT32_MAX);
    }
    return tiles;
}

}  // namespace

int score_on_device(bamm_ctx* c, bamm_seqs* s, const uint8_t* seq_mask, uint32_t K, uint32_t W, uint32_t bg_order, const float* v,
                    const float* vbg, bool want_mops, bool pooled_mops, DevBlocks& tmp, DeviceScores* out) {
    const uint32_t Y = (uint32_t)ipow4(K + 1), Ys = Y + 1, Kbg = std::min(bg_order, K);
    const uint32_t Yb = (uint32_t)ipow4(Kbg + 1);
    // Motif::calculateLogS (Motif.cpp:471-483) with the host's logf, laid out [j][y] + neutral row
    std::vector<float> tab((size_t)W * Ys, 0.0f);
    const float* vK = v + v_offset(K, W);
    const float* b = vbg + bg_offset(Kbg);
    for (uint32_t y = 0; y < Y; y++)
        for (uint32_t j = 0; j < W; j++)
            tab[(size_t)j * Ys + y] = logf(vK[(size_t)y * W + j] + 1e-5f) - logf(b[y % Yb]);
    std::vector<uint64_t>& moff = out->moff;
    moff.assign(s->n + 1, 0);
    for (uint64_t n = 0; n < s->n; n++) moff[n + 1] = moff[n] + (s->h_len[n] - W + 1);
    hipStream_t st = c->stream;
    ExcK* exc = nullptr;
    int rc = exceptions_for_order(s, K, &exc);
    if (rc) return rc;
    float *d_tab = nullptr, *d_mops = nullptr, *d_zoops = nullptr;
    uint64_t* d_moff = nullptr;
    uint32_t* d_z = nullptr;
    uint8_t* d_smask = nullptr;
    if ((rc = tmp.upload(&d_tab, tab.data(), tab.size())) || (rc = tmp.upload(&d_moff, moff.data(), moff.size())) ||
        (rc = tmp.alloc(&d_zoops, s->n)) || (rc = tmp.alloc(&d_z, s->n)) ||
        (want_mops && (rc = pooled_mops ? tmp.scratch(&d_mops, (size_t)std::max<uint64_t>(1, moff[s->n])) : tmp.alloc(&d_mops, moff[s->n]))) ||
        (seq_mask && (rc = tmp.upload(&d_smask, seq_mask, s->n)))) return rc;
    // column slices carry a float per window from launch to launch: in the MOPS scores where the caller wants them, else in a
    // block of the context's scratch pool
    uint32_t cps = W;
    const uint32_t slices = score_slices(c, K, W, &cps);
    float* d_part = d_mops;
    if (slices > 1 && !d_part && (rc = tmp.scratch(&d_part, (size_t)std::max<uint64_t>(1, moff[s->n])))) return rc;
    if (seq_mask) {                                          // sequences outside the subset report zeros
        hipError_t e = hipMemsetAsync(d_zoops, 0, s->n * sizeof(float), st);
        if (e == hipSuccess) e = hipMemsetAsync(d_z, 0, s->n * sizeof(uint32_t), st);
        if (e == hipSuccess && want_mops) e = hipMemsetAsync(d_mops, 0, moff[s->n] * sizeof(float), st);
        if (e != hipSuccess) { set_error("hipMemsetAsync failed: %s", hipGetErrorString(e)); return BAMM_ERR_HIP; }
    }
    for (size_t bi = 0; bi < s->buckets.size() && !rc; bi++) {
        const Bucket& bk = s->buckets[bi];
        ScoreKernelArgs a{};
        a.sv = make_view(s, exc, bk.d_idx, bk.count, d_smask);
        a.K = K; a.W = W; a.Y = Y; a.s = d_tab; a.mops = d_mops; a.mops_off = d_moff; a.zoops = d_zoops; a.z = d_z;
        ScoreRoute route = score_route(c, bk, K, W);
        // the launches of one bucket: a.s whole, or a slice of its columns after the other on the context's stream
        auto per_slice = [&](auto&& launch) {
            int r = BAMM_OK;
            for (uint32_t j0 = 0; j0 < W && !r; j0 += cps) r = launch(ScoreSlice{d_part, j0, std::min(W, j0 + cps)});
            return r;
        };
        if (route == ScoreRoute::kTiles) {
            ScoreTileArgs ta{};
            std::vector<uint32_t> toff;
            (void)score_tile_geometry(W, nullptr, &ta.stride);
            const uint64_t tiles = bucket_tiles(s, bk, seq_mask, W, ta.stride, &toff);
            if (tiles == 0) continue;                        // every long sequence is outside the mask
            if (tiles <= UINT32_MAX) {
                uint32_t* d_toff = nullptr;
                ta.n_tiles = (uint32_t)tiles;
                if ((rc = tmp.upload(&d_toff, toff.data(), toff.size())) || (rc = tmp.alloc(&ta.tile_best, tiles)) ||
                    (rc = tmp.alloc(&ta.tile_idx, tiles))) return rc;
                ta.k = a; ta.k.sv.mask = nullptr; ta.tile_off = d_toff;
                const uint32_t waves = score_tile_threads() / 64u;
                const uint32_t tblocks = std::min(default_blocks(c, score_tile_threads()), (ta.n_tiles + waves - 1) / waves);
                rc = slices > 1 ? per_slice([&](const ScoreSlice& sl) { return launch_score_tiles_slice(ta, sl, tblocks, st); })
                                : launch_score_tiles(ta, tblocks, st);
                continue;
            }
            route = ScoreRoute::kWindows;                    // (more tiles than a launch indexes: 2^32 of them)
        }
        if (route == ScoreRoute::kWindows) {                 // same sums in the same order, the table read from global memory
            rc = launch_long_score(a, std::min(bk.count, (uint32_t)std::max(1, c->num_cus) * 8u), st);
            continue;
        }
        const uint32_t threads = default_threads(c, bk.mclass);
        uint32_t blocks = default_blocks(c, threads);
        blocks = std::max(1u, std::min(blocks, (bk.count + threads / 64u - 1) / (threads / 64u)));
        rc = slices > 1 ? per_slice([&](const ScoreSlice& sl) { return launch_score_slice(bk.mclass, a, sl, blocks, threads, st); })
                        : launch_score(bk.mclass, a, blocks, threads, st);
    }
    out->mops = d_mops; out->zoops = d_zoops; out->z = d_z;
    return rc;
}

// the widest slice whose columns fit the LDS, then the fewest slices, then those balanced
bool score_slice_geometry(uint32_t K, uint32_t W, uint32_t* columns_per_slice, uint32_t* slices) {
    const uint32_t cmax = (uint32_t)(kScoreLdsBytes / ((ipow4(K + 1) + 1) * sizeof(float)));
    if (W == 0 || cmax == 0) return false;
    const uint32_t S = (W + cmax - 1) / cmax;
    if (columns_per_slice) *columns_per_slice = (W + S - 1) / S;
    if (slices) *slices = S;
    return true;
}

}  // namespace bamm

extern "C" {

int bamm_score_slice_geometry(uint32_t K, uint32_t W, uint32_t* columns_per_slice, uint32_t* slices) {
    if (K > BAMM_MAX_ORDER || !score_slice_geometry(K, W, columns_per_slice, slices)) {
        set_error("bamm_score_slice_geometry: K=%u, W=%u: no column of the table fits the LDS", K, W);
        return BAMM_ERR_ARG;
    }
    return BAMM_OK;
}

int bamm_score_tile_geometry(uint32_t W, uint32_t* tile_positions, uint32_t* stride) {
    if (!score_tile_geometry(W, tile_positions, stride)) {
        set_error("bamm_score_tile_geometry: W=%u leaves a tile no stride of at least 16 positions", W);
        return BAMM_ERR_ARG;
    }
    return BAMM_OK;
}

int bamm_score_plan(bamm_ctx* c, const bamm_seqs* s, uint32_t K, uint32_t W, uint64_t* wave_seqs, uint64_t* tiled_seqs,
                    uint64_t* tiles, uint64_t* window_seqs) {
    if (!c || !s) { set_error("bamm_score_plan: null argument"); return BAMM_ERR_ARG; }
    if (K > BAMM_MAX_ORDER || W == 0) { set_error("bamm_score_plan: bad K/W"); return BAMM_ERR_ARG; }
    if (s->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    if (s->n && s->min_len < W) { set_error("a sequence is shorter than the motif (W=%u)", W); return BAMM_ERR_ARG; }
    uint64_t n[3] = {0, 0, 0}, nt = 0;
    uint32_t stride = 0;
    for (const Bucket& bk : s->buckets) {
        ScoreRoute route = score_route(c, bk, K, W);
        if (route == ScoreRoute::kTiles) {
            (void)score_tile_geometry(W, nullptr, &stride);
            const uint64_t t = bucket_tiles(s, bk, nullptr, W, stride, nullptr);
            if (t <= UINT32_MAX) nt += t; else route = ScoreRoute::kWindows;
        }
        n[(int)route] += bk.count;
    }
    if (wave_seqs) *wave_seqs = n[(int)ScoreRoute::kWave];
    if (tiled_seqs) *tiled_seqs = n[(int)ScoreRoute::kTiles];
    if (tiles) *tiles = nt;
    if (window_seqs) *window_seqs = n[(int)ScoreRoute::kWindows];
    return BAMM_OK;
}

int bamm_seed_from_pwm(bamm_ctx* c, bamm_seqs* s, uint32_t K, uint32_t W, const float* score, float q, const double* u,
                       int32_t* counts, uint32_t* z) {
    if (!c || !s || !score || !u || !counts) { set_error("bamm_seed_from_pwm: null argument"); return BAMM_ERR_ARG; }
    if (K > BAMM_MAX_ORDER || W == 0) { set_error("bamm_seed_from_pwm: bad K/W"); return BAMM_ERR_ARG; }
    if (s->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    const size_t vsz = v_size(K, W);
    std::fill(counts, counts + vsz, 0);
    if (s->n == 0) return BAMM_OK;
    BAMM_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    ExcK* exc = nullptr;
    int rc = exceptions_for_order(s, K, &exc);
    if (rc) return rc;
    float* d_score = nullptr;
    double* d_u = nullptr;
    int* d_counts = nullptr;
    uint32_t* d_z = nullptr;
    unsigned char* d_wave = nullptr;
    DevBlocks tmp(c);
    if ((rc = tmp.upload(&d_score, score, (size_t)4 * W)) || (rc = tmp.upload(&d_u, u, s->n)) ||
        (rc = tmp.alloc(&d_counts, vsz)) || (z && (rc = tmp.alloc(&d_z, s->n)))) return rc;
    if (hipMemsetAsync(d_counts, 0, vsz * sizeof(int), st) != hipSuccess) { set_error("hipMemsetAsync failed"); return BAMM_ERR_HIP; }
    SeedKernelArgs a{};
    a.sv = make_view(s, exc, nullptr, (uint32_t)s->n, nullptr);   // every sequence, natural order
    a.K = K; a.W = W; a.Y = (uint32_t)ipow4(K + 1);
    a.max_len = s->max_len; a.vsize = (uint32_t)vsz;
    a.score = d_score; a.q = q; a.u = d_u; a.counts = d_counts; a.z_out = d_z;
    if (const size_t need = seed_global_scratch_bytes(a, (uint32_t)std::max(1, c->num_cus))) {   // sequences beyond the LDS plan
        if ((rc = tmp.scratch(&d_wave, need))) return rc;
        a.wave_scratch = d_wave;
    }
    rc = launch_seed_pwm(a, (uint32_t)std::max(1, c->num_cus), st);
    if (!rc) {
        hipError_t e = ctx_download(c, counts, d_counts, vsz * sizeof(int)) ? hipErrorUnknown : hipSuccess;
        if (e == hipSuccess && z && ctx_download(c, z, d_z, s->n * sizeof(uint32_t))) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("bamm_seed_from_pwm: copy failed: %s", hipGetErrorString(e)); rc = BAMM_ERR_HIP; }
    }
    return rc;
}

int bamm_logodds(bamm_ctx* c, bamm_seqs* s, uint32_t K, uint32_t W, uint32_t bg_order, const float* v, const float* vbg,
                 float* mops, uint64_t mops_cap, float* zoops, uint64_t* z) {
    return bamm_logodds_subset(c, s, nullptr, K, W, bg_order, v, vbg, mops, mops_cap, zoops, z);
}

int bamm_logodds_subset(bamm_ctx* c, bamm_seqs* s, const uint8_t* seq_mask, uint32_t K, uint32_t W, uint32_t bg_order,
                        const float* v, const float* vbg, float* mops, uint64_t mops_cap, float* zoops, uint64_t* z) {
    if (!c || !s || !v || !vbg || !zoops || !z) { set_error("bamm_logodds: null argument"); return BAMM_ERR_ARG; }
    if (K > BAMM_MAX_ORDER || W == 0) { set_error("bamm_logodds: bad K/W"); return BAMM_ERR_ARG; }
    if (s->n && s->min_len < W) { set_error("a sequence is shorter than the motif (W=%u)", W); return BAMM_ERR_ARG; }
    if (s->n == 0) return BAMM_OK;
    BAMM_HIP(hipSetDevice(c->device));
    if (mops) {
        uint64_t windows = 0;
        for (uint64_t n = 0; n < s->n; n++) windows += s->h_len[n] - W + 1;
        if (mops_cap < windows) { set_error("mops buffer too small"); return BAMM_ERR_ARG; }
    }
    DevBlocks tmp(c);
    DeviceScores d;
    int rc = score_on_device(c, s, seq_mask, K, W, bg_order, v, vbg, mops != nullptr, false, tmp, &d);
    std::vector<uint32_t> hz(s->n);
    if (!rc) {
        hipError_t e = ctx_download(c, zoops, d.zoops, s->n * sizeof(float)) ? hipErrorUnknown : hipSuccess;
        if (e == hipSuccess && ctx_download(c, hz.data(), d.z, s->n * sizeof(uint32_t))) e = hipErrorUnknown;
        if (e == hipSuccess && mops && ctx_download(c, mops, d.mops, d.moff[s->n] * sizeof(float))) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { set_error("bamm_logodds: copy failed: %s", hipGetErrorString(e)); rc = BAMM_ERR_HIP; }
    }
    if (!rc) for (uint64_t n = 0; n < s->n; n++) z[n] = hz[n];
    return rc;
}

}  // extern "C"
