// extern "C" test hooks over the C++ host code (libbamm_host.so), so that the CPU test-suite can
// drive the FASTA reader, the seeders and the model-file writers through ctypes.
#include <algorithm>
#include <cstring>

#include <omp.h>

#include <charconv>
#include "bamm_host.h"
#include "host_util.h"
#include "slot_plan.h"
#include "../csrc/occ_pvalue.h"

using namespace bammhost;

static thread_local std::string g_err;

static BgModel bg_from(uint32_t order, const float* vbg) {
    BgModel bg;
    bg.K = order;
    bg.v.assign(vbg, vbg + bamm_bg_size(order));
    return bg;
}

// "<prefix>0", "<prefix>1", ... or, not numbered, the prefix n times
static std::vector<std::string> numbered_headers(const std::string& prefix, uint64_t n, bool numbered = true) {
    std::vector<std::string> headers;
    for (uint64_t i = 0; i < n; i++) headers.push_back(numbered ? prefix + std::to_string(i) : prefix);
    return headers;
}

extern "C" {

const char* bh_last_error(void) { return g_err.c_str(); }

// two-call protocol: first with codes == NULL to get sizes
int bh_read_fasta(const char* path, uint64_t* n_seqs, uint64_t* n_codes, uint8_t* codes, uint64_t* off, float* base_freq) {
    FastaSet fs;
    if (read_fasta(path, fs, g_err)) return 1;
    *n_seqs = fs.size();
    *n_codes = fs.codes.size();
    if (codes) {
        memcpy(codes, fs.codes.data(), fs.codes.size());
        memcpy(off, fs.off.data(), fs.off.size() * sizeof(uint64_t));
        if (base_freq) memcpy(base_freq, fs.base_freq, sizeof fs.base_freq);
    }
    return 0;
}

int bh_write_bg(const char* dir, const char* base, uint32_t K, const float* alpha, const float* v) {
    BgModel bg = bg_from(K, v);
    bg.alpha.assign(alpha, alpha + K + 1);
    return bg_write(dir, base, bg, g_err);
}

int bh_read_bg(const char* path, uint32_t* K, float* alpha, float* v, uint32_t cap_k) {
    BgModel bg;
    if (bg_read(path, bg, g_err)) return 1;
    if (bg.K > cap_k) { g_err = "order too high for the caller's buffers"; return 1; }
    *K = bg.K;
    memcpy(alpha, bg.alpha.data(), bg.alpha.size() * sizeof(float));
    memcpy(v, bg.v.data(), bg.v.size() * sizeof(float));
    return 0;
}

int bh_write_motif(const char* dir, const char* base, uint32_t W, uint32_t K, const float* v, uint32_t bg_order, const float* vbg) {
    Motif m;
    motif_alloc(m, W, K, std::vector<float>(K + 1, 1.f), 0.3f);
    m.v.assign(v, v + bamm_v_size(K, W));
    motif_calculate_p(m, bg_from(bg_order, vbg));
    return motif_write(dir, base, m, g_err);
}

// seeds: returns the number of motifs; v_out holds motif `index` (flat), w_out its width, q_out its q
static int load_seed_impl(const char* path, const char* tag, uint32_t l_flank, uint32_t r_flank, uint32_t K, const float* alpha,
                 uint64_t max_pwm, float glob_q, uint32_t bg_order, const float* vbg, const bamm_packed* packed,
                 uint32_t index, uint32_t* n_motifs, uint32_t* w_out, float* q_out, float* v_out, uint64_t v_cap,
                 const SeedDevice* dev) {
    std::vector<uint32_t> yK(packed->total_len ? packed->total_len : 1);
    if (bamm_unpack_y(packed, K, yK.data())) { g_err = bamm_last_error(); return 1; }
    SeedSet seeds;
    std::vector<float> al(alpha, alpha + K + 1);
    if (load_seeds(path, tag, l_flank, r_flank, K, al, max_pwm, glob_q, bg_from(bg_order, vbg), yK.data(), offsets_of(packed).data(), packed->n_seqs, seeds,
                   g_err, dev)) return 1;
    *n_motifs = (uint32_t)seeds.motifs.size();
    if (index >= seeds.motifs.size()) { g_err = "motif index out of range"; return 1; }
    const Motif& m = seeds.motifs[index];
    *w_out = m.W;
    *q_out = m.q;
    if (m.v.size() > v_cap) { g_err = "v buffer too small"; return 1; }
    memcpy(v_out, m.v.data(), m.v.size() * sizeof(float));
    return 0;
}

// Motif::initFromPWM on a caller-provided PWM ([4][W]): the model and the sampled site of every sequence, through
// the host path (std::mt19937 + std::discrete_distribution) or, with ctx/seqs, the device path
int bh_pwm_sites(const float* pwm, uint32_t W, uint32_t K, const float* alpha, uint32_t bg_order, const float* vbg,
                 const bamm_packed* packed, float q, float* v_out, uint32_t* z_out, bamm_ctx* ctx, bamm_seqs* seqs) {
    Motif m;
    motif_alloc(m, W, K, std::vector<float>(alpha, alpha + K + 1), q);
    std::vector<uint32_t> yK(packed->total_len ? packed->total_len : 1), z;
    if (bamm_unpack_y(packed, K, yK.data())) { g_err = bamm_last_error(); return 1; }
    const SeedDevice dev{ctx, seqs};
    if (motif_init_from_pwm(m, std::vector<float>(pwm, pwm + 4 * (size_t)W), bg_from(bg_order, vbg), yK.data(), offsets_of(packed).data(), packed->n_seqs, q,
                            ctx ? &dev : nullptr, g_err, &z)) return 1;
    memcpy(v_out, m.v.data(), m.v.size() * sizeof(float));
    memcpy(z_out, z.data(), z.size() * sizeof(uint32_t));
    return 0;
}

int bh_load_seed(const char* path, const char* tag, uint32_t l_flank, uint32_t r_flank, uint32_t K, const float* alpha,
                 uint64_t max_pwm, float glob_q, uint32_t bg_order, const float* vbg, const bamm_packed* packed,
                 uint32_t index, uint32_t* n_motifs, uint32_t* w_out, float* q_out, float* v_out, uint64_t v_cap) {
    return load_seed_impl(path, tag, l_flank, r_flank, K, alpha, max_pwm, glob_q, bg_order, vbg, packed, index, n_motifs,
                          w_out, q_out, v_out, v_cap, nullptr);
}

// the same with initFromPWM's pass over the sequences on the device (ctx / seqs: the uploaded `packed`)
int bh_load_seed_dev(const char* path, const char* tag, uint32_t l_flank, uint32_t r_flank, uint32_t K, const float* alpha,
                     uint64_t max_pwm, float glob_q, uint32_t bg_order, const float* vbg, const bamm_packed* packed,
                     uint32_t index, uint32_t* n_motifs, uint32_t* w_out, float* q_out, float* v_out, uint64_t v_cap,
                     bamm_ctx* ctx, bamm_seqs* seqs) {
    const SeedDevice dev{ctx, seqs};
    return load_seed_impl(path, tag, l_flank, r_flank, K, alpha, max_pwm, glob_q, bg_order, vbg, packed, index, n_motifs,
                          w_out, q_out, v_out, v_cap, &dev);
}

// ---- de novo seeds (seeder.cpp) ----
// kmer_seeds on a caller-provided table: *n_out seeds (at most max_seeds); kmer / count / z hold max_seeds entries, pwm
// max_seeds x [4][w]
int bh_kmer_seeds(const uint64_t* counts, uint64_t n_windows, uint32_t w, uint32_t bg_order, const float* vbg, uint64_t max_seeds,
                  int ss, uint32_t* n_out, uint32_t* kmer, uint64_t* count, double* z, float* pwm) {
    std::vector<KmerSeed> seeds;
    kmer_seeds(counts, n_windows, w, bg_from(bg_order, vbg), (size_t)max_seeds, ss != 0, seeds);
    *n_out = (uint32_t)seeds.size();
    for (size_t i = 0; i < seeds.size(); i++) {
        kmer[i] = seeds[i].kmer; count[i] = seeds[i].count; z[i] = seeds[i].z;
        memcpy(pwm + i * 4 * (size_t)w, seeds[i].pwm.data(), 4 * (size_t)w * sizeof(float));
    }
    return 0;
}

int bh_kmer_seeds_write(const char* path, uint32_t w, uint32_t n, const uint32_t* kmer, const uint64_t* count, const double* z, const float* pwm) {
    std::vector<KmerSeed> seeds(n);
    for (uint32_t i = 0; i < n; i++) {
        seeds[i].kmer = kmer[i]; seeds[i].count = count[i]; seeds[i].z = z[i];
        seeds[i].pwm.assign(pwm + i * 4 * (size_t)w, pwm + (i + 1) * 4 * (size_t)w);
    }
    return kmer_seeds_write(path, w, seeds, g_err);
}

// kmer_seeds_gapped on caller-provided tables: as bh_kmer_seeds, with gap[max_seeds] and pwm max_seeds x [4][w + gap_hi]
// (seed i's [4][w + gap[i]] at the start of its slot)
int bh_kmer_seeds_gapped(const uint64_t* counts, const uint64_t* n_windows, uint32_t w, uint32_t gap_lo, uint32_t gap_hi, uint32_t bg_order,
                         const float* vbg, uint64_t max_seeds, int ss, uint32_t* n_out, uint32_t* kmer, uint32_t* gap, uint64_t* count,
                         double* z, float* pwm) {
    if (w < 6 || w > 8 || gap_lo > gap_hi || w + gap_hi > 16 || ((w & 1u) && gap_hi)) { g_err = "bh_kmer_seeds_gapped: bad w or gaps"; return 1; }
    std::vector<KmerSeed> seeds;
    kmer_seeds_gapped(counts, n_windows, w, gap_lo, gap_hi, bg_from(bg_order, vbg), (size_t)max_seeds, ss != 0, seeds);
    *n_out = (uint32_t)seeds.size();
    for (size_t i = 0; i < seeds.size(); i++) {
        kmer[i] = seeds[i].kmer; gap[i] = seeds[i].gap; count[i] = seeds[i].count; z[i] = seeds[i].z;
        memcpy(pwm + i * 4 * (size_t)(w + gap_hi), seeds[i].pwm.data(), seeds[i].pwm.size() * sizeof(float));
    }
    return 0;
}

// kmer_seeds_write for seeds with gaps: pwm as bh_kmer_seeds_gapped lays it out, slots of [4][w + max_gap]
int bh_kmer_seeds_write_gapped(const char* path, uint32_t w, uint32_t max_gap, uint32_t n, const uint32_t* kmer, const uint32_t* gap,
                               const uint64_t* count, const double* z, const float* pwm) {
    std::vector<KmerSeed> seeds(n);
    for (uint32_t i = 0; i < n; i++) {
        if (gap[i] > max_gap) { g_err = "bh_kmer_seeds_write_gapped: a gap above max_gap"; return 1; }
        seeds[i].kmer = kmer[i]; seeds[i].gap = gap[i]; seeds[i].count = count[i]; seeds[i].z = z[i];
        const float* at = pwm + i * 4 * (size_t)(w + max_gap);
        seeds[i].pwm.assign(at, at + 4 * (size_t)(w + gap[i]));
    }
    return kmer_seeds_write(path, w, seeds, g_err);
}

// the MEME reader of load_seeds on its own: motif `index` of the file as [4][*w_out] floats; *n_motifs = motifs in the file
int bh_read_meme_pwm(const char* path, uint32_t index, uint32_t* n_motifs, uint32_t* w_out, float* pwm_out, uint64_t pwm_cap) {
    uint32_t seen = 0;
    int bad = 0;
    if (read_meme_pwms(path, 0, 0, 0.3f, g_err, [&](uint32_t W, float, const std::vector<float>& pwm) {
            if (seen++ == index) {
                if (pwm.size() > pwm_cap) { g_err = "pwm buffer too small"; bad = 1; return 1; }
                *w_out = W;
                memcpy(pwm_out, pwm.data(), pwm.size() * sizeof(float));
            }
            return 0;
        })) return 1;
    *n_motifs = seen;
    if (index >= seen) { g_err = "motif index out of range"; return 1; }
    return bad;
}

// OpenMP threads of the host-side loops (the CLI's --threads)
void bh_set_threads(int n) { omp_set_num_threads(n > 0 ? n : 1); set_host_parallelism(n > 0 ? n : 1); }
void bh_auto_threads() { set_host_parallelism(0); }

const char* bh_base_name(const char* path) {
    g_err = base_name(path);
    return g_err.c_str();
}

// the per-window formula the host and the device path share (csrc/occ_pvalue.h) on caller-provided ranks and neighbours
int bh_occ_window_pvalues(const float* score, const uint64_t* fp, const float* higher, const float* lower, uint64_t n,
                          const float* lowest, uint64_t negN, float* p_out, float* s_ntop, float* lambda, uint32_t* n_top) {
    const bamm::OccScalars sc = bamm::occ_scalars(lowest, negN);
    for (uint64_t i = 0; i < n; i++) p_out[i] = bamm::occ_window_pvalue(score[i], fp[i], higher[i], lower[i], sc);
    *s_ntop = sc.S_ntop; *lambda = sc.lambda; *n_top = (uint32_t)sc.nTop;
    return 0;
}

int bh_occurrence_hits(const char* dir, const char* base, const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int ss,
                       uint32_t W, uint64_t n_hits, const uint64_t* seq, const uint32_t* pos, const float* p, const float* e) {
    return occurrence_write_hits(dir, base, numbered_headers("seq", n_seqs), codes, off, n_seqs, ss != 0, W, n_hits, seq, pos, p, e, g_err);
}

// EM::write's .positions from a site list / from dense r; headers: n_seqs C strings
int bh_positions_hits(const char* dir, const char* base, const char* const* headers, const uint8_t* codes, const uint64_t* off,
                      uint64_t n_seqs, int ss, uint32_t W, uint64_t n_hits, const uint64_t* seq, const uint32_t* pos) {
    const std::vector<std::string> hd(headers, headers + n_seqs);
    return positions_write_hits(dir, base, hd, codes, off, n_seqs, ss != 0, W, n_hits, seq, pos, g_err);
}

int bh_positions(const char* dir, const char* base, const char* const* headers, const uint8_t* codes, const uint64_t* off,
                 uint64_t n_seqs, int ss, uint32_t W, const float* r, float cutoff) {
    const std::vector<std::string> hd(headers, headers + n_seqs);
    return positions_write(dir, base, hd, codes, off, n_seqs, ss != 0, W, r, cutoff, g_err);
}

// ---- evaluation-side hooks ---------------------------------------------------------------

// negatives for a packed (positive) set; two-call protocol (codes == NULL -> sizes only)
// keep_stride > 1: only every keep_stride-th negative (what --FDR scores, FDR.cpp:58-60) is generated and returned
int bh_sample_negatives_strided(const bamm_packed* packed, uint32_t s_order, uint64_t m_fold, int generic, uint64_t keep_stride,
                                uint64_t* n_out, uint64_t* n_codes, uint8_t* codes, uint64_t* off) {
    static thread_local ByteVec c;
    static thread_local std::vector<uint64_t> o;
    if (!codes) {
        std::vector<uint32_t> ys(packed->total_len ? packed->total_len : 1);
        if (bamm_unpack_y(packed, s_order, ys.data())) { g_err = bamm_last_error(); return 1; }
        if (sample_negatives(ys.data(), offsets_of(packed).data(), packed->n_seqs, s_order, m_fold, generic != 0, c, o, g_err, (size_t)keep_stride)) return 1;
        *n_out = o.size() - 1;
        *n_codes = c.size();
        return 0;
    }
    memcpy(codes, c.data(), c.size());
    memcpy(off, o.data(), o.size() * sizeof(uint64_t));
    return 0;
}
int bh_sample_negatives(const bamm_packed* packed, uint32_t s_order, uint64_t m_fold, int generic, uint64_t* n_out,
                        uint64_t* n_codes, uint8_t* codes, uint64_t* off) {
    return bh_sample_negatives_strided(packed, s_order, m_fold, generic, 0, n_out, n_codes, codes, off);
}

int bh_fdr_stats(const float* pos_max, uint64_t n_pos_max, const float* neg_max, uint64_t n_neg_max, const float* pos_all,
                 uint64_t n_pos_all, const float* neg_all, uint64_t n_neg_all, uint64_t posN, uint64_t negN, float q, int mops,
                 int zoops, int save_pvalues, const char* dir, const char* base) {
    FdrResult r;
    fdr_statistics(std::vector<float>(pos_max, pos_max + n_pos_max), std::vector<float>(neg_max, neg_max + n_neg_max),
                   std::vector<float>(pos_all, pos_all + n_pos_all), std::vector<float>(neg_all, neg_all + n_neg_all), posN, negN,
                   q, mops != 0, zoops != 0, save_pvalues != 0, r);
    return fdr_write(dir, base, r, posN, negN, mops != 0, zoops != 0, true, save_pvalues != 0, g_err);
}

// the MOPS half of fdr_statistics as arrays: tp / fp (n_pos + n_neg values), fdr / rec (*n_rows values; room for n_pos + n_neg),
// the p-values of the ascending positives (n_pos values); any array may be NULL
int bh_fdr_mops_rows(const float* pos_all, uint64_t n_pos, const float* neg_all, uint64_t n_neg, uint64_t posN, uint64_t negN,
                     uint64_t* n_rows, float* occ_mult, float* tp, float* fp, float* fdr, float* rec, float* pvalues) {
    FdrResult r;
    fdr_statistics({}, {}, std::vector<float>(pos_all, pos_all + n_pos), std::vector<float>(neg_all, neg_all + n_neg), posN, negN, 0.f,
                   true, false, pvalues != nullptr, r);
    auto out = [](float* dst, const std::vector<float>& v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(float)); };
    if (n_rows) *n_rows = r.mops_fdr.size();
    if (occ_mult) *occ_mult = r.occ_mult;
    out(tp, r.mops_tp); out(fp, r.mops_fp); out(fdr, r.mops_fdr); out(rec, r.mops_rec); out(pvalues, r.mops_pvalue);
    return 0;
}

// .mops.stats / .mops.pvalues from caller-provided rows, handed to the writer `chunk` rows at a time through its fetchers
int bh_fdr_mops_chunked(const float* tp, const float* fp, const float* fdr, const float* rec, uint64_t n_rows, const float* p, uint64_t n_p,
                        float occ_mult, uint64_t chunk, const char* dir, const char* base) {
    return fdr_write_mops_chunked(dir, base, occ_mult, n_rows,
        [&](uint64_t a, uint64_t b, float* t, float* f, float* d, float* r, std::string&) {
            std::copy(tp + a, tp + b, t); std::copy(fp + a, fp + b, f); std::copy(fdr + a, fdr + b, d); std::copy(rec + a, rec + b, r);
            return 0;
        },
        n_p, [&](uint64_t a, uint64_t b, float* out, std::string&) { std::copy(p + a, p + b, out); return 0; }, true, true, g_err, chunk);
}

// tests: format_g against std::to_chars (which is printf's %g) on n floats; returns the number of differing strings and
// the first offender's bits
uint64_t bh_format_g_check(const float* x, uint64_t n, int precision, uint32_t* first_bad_bits) {
    uint64_t bad = 0;
    char a[48], b[48];
    for (uint64_t i = 0; i < n; i++) {
        const size_t la = format_g(a, x[i], precision);
        const size_t lb = (size_t)(std::to_chars(b, b + sizeof b, x[i], std::chars_format::general, precision).ptr - b);
        if (la != lb || memcmp(a, b, la)) { if (!bad && first_bad_bits) memcpy(first_bad_bits, &x[i], 4); bad++; }
    }
    return bad;
}

// --saveLogOdds writers on caller-provided scores
int bh_fdr_logodds(const float* pos_max, uint64_t n_pos_max, const float* neg_max, uint64_t n_neg_max, const float* pos_all,
                   uint64_t n_pos_all, const float* neg_all, uint64_t n_neg_all, uint64_t posN, uint64_t negN, int mops, int zoops,
                   int ascending, const char* dir, const char* base) {
    return fdr_logodds_write(dir, base, std::vector<float>(pos_max, pos_max + n_pos_max), std::vector<float>(neg_max, neg_max + n_neg_max),
                             std::vector<float>(pos_all, pos_all + n_pos_all), std::vector<float>(neg_all, neg_all + n_neg_all), posN, negN,
                             mops != 0, zoops != 0, ascending != 0, g_err);
}

int bh_logodds_zoops(const char* dir, const char* base, const char* header_prefix, int number_headers, const uint8_t* codes,
                     const uint64_t* off, uint64_t n_seqs, int revcomp, int ss, uint32_t W, const float* zoops, const uint64_t* z) {
    return logodds_zoops_write(dir, base, numbered_headers(header_prefix, n_seqs, number_headers != 0), codes, off, n_seqs, revcomp != 0, ss != 0, W, zoops, z, g_err);
}

int bh_mops_pvalues(const float* pos_scores, uint64_t n_pos, const float* neg_all, uint64_t n_neg, uint64_t posN, float* p_out,
                    float* e_out) {
    std::vector<float> p, e;
    mops_pvalues(pos_scores, n_pos, std::vector<float>(neg_all, neg_all + n_neg), posN, p, e);
    memcpy(p_out, p.data(), p.size() * sizeof(float));
    memcpy(e_out, e.data(), e.size() * sizeof(float));
    return 0;
}

int bh_occurrence(const char* dir, const char* base, const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int ss,
                  uint32_t W, const float* p, const float* e, float cutoff) {
    return occurrence_write(dir, base, numbered_headers("seq", n_seqs), codes, off, n_seqs, ss != 0, W, p, e, cutoff, g_err);
}

// the CLI's GPU slot plan (slot_plan.h) as arrays: devices, em_slots, in_em_group and runs_folds hold n_slots entries (the
// first *n_em of em_slots are set), fold_slot max(1, cv_fold)
int bh_slot_plan(uint64_t n_slots, uint64_t cv_fold, int em, int fdr, int one_slot_chain, const int* devices, uint64_t* n_em,
                 uint64_t* em_slots, uint64_t* fold_slot, int* overlap, int* sharded, int* distinct, uint8_t* in_em_group, uint8_t* runs_folds) {
    const SlotPlan p = make_slot_plan(n_slots, cv_fold, em != 0, fdr != 0, one_slot_chain != 0, std::vector<int>(devices, devices + n_slots));
    *n_em = p.em_slots.size();
    std::copy(p.em_slots.begin(), p.em_slots.end(), em_slots);
    std::copy(p.fold_slot.begin(), p.fold_slot.end(), fold_slot);
    *overlap = p.overlap; *sharded = p.sharded; *distinct = p.distinct;
    for (uint64_t d = 0; d < n_slots; d++) { in_em_group[d] = p.in_em_group(d); runs_folds[d] = p.runs_folds(d); }
    return 0;
}

}  // extern "C"
