// Evaluation and output side of the BaMMmotif drop-in, in bamm_host.h's order: the negative set, the FDR / PR statistics
// and window p-values, the files.  Restated from the reference lines cited in bamm_host.h; fp32 expression order kept.
#include <omp.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <thread>

#include "bamm_host.h"
#include "neg_sampler.h"
#include "row_text.h"
#include "../csrc/occ_pvalue.h"
#include "../csrc/fdr_rows.h"

namespace bammhost {

// ---------------------------------------------------------------------------------- negatives ----
// Host threads for work whose result does not depend on how it is cut (this sampler, packing, sorts): every core
// the process may use -- the affinity mask capped by the cgroup CPU quota -- whatever --threads says (the
// reference's flag sized its OpenMP EM loops, Global.cpp:331-333; a container may show 256 CPUs and grant 16).
static std::atomic<int> g_parallelism_override{0};
void set_host_parallelism(int n) { g_parallelism_override.store(n > 0 ? n : 0); }
int host_parallelism() {
    if (const int forced = g_parallelism_override.load()) return forced;
    static const int n = [] {
        int c = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) c = CPU_COUNT(&set);
        std::ifstream f("/sys/fs/cgroup/cpu.max");
        std::string quota;
        double period = 0;
        if (f >> quota >> period && quota != "max" && period > 0) c = std::min(c, std::max(1, (int)(std::stod(quota) / period + 0.5)));
        return std::max(1, std::min(c, 64));
    }();
    return n;
}

int sample_negatives(const uint32_t* y_s, const uint64_t* off, size_t n_seqs, uint32_t s_order, size_t m_fold,
                     bool generic, ByteVec& codes_out, std::vector<uint64_t>& off_out, std::string& err, size_t keep_stride) {
    if (!generic && s_order != 2) {
        err = "Error: the sequence-specific negative sampler is written for -s 2 (SeqGenerator.cpp:112-186); use --genericNeg";
        return 1;
    }
    NegSampler g(s_order);
    g.stream.start();                                  // SeqGenerator.cpp:35: the stream as srand(42) leaves it
    // libc itself is touched only where its rand() is not the restated generator (then the draws below come from it, one
    // thread): this function runs on a thread beside the main one in the CLI, and libc's stream is process-global
    if (!g.stream.fast) srand(42);
    g.kmer_frequency(y_s, off, n_seqs);
    // Every negative consumes exactly L draws of the one rand() stream, in order, so where each positive
    // sequence's draws start is known up front.  With the restated generator (stream.fast) the stream
    // is cut into contiguous ranges, every range jumps to its first draw (GlibcRandStream::jump) and the ranges
    // are sampled on separate threads -- same draws, same negatives.
    // Which negatives are kept under keep_stride, where each positive's draws start and where its kept negatives go is
    // csrc/neg_layout.h's, shared with the device sampler.
    const bamm::NegLayout lay(n_seqs, [&](uint64_t i) { return off[i + 1] - off[i]; }, m_fold, keep_stride);
    const std::vector<uint64_t>& d0 = lay.draw0;             // first draw of positive i
    const std::vector<uint64_t>& k0 = lay.first_kept;        // first kept negative of positive i
    std::vector<uint64_t> c0(n_seqs + 1, 0);                 // first output byte of positive i
    for (size_t i = 0; i < n_seqs; i++) c0[i + 1] = c0[i] + (off[i + 1] - off[i]) * lay.n_kept(i);
    codes_out.resize((size_t)c0[n_seqs]);                     // every byte is written by the range that owns it
    off_out.assign((size_t)lay.n_neg() + 1, 0);
    const int threads = host_parallelism();
    const bool parallel = g.stream.fast && threads > 1 && n_seqs >= 256;
    const size_t P = parallel ? (size_t)threads : 1;
    std::vector<size_t> first(P + 1, n_seqs);
    first[0] = 0;
    for (size_t p = 1; p < P; p++)                            // ranges of about equal numbers of draws
        first[p] = (size_t)(std::lower_bound(d0.begin(), d0.end(), d0[n_seqs] * p / P) - d0.begin());
    for (size_t p = 1; p <= P; p++) first[p] = std::max(first[p], first[p - 1]);
    first[P] = n_seqs;
    std::vector<decltype(g.stream)> start(P, g.stream);
    for (size_t p = 1; p < P; p++) start[p].jump(d0[first[p]]);   // nobody steps through the stream
#pragma omp parallel for schedule(static, 1) num_threads((int)P)
    for (long p = 0; p < (long)P; p++) {
        NegSampler w = g;                                      // own tables (rescale writes them), own stream position
        w.stream = start[(size_t)p];
        std::vector<float> rnd2;
        std::vector<size_t> ctx2;
        std::vector<uint8_t> keep_f(m_fold, 1);
        for (size_t i = first[(size_t)p]; i < first[(size_t)p + 1]; i++) {
            const size_t L = off[i + 1] - off[i];
            // the reference recomputes the rescaled tables for every fold (SeqGenerator.cpp:296); they
            // only depend on the positive sequence, so once per sequence gives the same tables
            if (!generic) w.rescale(y_s + off[i], L);
            size_t nk = 0;
            for (size_t f = 0; f < m_fold; f++) {
                keep_f[f] = lay.kept(i, f) ? 1 : 0;
                if (keep_f[f]) { off_out[(size_t)k0[i] + nk + 1] = c0[i] + L * (nk + 1); nk++; }
            }
            w.draw_many(L, m_fold, codes_out.data() + c0[i], rnd2, ctx2, keep_stride > 1 ? keep_f.data() : nullptr);
        }
    }
    return 0;
}

// --------------------------------------------------------------------------------- statistics ----
// Scores in the reference's order (std::sort with greater / less, FDR.cpp:158-159,203-204,288-289) on every granted core:
// sorted runs per thread, merged pairwise.  A sorted sequence of floats is the same whatever produced it (equal
// scores are indistinguishable -- the rare +0 / -0 pair aside, which no statistic tells apart).
void sort_scores(std::vector<float>& v, bool descending) {
    const size_t n = v.size();
    const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)host_parallelism(), n / 100000 + 1));
    auto less = [descending](float a, float b) { return descending ? a > b : a < b; };
    if (T == 1) { std::sort(v.begin(), v.end(), less); return; }
    std::vector<size_t> cut(T + 1);
    for (size_t t = 0; t <= T; t++) cut[t] = n * t / T;
#pragma omp parallel for schedule(static, 1) num_threads((int)T)
    for (long t = 0; t < (long)T; t++) std::sort(v.begin() + cut[t], v.begin() + cut[t + 1], less);
    for (size_t w = 1; w < T; w *= 2) {                   // runs of w ranges -> runs of 2w
        const long pairs = (long)((T + 2 * w - 1) / (2 * w));
#pragma omp parallel for schedule(static, 1) num_threads((int)T)
        for (long p = 0; p < pairs; p++) {
            const size_t a = (size_t)p * 2 * w, m = std::min(T, a + w), b = std::min(T, a + 2 * w);
            if (m < b) std::inplace_merge(v.begin() + cut[a], v.begin() + cut[m], v.begin() + cut[b], less);
        }
    }
}

void fdr_statistics(std::vector<float> posMax, std::vector<float> negMax, std::vector<float> posAll,
                    std::vector<float> negAll, size_t posN, size_t negN, float q, bool mops, bool zoops,
                    bool with_pvalues, FdrResult& r) {
    r = FdrResult();
    const float mFold = bamm::fdr_mfold(posN, negN);
    srand(42);                                         // FDR.cpp:153
    if (mops) {                                        // FDR.cpp:156-196; the numbers are csrc/fdr_rows.h's, as on the device (csrc/fdr.hip)
        sort_scores(posAll, true);
        sort_scores(negAll, true);
        size_t ip = 0, in = 0;
        float E_TP = 0.0f;
        size_t idx_max = posN + negN;
        const size_t len_all = posAll.size() + negAll.size();
        for (size_t i = 0; i < len_all; i++) {
            // the reference indexes past the end of both vectors here (FDR.cpp:174); an exhausted
            // list is treated as "-inf" instead of reading stale heap memory
            const bool take_pos = (ip < posAll.size()) && (in >= negAll.size() || posAll[ip] > negAll[in]);
            if (take_pos) ip++; else in++;
            r.mops_tp.push_back(bamm::fdr_tp(ip, in, mFold));
            r.mops_fp.push_back(bamm::fdr_fp(in, mFold));
            const bamm::FdrPeakStep step = bamm::fdr_peak_step(E_TP, r.mops_tp[i]);
            if (step.equal) idx_max = i;
            E_TP = step.e_tp;
        }
        for (size_t i = 0; i < idx_max && i < len_all; i++) {
            r.mops_fdr.push_back(bamm::fdr_fdr(r.mops_tp[i], r.mops_fp[i]));
            r.mops_rec.push_back(bamm::fdr_rec(r.mops_tp[i], E_TP));
        }
        r.occ_mult = E_TP / (float)posN;
    }
    if (zoops) {                                       // FDR.cpp:199-275
        sort_scores(posMax, true);
        sort_scores(negMax, true);
        size_t ip = 0, in = 0, min_idx_pos = 0;
        const size_t posN_est = static_cast<size_t>(q * (float)posN);
        // The strided CV split (FDR.cpp:49-60) drops the last posN % cvFold positives and keeps
        // cvFold * floor(negN / cvFold) negative scores, so the lists can be shorter than posN / negN.  The
        // reference walks posN + negN steps regardless and reads past the end of both (FDR.cpp:227-239);
        // here the walk covers the scores that exist -- the same rows whenever the counts divide evenly.
        const size_t nP = posMax.size(), nN = negMax.size();
        size_t n_top = (size_t)std::fmin(100, negN / 10);
        if (n_top >= nN) n_top = nN ? nN - 1 : 0;
        float lambda = 1e-16f;
        for (size_t l = 0; l < n_top; l++) lambda += negMax[l] - negMax[n_top];
        lambda /= n_top;
        float Sl = 0.f;
        auto P = [&](size_t i) { return i < nP ? posMax[i] : -INFINITY; };
        auto N = [&](size_t i) { return i < nN ? negMax[i] : -INFINITY; };
        // the walk itself is a serial chain (which list the next score comes from, one rand() per tie): it only
        // records, per step, the score and the two counts; everything computed FROM those -- the p-value with its two
        // binary searches, FDR, recall: most of the time at 2.2 M steps -- is then filled in on every granted core by
        // the same expressions
        const size_t steps = nP + nN;
        std::vector<float> step_score(steps);
        std::vector<uint32_t> step_ip(steps), step_in(steps);
        for (size_t i = 0; i < steps; i++) {
            if ((P(ip) > N(in) || ip == 0 || in >= nN) && ip < nP) {
                Sl = posMax[ip];
                ip++;
            } else if (P(ip) == N(in) && rand() % 2 == 0 && ip < nP) {       // same evaluation order: rand() drawn on every tie
                Sl = posMax[ip];
                ip++;
            } else {
                Sl = negMax[in];                                             // in < nN: both lists cannot be exhausted inside the walk
                in++;
            }
            step_score[i] = Sl; step_ip[i] = (uint32_t)ip; step_in[i] = (uint32_t)in;
            if (ip == posN_est) min_idx_pos = i;
        }
        r.zoops_tp.resize(steps); r.zoops_fp.resize(steps); r.pn_pvalue.resize(steps);
        r.zoops_fdr.resize(steps); r.zoops_rec.resize(steps);
#pragma omp parallel for schedule(static) num_threads(host_parallelism())
        for (long ii = 0; ii < (long)steps; ii++) {
            const size_t i = (size_t)ii, in = step_in[i];
            const float Sl = step_score[i];
            const float TP = (float)step_ip[i], FP = (float)in / mFold;
            r.zoops_tp[i] = TP;
            r.zoops_fp[i] = FP;
            float p_value;
            if (nN && Sl <= negMax[n_top]) {
                auto lo = std::lower_bound(negMax.begin(), negMax.end(), Sl, std::greater<float>());
                auto up = std::upper_bound(negMax.begin(), negMax.end(), Sl, std::greater<float>());
                const float Sl_upper = (lo == negMax.begin()) ? Sl : *(lo - 1);
                // for scores at or below the lowest negative the reference dereferences end() (FDR.cpp:244);
                // with its vectors that is untouched zero-filled heap, so 0 is what it computes with
                const float Sl_lower = (up == negMax.end()) ? 0.0f : *up;
                p_value = (in + (Sl_upper - Sl) / (Sl_upper - Sl_lower + 1e-5)) / (float)negN;
            } else if (nN) {
                p_value = n_top * expf((negMax[n_top] - Sl) / lambda) / negN;
            } else {
                p_value = 1.0f;                                              // no negative score at all
            }
            r.pn_pvalue[i] = p_value;
            r.zoops_fdr[i] = FP / (TP + FP);
            r.zoops_rec[i] = TP / (float)posN;
        }
        r.occ_frac = r.zoops_fp.empty() ? 1.0f : 1.0f - r.zoops_fp[min_idx_pos] / (float)posN;
    }
    if (with_pvalues) {                                // FDR.cpp:278-333
        auto pv = [](std::vector<float>& pos, std::vector<float>& neg, std::vector<float>& out) {
            sort_scores(neg, false);
            sort_scores(pos, false);
            for (size_t i = 0; i < pos.size(); i++) {
                const size_t low = std::lower_bound(neg.begin(), neg.end(), pos[i]) - neg.begin();
                const size_t up = std::upper_bound(neg.begin(), neg.end(), pos[i]) - neg.begin();
                out.push_back(bamm::fdr_pvalue(low, up, neg.size()));
            }
        };
        if (mops) pv(posAll, negAll, r.mops_pvalue);
        if (zoops) pv(posMax, negMax, r.zoops_pvalue);
    }
}

void mops_pvalues(const float* pos_scores, size_t n_pos_scores, std::vector<float> neg, size_t posN,
                  std::vector<float>& p_out, std::vector<float>& e_out) {
    const size_t negN = neg.size();                    // ScoreSeqSet.cpp:75-93
    std::sort(neg.begin(), neg.end(), std::less<float>());
    const bamm::OccScalars sc = bamm::occ_scalars(neg.data(), negN);
    p_out.resize(n_pos_scores);
    e_out.resize(n_pos_scores);
    for (size_t i = 0; i < n_pos_scores; i++) {        // ScoreSeqSet.cpp:97-125: the branches are occ_window_pvalue's
        const float Sl = pos_scores[i];
        const size_t FPl = neg.end() - std::upper_bound(neg.begin(), neg.end(), Sl);
        float SlHigher = 0.f, SlLower = 0.f;
        if (bamm::occ_uses_neighbours(FPl, sc)) { SlHigher = neg[negN - FPl - 1]; SlLower = neg[negN - FPl]; }
        const float p = bamm::occ_window_pvalue(Sl, FPl, SlHigher, SlLower, sc);
        p_out[i] = p;
        e_out[i] = p * (float)posN;
    }
}

// -------------------------------------------------------------------------------------- files ----
// `ostream << float` at precision P, i.e. printf's %.Pg, without the general-purpose machinery: the P significant digits
// come from one double multiplication (a float times a power of ten up to 1e22 is one rounding away from exact) and
// are used only when that rounding cannot have changed them -- the scaled value further than 1e-6 from a half; anything
// else (zero, non-finite, exponents beyond the exact powers, the rare near-tie) goes to std::to_chars, which IS %g.
// 11 M numbers per .stats file: most of what the file costs.
size_t format_g(char* out, float xf, int P) {
    static const double p10[] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    auto slow = [&]() { return (size_t)(std::to_chars(out, out + 40, xf, std::chars_format::general, P).ptr - out); };
    if (P < 1 || P > 9 || !(xf == xf) || xf == 0.0f || std::isinf(xf)) return slow();
    char* o = out;
    double x = (double)xf;
    if (x < 0) { *o++ = '-'; x = -x; }
    int e2;
    (void)std::frexp(x, &e2);                                // x in [2^(e2-1), 2^e2)
    int e = (int)std::floor((e2 - 1) * 0.30102999566398120); // floor(log10(x)) or one below
    if (e < -15 || e > 15) return slow();
    auto ge_pow = [&](int k) { return k >= 0 ? x >= p10[k] : x * p10[-k] >= 1.0; };   // x >= 10^k (x * 10^-k exact enough: checked again below)
    if (ge_pow(e + 1)) e++;
    const int k = P - 1 - e;                                 // scale to P digits in front of the point
    if (k < -22 || k > 22) return slow();
    double v = k >= 0 ? x * p10[k] : x / p10[-k];
    const double lo = p10[P - 1], hi = p10[P];
    if (v < lo || v >= hi) {                                 // e was one off at a power of ten (x * 10^-k rounding): settle it exactly
        if (v < lo) { e--; } else { e++; }
        const int k2 = P - 1 - e;
        if (k2 < -22 || k2 > 22) return slow();
        v = k2 >= 0 ? x * p10[k2] : x / p10[-k2];
        if (v < lo || v >= hi) return slow();
    }
    uint64_t m = (uint64_t)v;
    const double frac = v - (double)m;
    if (std::fabs(frac - 0.5) < 1e-6) return slow();         // too close to a tie for one rounding to be trusted
    if (frac > 0.5 && ++m == (uint64_t)hi) { m = (uint64_t)lo; e++; }
    char dig[16];
    for (int i = P - 1; i >= 0; i--) { dig[i] = (char)('0' + m % 10); m /= 10; }
    int nd = P;
    while (nd > 1 && dig[nd - 1] == '0') nd--;               // %g drops trailing zeros
    if (e < -4 || e >= P) {                                  // d.ddde+XX
        *o++ = dig[0];
        if (nd > 1) { *o++ = '.'; memcpy(o, dig + 1, (size_t)nd - 1); o += nd - 1; }
        *o++ = 'e';
        int ae = e;
        if (ae < 0) { *o++ = '-'; ae = -ae; } else { *o++ = '+'; }
        *o++ = (char)('0' + ae / 10); *o++ = (char)('0' + ae % 10);
    } else if (e >= 0) {
        const int ip = e + 1;                                // digits in front of the point (<= P)
        for (int i = 0; i < ip; i++) *o++ = i < nd ? dig[i] : '0';
        if (nd > ip) { *o++ = '.'; memcpy(o, dig + ip, (size_t)(nd - ip)); o += nd - ip; }
    } else {
        *o++ = '0'; *o++ = '.';
        for (int i = 0; i < -e - 1; i++) *o++ = '0';
        memcpy(o, dig, (size_t)nd); o += nd;
    }
    return (size_t)(o - out);
}

// .mops.stats / .mops.pvalues (FDR.cpp:409-425, :428-449 at setprecision(3)) from rows that are fetched range by range
// (the device path: bamm_fdr_rows / bamm_fdr_pvalues): `chunk` rows on the host at a time instead of every window's
int fdr_write_mops_chunked(const std::string& dir, const std::string& basename, float occ_mult, uint64_t n_rows, const FdrRowFetch& rows,
                           uint64_t n_pvalues, const FdrPvalueFetch& pvalues, bool save_prs, bool save_pvalues, std::string& err,
                           uint64_t chunk) {
    if (chunk == 0) { err = "Error: the MOPS files cannot be written zero rows at a time"; return 1; }
    const std::string opath = dir + '/' + basename;
    std::vector<float> col[4];
    if (save_prs) {
        std::ofstream f;
        if (!open_output(f, opath + ".mops.stats", dir, err)) return 1;
        f << "TP" << '\t' << "FP" << '\t' << "FDR" << '\t' << "Recall" << '\t' << occ_mult << std::endl;
        for (auto& c : col) c.resize((size_t)std::min(chunk, n_rows));
        for (uint64_t at = 0; at < n_rows; at += chunk) {
            const uint64_t stop = std::min(n_rows, at + chunk);
            if (rows(at, stop, col[0].data(), col[1].data(), col[2].data(), col[3].data(), err)) return 1;
            write_rows(f, (size_t)(stop - at), 6, [&](RowWriter& w, size_t i) {
                w.num(col[0][i]); w.tab(); w.num(col[1][i]); w.tab(); w.num(col[2][i]); w.tab(); w.num(col[3][i]); w.tab(); w.nl();
            });
        }
    }
    if (save_pvalues) {
        std::ofstream f;
        if (!open_output(f, opath + ".mops.pvalues", dir, err)) return 1;
        col[0].resize((size_t)std::min(chunk, n_pvalues));
        for (uint64_t at = 0; at < n_pvalues; at += chunk) {
            const uint64_t stop = std::min(n_pvalues, at + chunk);
            if (pvalues(at, stop, col[0].data(), err)) return 1;
            write_rows(f, (size_t)(stop - at), 3, [&](RowWriter& w, size_t i) { w.num(col[0][i]); w.nl(); });
        }
    }
    return 0;
}

int fdr_write(const std::string& dir, const std::string& basename, const FdrResult& r, size_t posN, size_t negN,
              bool mops, bool zoops, bool save_prs, bool save_pvalues, std::string& err) {
    const std::string opath = dir + '/' + basename;
    if (zoops && save_prs) {                           // FDR.cpp:385-407
        std::ofstream f;
        if (!open_output(f, opath + ".zoops.stats", dir, err)) return 1;
        f << "TP" << '\t' << "FP" << '\t' << "FDR" << '\t' << "Recall" << '\t' << "p-value" << '\t'
          << (float)negN / (float)posN << '\t' << r.occ_frac << std::endl;
        write_rows(f, r.zoops_fdr.size(), 6, [&](RowWriter& w, size_t i) {
            w.num(r.zoops_tp[i]); w.tab(); w.num(r.zoops_fp[i]); w.tab(); w.num(r.zoops_fdr[i]); w.tab();
            w.num(r.zoops_rec[i]); w.tab(); w.num(r.pn_pvalue[i]); w.tab(); w.nl();
        });
    }
    if (zoops && save_pvalues) {                       // FDR.cpp:428-449, setprecision(3)
        std::ofstream f;
        if (!open_output(f, opath + ".zoops.pvalues", dir, err)) return 1;
        write_rows(f, r.zoops_pvalue.size(), 3, [&](RowWriter& w, size_t i) { w.num(r.zoops_pvalue[i]); w.nl(); });
    }
    if (!mops) return 0;
    auto range = [](const std::vector<float>& v, uint64_t begin, uint64_t end, float* dst) { std::copy(v.begin() + (ptrdiff_t)begin, v.begin() + (ptrdiff_t)end, dst); };
    return fdr_write_mops_chunked(dir, basename, r.occ_mult, r.mops_fdr.size(),
        [&](uint64_t a, uint64_t b, float* tp, float* fp, float* fdr, float* rec, std::string&) {
            range(r.mops_tp, a, b, tp); range(r.mops_fp, a, b, fp); range(r.mops_fdr, a, b, fdr); range(r.mops_rec, a, b, rec);
            return 0;
        },
        r.mops_pvalue.size(), [&](uint64_t a, uint64_t b, float* p, std::string&) { range(r.mops_pvalue, a, b, p); return 0; },
        save_prs, save_pvalues, err);
}

// FDR::write, saveLogOdds_ branch (FDR.cpp:416-450): score i of the positives beside score
// i * negN / posN of the negatives.  The reference writes its vectors in whatever order the statistics left
// them: descending after calculatePR (FDR.cpp:158-159,203-204), ascending when calculatePvalues ran as well
// (FDR.cpp:288-289,310-311).  A negative index beyond the list (negN not a multiple of cvFold) ends the file:
// the reference reads past the end there.
int fdr_logodds_write(const std::string& dir, const std::string& basename, std::vector<float> posMax, std::vector<float> negMax,
                      std::vector<float> posAll, std::vector<float> negAll, size_t posN, size_t negN, bool mops, bool zoops,
                      bool ascending, std::string& err) {
    auto emit = [&](const std::string& path, std::vector<float>& pos, std::vector<float>& neg) {
        sort_scores(pos, !ascending);
        sort_scores(neg, !ascending);
        std::ofstream f;
        if (!open_output(f, path, dir, err)) return 1;
        RowWriter w(6);
        w.text("positive\tnegative\n");
        for (size_t i = 0; i < pos.size(); i++) {
            const size_t j = i * negN / posN;
            if (j >= neg.size()) break;
            w.num(pos[i]); w.tab(); w.num(neg[j]); w.nl();
            w.maybe_flush(f);
        }
        w.flush_to(f);
        return 0;
    };
    if (zoops && emit(dir + '/' + basename + ".zoops.logOdds", posMax, negMax)) return 1;
    if (mops && emit(dir + '/' + basename + ".mops.logOdds", posAll, negAll)) return 1;
    return 0;
}

// ScoreSeqSet::writeLogOdds (seq_scoring/ScoreSeqSet.cpp:293-331): the best window of every sequence.
// `revcomp`: the stored sequences carry the reverse strand behind an N (positives unless --ss); the sampled
// negatives never do, although the reference halves their length column too when --ss is absent.
int logodds_zoops_write(const std::string& dir, const std::string& basename, const std::vector<std::string>& headers,
                        const uint8_t* codes, const uint64_t* off, size_t n_seqs, bool revcomp, bool ss, uint32_t W,
                        const float* zoops, const uint64_t* z, std::string& err) {
    WindowRows out{headers, codes, off, W, revcomp, !ss};
    if (!out.open(dir, basename + ".logOddsZoops", "\tzoops_score", err)) return 1;
    for (size_t n = 0; n < n_seqs; n++) out.row(n, z[n], {zoops[n]});
    return out.close();
}

// ScoreSeqSet::write's .occurrence (ScoreSeqSet.cpp:245-291): one row per window with p < cutoff, p- and e-value behind it
int occurrence_write(const std::string& dir, const std::string& basename, const std::vector<std::string>& headers,
                     const uint8_t* codes, const uint64_t* off, size_t n_seqs, bool ss, uint32_t W, const float* p,
                     const float* e, float cutoff, std::string& err) {
    WindowRows out{headers, codes, off, W, !ss, !ss};
    if (!out.open(dir, basename + ".occurrence", "\tp-value\te-value", err)) return 1;
    size_t o = 0;
    for (size_t n = 0; n < n_seqs; n++) {
        const size_t LW1 = out.full_length(n) - W + 1;
        for (size_t i = 0; i < LW1; i++)
            if (p[o + i] < cutoff) out.row(n, i, {p[o + i], e[o + i]});
        o += LW1;
    }
    return out.close();
}

int occurrence_write_hits(const std::string& dir, const std::string& basename, const std::vector<std::string>& headers,
                          const uint8_t* codes, const uint64_t* off, size_t n_seqs, bool ss, uint32_t W, size_t n_hits,
                          const uint64_t* seq, const uint32_t* pos, const float* p, const float* e, std::string& err) {
    WindowRows out{headers, codes, off, W, !ss, !ss};
    if (!out.open(dir, basename + ".occurrence", "\tp-value\te-value", err)) return 1;
    for (size_t h = 0; h < n_hits; h++) {
        if (seq[h] >= n_seqs) { err = "Error: occurrence list names a sequence beyond the set"; return 1; }
        out.row((size_t)seq[h], pos[h], {p[h], e[h]});
    }
    return out.close();
}

// EM::write's .positions (refinement/EM.cpp:577-601): one row per window whose r reaches the cut-off, the window alone
int positions_write(const std::string& dir, const std::string& basename, const std::vector<std::string>& headers,
                    const uint8_t* codes, const uint64_t* off, size_t n_seqs, bool ss, uint32_t W, const float* r, float cutoff,
                    std::string& err) {
    WindowRows out{headers, codes, off, W, !ss, !ss};
    if (!out.open(dir, basename + ".positions", "", err)) return 1;
    size_t ro = 0;
    for (size_t n = 0; n < n_seqs; n++) {
        const size_t L = out.full_length(n);
        for (size_t i = 0; i + W <= L; i++)
            if (r[ro + L - W - i] >= cutoff) out.row(n, i);
        ro += L;
    }
    return out.close();
}

int positions_write_hits(const std::string& dir, const std::string& basename, const std::vector<std::string>& headers,
                         const uint8_t* codes, const uint64_t* off, size_t n_seqs, bool ss, uint32_t W, size_t n_hits,
                         const uint64_t* seq, const uint32_t* pos, std::string& err) {
    WindowRows out{headers, codes, off, W, !ss, !ss};
    if (!out.open(dir, basename + ".positions", "", err)) return 1;
    for (size_t h = 0; h < n_hits; h++) {
        if (seq[h] >= n_seqs || (size_t)pos[h] + W > out.full_length((size_t)seq[h])) { err = "Error: site list names a window beyond the set"; return 1; }
        out.row((size_t)seq[h], pos[h]);
    }
    return out.close();
}

}  // namespace bammhost
