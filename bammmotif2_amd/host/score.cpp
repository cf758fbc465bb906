// --scoreSeqset (mainBaMM.cpp:171-236, ScoreSeqSet.cpp): window p-values against the negative set and the .occurrence file of
// one motif, on slot 0; and the scorer over a resident set that the folds of --FDR use as well.
#include "driver.h"

namespace bammhost {

int score_set(const BgModel& bg, bamm_ctx* ctx, bamm_seqs* set, const std::vector<uint32_t>& lens, const Motif& m, std::vector<float>& mops,
              std::vector<float>& zoops, const uint8_t* subset, bool want_mops, std::vector<uint64_t>* z_out) {
    size_t total = 0;
    if (want_mops) for (uint32_t L : lens) total += L - m.W + 1;
    mops.assign(total ? total : 1, 0.f);
    zoops.assign(lens.size() ? lens.size() : 1, 0.f);
    std::vector<uint64_t> z_local;
    std::vector<uint64_t>& z = z_out ? *z_out : z_local;
    z.assign(lens.size() ? lens.size() : 1, 0);
    if (bamm_logodds_subset(ctx, set, subset, m.K, m.W, bg.K, m.v.data(), bg.v.data(), want_mops ? mops.data() : nullptr, total,
                            zoops.data(), z.data())) return 1;
    mops.resize(total);
    zoops.resize(lens.size());
    return 0;
}

void score_seqset(Run& run, const NegativeSet& neg, const Motif& sm, const std::string& mbase) {
    const Options& o = run.o;
    const BgModel& bg = run.bg;
    const Dev& dv = run.devs[0];
    const size_t P = run.kept_len.size();
    std::string err;
    if (o.verbose) std::cout << std::endl << "*************************" << std::endl << "*    Score Sequences    *" << std::endl << "*************************" << std::endl << std::endl;
    if (!o.EM && o.seed_tag == "BaMM" && o.bg_file.empty()) die("No background Model file provided for initial search motif!");
    std::vector<float> neg_mops, neg_zoops, pos_mops, pos_zoops, pv, ev;
    std::vector<uint64_t> neg_z, pos_z;
    // --hostPvalues: every window's score comes to the host, which sorts, ranks and walks them; the default leaves
    // them on the device (bamm_occurrences) and asks the scorer for the per-sequence maxima of --saveLogOdds only
    const bool want_mops = o.hostPvalues;
    if (want_mops || o.saveLogOdds) {
        if (score_set(bg, dv.ctx, neg.all, neg.len, sm, neg_mops, neg_zoops, nullptr, want_mops, &neg_z)) die_abi("calcLogOdds");
        if (score_set(bg, dv.ctx, dv.full, run.kept_len, sm, pos_mops, pos_zoops, nullptr, want_mops, &pos_z)) die_abi("calcLogOdds");
    }
    if (o.saveLogOdds) {                                     // mainBaMM.cpp:204-208, :223-227
        const std::vector<std::string> neg_headers(run.negN, "> bg_seq");                     // SeqGenerator.cpp:228
        if (logodds_zoops_write(o.out_dir, o.basename + ".negSet", neg_headers, neg.codes.data(), neg.off.data(), run.negN, false,
                                o.ss, sm.W, neg_zoops.data(), neg_z.data(), err)) die(err);
        if (logodds_zoops_write(o.out_dir, mbase, run.kept_headers(), run.kept_codes(), run.kept_off(), P, !o.ss,
                                o.ss, sm.W, pos_zoops.data(), pos_z.data(), err)) die(err);
    }
    if (o.hostPvalues) {
        mops_pvalues(pos_mops.data(), pos_mops.size(), neg_mops, P, pv, ev);
        if (occurrence_write(o.out_dir, mbase, run.kept_headers(), run.kept_codes(), run.kept_off(), P, o.ss, sm.W,
                             pv.data(), ev.data(), o.pvalCutoff, err)) die(err);
    } else {
        bamm_occ* occ = nullptr;
        if (bamm_occurrences(dv.ctx, dv.full, neg.all, sm.K, sm.W, bg.K, sm.v.data(), bg.v.data(), o.pvalCutoff, &occ)) die_abi("calcPvalues");
        uint64_t n_hits = 0;
        bamm_occ_info(occ, &n_hits, nullptr, nullptr, nullptr, nullptr, nullptr);
        std::vector<uint64_t> hit_seq(n_hits ? n_hits : 1);
        std::vector<uint32_t> hit_pos(hit_seq.size());
        pv.assign(hit_seq.size(), 0.f);
        ev.assign(hit_seq.size(), 0.f);
        if (bamm_occ_get(occ, hit_seq.data(), hit_pos.data(), nullptr, nullptr, pv.data(), ev.data(), hit_seq.size())) die_abi("calcPvalues");
        bamm_occ_destroy(occ);
        if (occurrence_write_hits(o.out_dir, mbase, run.kept_headers(), run.kept_codes(), run.kept_off(), P, o.ss, sm.W,
                                  n_hits, hit_seq.data(), hit_pos.data(), pv.data(), ev.data(), err)) die(err);
    }
    run.stage("--scoreSeqset: score + p-values + .occurrence");
}

}  // namespace bammhost
