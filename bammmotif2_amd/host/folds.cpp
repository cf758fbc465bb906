// --FDR: the folds of one motif (FDR.cpp:37-127) and the stage that merges them (mainBaMM.cpp:243-265).  Fold f trains on the
// positives {n : n mod cvFold != f} from the SEED model and scores its test positives and every cvFold-th negative on slot
// fold_slot[f]; one host thread per slot in use (the reference runs its folds on OpenMP threads, FDR.cpp:37); every fold
// keeps its scores to itself and they are merged in fold order afterwards, so the files do not depend on the plan or on
// which fold finishes first.
// --mops: the window scores of every fold stay where they are scored and the MOPS statistics are computed there
// (bamm_fdr): one handle per motif and per slot in use.  With several slots each slot's thread seals its handle when
// its folds are done -- the slots sort their scores side by side, beside the other slots' training -- and the runs
// are then absorbed, in ascending slot order, by a handle on fold_slot[0]'s context, which merges them; one slot
// keeps its one handle and sorts in bamm_fdr_statistics.
#include <sstream>

#include "driver.h"

namespace bammhost {
namespace {

// One motif's folds in flight.  Between start and join of the team, slot s's thread alone writes folds[f] of the folds
// planned on s and seal[s], and uses fdr[s]; the caller reads them after the join.
struct FoldTeam {
    const Run& run;
    const NegativeSet& neg;
    const Motif& seed;
    std::vector<FoldOut>& folds;
    std::vector<bamm_fdr*> fdr;            // by slot; null without the device path
    std::vector<double> seal;              // by slot
    bool several = false;                  // more than one slot in use

    void drop_handles() { for (bamm_fdr*& h : fdr) { bamm_fdr_destroy(h); h = nullptr; } }
    void one_fold(size_t fold);
    void slot_thread(size_t slot);
};

void FoldTeam::one_fold(size_t fold) {
    const Options& o = run.o;
    const BgModel& bg = run.bg;
    const size_t cv = o.cvFold, P = run.kept_len.size(), slot = run.plan.fold_slot[fold];
    const Dev& dv = run.devs[slot];
    FoldOut& fo = folds[fold];
    bamm_fdr* const h = fdr[slot];
    Motif m = seed;
    std::vector<uint8_t> train(P, 0), test(P, 0);
    for (size_t i = 0; i + cv <= P; i += cv)                 // strided split; the last P mod cv records are unused
        for (size_t f = 0; f < cv; f++) (f != fold ? train : test)[i + f] = 1;
    if (o.EM) {
        bamm_em_params p = em_params(run, m);
        bamm_em* em = nullptr;
        if (bamm_em_create(dv.ctx, dv.full, &p, bg.v.data(), m.A.data(), m.v.data(), train.data(), &em)) { fo.err = bamm_last_error(); return; }
        uint32_t it = 0;
        const auto t0 = Clock::now();
        int rc;
        if (!o.advanceEM) rc = bamm_em_optimize(em, &it);                                      // FDR.cpp:67-72
        else rc = bamm_em_mask(em, o.f, &it, nullptr, nullptr);
        if (rc) { fo.err = bamm_last_error(); bamm_em_destroy(em); return; }
        bamm_em_get_v(em, m.v.data());
        bamm_em_get_q(em, &fo.q);
        bamm_em_destroy(em);
        std::ostringstream os;
        os << "\n--- Runtime for EM: " << seconds_since(t0) << " seconds ---\n";
        fo.log = os.str();
    }
    std::vector<float> mops, zoops;
    const bool host_mops = o.mops && !h;
    if (score_set(bg, dv.ctx, dv.full, run.kept_len, m, mops, zoops, test.data(), host_mops)) { fo.err = bamm_last_error(); return; }
    if (h && bamm_fdr_add_set(h, 0, dv.full, test.data(), m.K, m.W, bg.K, m.v.data(), bg.v.data())) { fo.err = bamm_last_error(); return; }
    size_t o_m = 0;
    for (size_t i = 0; i < P; i++) {
        const size_t nw = run.kept_len[i] - m.W + 1;
        if (test[i]) {
            if (host_mops) fo.posAll.insert(fo.posAll.end(), mops.begin() + o_m, mops.begin() + o_m + nw);
            if (o.zoops) fo.posMax.push_back(zoops[i]);
        }
        o_m += nw;
    }
    // negSet = every cv-th negative (FDR.cpp:58-60): resident as a set of its own, scored as a whole
    if (score_set(bg, dv.ctx, neg.cv[slot], neg.cv_len, m, mops, zoops, nullptr, host_mops)) { fo.err = bamm_last_error(); return; }
    if (h && bamm_fdr_add_set(h, 1, neg.cv[slot], nullptr, m.K, m.W, bg.K, m.v.data(), bg.v.data())) { fo.err = bamm_last_error(); return; }
    if (host_mops) fo.negAll = mops;
    if (o.zoops) fo.negMax = zoops;
}

void FoldTeam::slot_thread(size_t slot) {
    const size_t cv = folds.size();
    size_t last = cv;
    for (size_t f = 0; f < cv; f++) if (run.plan.fold_slot[f] == slot) { one_fold(f); last = f; }
    if (!several || !fdr[slot] || last == cv || !folds[last].err.empty()) return;
    const auto t0 = Clock::now();
    if (bamm_fdr_seal(fdr[slot])) folds[last].err = bamm_last_error();
    seal[slot] = seconds_since(t0);
}

// several slots: their sealed handles are absorbed in ascending slot order by one on fold_slot[0]'s context, which merges
// them; the handle, or null with the message in folds[0].err
bamm_fdr* absorb_slots(FoldTeam& team, const std::vector<size_t>& slots_in_use, FdrPlanTimes& ft) {
    ft.seal = *std::max_element(team.seal.begin(), team.seal.end());
    bamm_ctx* const owner_ctx = team.run.devs[team.run.plan.fold_slot[0]].ctx;
    bamm_fdr* owner = nullptr;
    auto t0 = Clock::now();
    bool ok = bamm_fdr_create(owner_ctx, &owner) == 0;
    for (size_t slot : slots_in_use) {
        uint64_t n_pos = 0;
        if (!ok) break;
        bamm_fdr_info(team.fdr[slot], &n_pos, nullptr, nullptr, nullptr, nullptr);
        ft.runs += n_pos ? 1 : 0;                            // runs of the positive list
        ok = bamm_fdr_absorb(owner, team.fdr[slot]) == 0;
    }
    ok = ok && bamm_ctx_sync(owner_ctx) == 0;
    ft.absorb = seconds_since(t0);
    t0 = Clock::now();
    ok = ok && bamm_fdr_seal(owner) == 0;                    // the merge: each list one run, bamm_fdr_statistics finds nothing left to sort
    ft.merge = seconds_since(t0);
    if (!ok) { team.folds[0].err = bamm_last_error(); bamm_fdr_destroy(owner); owner = nullptr; }
    return owner;
}

// the MOPS half where the scores are: rows and p-values arrive chunk by chunk
void write_device_mops(Run& run, bamm_fdr* fdr, const FdrPlanTimes& ft, const std::string& fbase) {
    const Options& o = run.o;
    std::string err;
    uint64_t n_pos = 0, n_neg = 0, n_rows = 0;
    float occ_mult = 0.f;
    if (bamm_fdr_statistics(fdr, run.kept_len.size(), run.negN, o.savePvalues ? 1 : 0) || bamm_fdr_info(fdr, &n_pos, &n_neg, &n_rows, nullptr, &occ_mult)) die_abi("MOPS statistics");
    auto rows = [&](uint64_t b, uint64_t e, float* tp, float* fp, float* fd, float* rec, std::string& msg) {
        if (bamm_fdr_rows(fdr, b, e, tp, fp, fd, rec)) { msg = std::string("Error: MOPS statistics: ") + bamm_last_error(); return 1; }
        return 0;
    };
    auto pvals = [&](uint64_t b, uint64_t e, float* p, std::string& msg) {
        if (bamm_fdr_pvalues(fdr, b, e, p)) { msg = std::string("Error: MOPS p-values: ") + bamm_last_error(); return 1; }
        return 0;
    };
    if (fdr_write_mops_chunked(o.out_dir, fbase, occ_mult, n_rows, rows, n_pos, pvals, o.savePRs, o.savePvalues, err)) die(err);
    bamm_fdr_destroy(fdr);
    if (o.timing) std::cerr << "[timing-beside] MOPS window scores: device, " << ft.runs << " runs from " << ft.slots << " slots: seal "
                            << ft.seal << " s (the slowest slot, beside the other slots' folds), absorb " << ft.absorb
                            << " s, merge " << ft.merge << " s" << std::endl;
    if (o.timing) std::cerr << "[timing-beside] MOPS statistics on the device: " << n_pos << " + " << n_neg << " window scores, " << n_rows << " rows, "
                            << (o.savePRs ? n_rows * 16 : 0) + (o.savePvalues ? n_pos * 4 : 0) + 16
                            << " bytes downloaded (computed: 16 per row written, 4 per p-value written, the 16-byte peak)" << std::endl;
}

}  // namespace

Folds::Folds(const Run& run_, const NegativeSet& neg_)
    : run(run_), neg(neg_), device_fdr(run_.o.need_gpu() && run_.o.FDR && run_.o.mops && !run_.o.hostFdr && !run_.o.saveLogOdds),
      results(run_.seeds.motifs.size()), handles(run_.seeds.motifs.size(), nullptr), times(run_.seeds.motifs.size()) {}

void Folds::start(size_t n) { g_threads.folds = std::thread(&Folds::run_motif, this, n); }

void Folds::run_motif(size_t n) {
    const size_t cv = run.o.cvFold;
    std::vector<FoldOut>& folds = results[n];
    folds.assign(cv, FoldOut());
    for (auto& f : folds) f.q = run.seeds.motifs[n].q;
    std::vector<size_t> slots_in_use(run.plan.fold_slot.begin(), run.plan.fold_slot.begin() + cv);
    std::sort(slots_in_use.begin(), slots_in_use.end());
    slots_in_use.erase(std::unique(slots_in_use.begin(), slots_in_use.end()), slots_in_use.end());
    FoldTeam team{run, neg, run.seeds.motifs[n], folds, std::vector<bamm_fdr*>(run.devs.size(), nullptr), std::vector<double>(run.devs.size(), 0.0), slots_in_use.size() > 1};
    if (device_fdr)
        for (size_t slot : slots_in_use)
            if (bamm_fdr_create(run.devs[slot].ctx, &team.fdr[slot])) { folds[0].err = bamm_last_error(); team.drop_handles(); return; }
    std::vector<std::thread> threads;
    for (size_t slot : slots_in_use) threads.emplace_back(&FoldTeam::slot_thread, &team, slot);
    for (auto& t : threads) t.join();
    if (!device_fdr) return;
    FdrPlanTimes& ft = times[n];
    ft.slots = slots_in_use.size();
    if (!team.several) { handles[n] = team.fdr[slots_in_use[0]]; ft.runs = 1; return; }
    for (const FoldOut& fo : folds) if (!fo.err.empty()) { team.drop_handles(); return; }
    handles[n] = absorb_slots(team, slots_in_use, ft);
    team.drop_handles();
}

void fdr_stage(Run& run, Folds& fl) {
    const Options& o = run.o;
    std::string err;
    if (o.verbose) std::cout << std::endl << "***********************" << std::endl << "*   BaMM validation   *" << std::endl << "***********************" << std::endl;
    const size_t cv = o.cvFold, P = run.kept_len.size(), negN = run.negN;
    for (size_t n = 0; n < run.seeds.motifs.size(); n++) {
        // the folds of this motif: trained while the main run was training (overlap mode), else here
        if (fl.results[n].empty()) fl.run_motif(n);
        std::vector<float> posMax, negMax, posAll, negAll;
        float updatedQ = run.seeds.motifs[n].q;
        for (size_t fold = 0; fold < cv; fold++) {            // merge in fold order
            const FoldOut& fo = fl.results[n][fold];
            if (!fo.err.empty()) die("Error: fold " + std::to_string(fold) + ": " + fo.err);
            std::cout << fo.log;
            posMax.insert(posMax.end(), fo.posMax.begin(), fo.posMax.end());
            negMax.insert(negMax.end(), fo.negMax.begin(), fo.negMax.end());
            posAll.insert(posAll.end(), fo.posAll.begin(), fo.posAll.end());
            negAll.insert(negAll.end(), fo.negAll.begin(), fo.negAll.end());
            if (o.EM) updatedQ = fo.q;                        // the reference keeps whichever fold wrote last (FDR.cpp:73): the last one here
        }
        run.stage("--FDR: fold EMs + scoring (GPU)");
        const std::string fbase = o.basename + "_motif_" + std::to_string(n + 1);
        if (o.saveLogOdds && fdr_logodds_write(o.out_dir, fbase, posMax, negMax, posAll, negAll, P, negN, o.mops, o.zoops,
                                               o.savePvalues, err)) die(err);
        FdrResult res;
        bamm_fdr* const fdr = fl.handles[n];
        const bool host_mops = o.mops && !fdr;
        fdr_statistics(posMax, negMax, posAll, negAll, P, negN, updatedQ, host_mops, o.zoops, o.savePvalues, res);
        if (fdr_write(o.out_dir, fbase, res, P, negN, host_mops, o.zoops, o.savePRs, o.savePvalues, err)) die(err);
        if (fdr) {
            write_device_mops(run, fdr, fl.times[n], fbase);
            fl.handles[n] = nullptr;
        } else if (o.timing && o.mops) {
            std::cerr << "[timing-beside] MOPS window scores: host (every fold's scores downloaded, sorted and walked there)" << std::endl;
        }
        run.stage("--FDR: PR / p-value statistics + writers (host)");
    }
}

}  // namespace bammhost
