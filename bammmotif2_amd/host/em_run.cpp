// The main EM run of one motif (mainBaMM.cpp:131-147, EM.cpp): one handle per GPU of the plan's group over its shard, a host
// thread per rank, the read-back, EM.cpp's trace lines, and EM::write's .counts / .positions.
#include <fstream>

#include "driver.h"

namespace bammhost {

bamm_em_params em_params(const Run& run, const Motif& m) {
    bamm_em_params p;
    bamm_em_default_params(&p);
    p.K = m.K; p.W = m.W; p.bg_order = run.bg.K; p.q = m.q; p.optimize_q = run.o.optimizeQ;
    p.epsilon = run.o.epsilon; p.max_iterations = run.o.max_iter;
    p.n_seqs_bound = run.posN;                               // one unit for the count accumulator on every GPU
    return p;
}

namespace {

// By slot.  The main thread creates and destroys the handles; between start and join of the ranks, rank d's thread alone
// drives ems[d] and writes its[d] and err[d] (the ABI's message is thread-local: taken where the call failed).
struct EmRun {
    std::vector<bamm_em*> ems;
    std::vector<std::string> err;
    std::vector<uint32_t> its;
};

// a rank that fails aborts every communicator before it returns, so that its peers return
void run_rank(const Run& run, EmRun& er, size_t d) {
    int rc;
    if (!run.o.advanceEM) rc = bamm_em_optimize(er.ems[d], &er.its[d]);                        // mainBaMM.cpp:133-137
    else rc = bamm_em_mask(er.ems[d], run.o.f, &er.its[d], nullptr, nullptr);
    if (rc) {
        er.err[d] = bamm_last_error();
        for (const Dev& dv : run.devs) if (dv.comm) bamm_comm_abort(dv.comm);
    }
}

// one std::thread per rank, not an OpenMP team (which may come back smaller than asked for and leave ranks out of the
// collective); every pass ends in one all-reduce, after which all ranks hold the same model
void run_ranks(const Run& run, EmRun& er) {
    if (run.plan.sharded) {
        std::vector<std::thread> team;
        for (size_t d = 0; d < run.plan.em_slots.size(); d++) if (er.ems[d]) team.emplace_back(run_rank, std::cref(run), std::ref(er), d);
        for (auto& t : team) t.join();
    } else if (er.ems[0]) {
        run_rank(run, er, 0);
    }
    for (size_t d = 0; d < run.devs.size(); d++)
        if (!er.err[d].empty()) die("Error: EM on GPU " + std::to_string(run.devs[d].device) + ": " + er.err[d]);
}

void print_trace(const Options& o, bamm_em* em, uint32_t it) {   // the lines EM.cpp:112-115 prints
    std::vector<float> llh(it), vd(it), qq(it);
    uint32_t cnt = 0;
    bamm_em_get_trace(em, llh.data(), vd.data(), qq.data(), it, &cnt);
    for (uint32_t i = 0; i < cnt && i < it; i++) {
        if (o.advanceEM) {                                    // EM.cpp:487
            std::cout << i + 1 << "th iteration, delta_llikelihood=" << llh[i] - (i ? llh[i - 1] : 0.f) << std::endl;
            continue;
        }
        if (o.optimizeQ && i < 5) std::cout << "optimized q=" << qq[i] << std::endl;
        std::cout << i + 1 << " iter, llh=" << llh[i] << ", diff_llh=" << llh[i] - (i ? llh[i - 1] : 0.f)
                  << ", v_diff=" << vd[i] << std::endl;
    }
}

void write_counts(const Options& o, bamm_em* em, const Motif& motif, const std::string& mbase) {   // EM::write (EM.cpp:553-601)
    std::vector<float> cnts(bamm_v_size(motif.K, motif.W));
    bamm_em_get_counts(em, cnts.data());
    std::ofstream fn(o.out_dir + '/' + mbase + ".counts");
    for (uint32_t j = 0; j < motif.W; j++) {
        for (uint32_t k = 0; k <= motif.K; k++) {
            for (size_t y = 0; y < (size_t(1) << (2 * (k + 1))); y++)
                fn << static_cast<int>(cnts[bamm_v_offset(k, motif.W) + y * motif.W + j]) << '\t';
            fn << std::endl;
        }
        fn << std::endl;
    }
}

// --hostPositions: r of every kept sequence on the host, shard after shard (the shards are consecutive ranges), scanned there
void write_positions_dense(const Run& run, const EmRun& er, uint32_t W, const std::string& mbase) {
    std::string err;
    uint64_t total = 0;
    for (uint32_t L : run.kept_len) total += L;
    std::vector<float> r(total ? total : 1);
    uint64_t ro_base = 0;
    for (size_t d = 0; d < run.devs.size(); d++) {
        if (!er.ems[d]) continue;
        uint64_t ns = 0, tl = 0;
        bamm_seqs_info(run.devs[d].shard, &ns, &tl, nullptr, nullptr);
        if (tl && bamm_em_get_r(er.ems[d], 0, ns, r.data() + ro_base, tl)) die_abi("getR");
        ro_base += tl;
    }
    if (positions_write(run.o.out_dir, mbase, run.kept_headers(), run.kept_codes(), run.kept_off(), run.kept_len.size(), run.o.ss, W,
                        r.data(), 0.3f, err)) die(err);
    if (run.o.timing) std::cerr << "[timing-beside] .positions: dense r, " << total * sizeof(float) << " bytes of r (computed: 4 per position)" << std::endl;
}

// the windows with r >= 0.3 are found where r is (bamm_em_sites); a few rows per sequence cross
void write_positions_sites(const Run& run, const EmRun& er, uint32_t W, const std::string& mbase) {
    std::string err;
    std::vector<uint64_t> hit_seq;
    std::vector<uint32_t> hit_pos;
    uint64_t seq_base = 0;
    for (size_t d = 0; d < run.devs.size(); d++) {
        if (!er.ems[d]) continue;
        uint64_t ns = 0, n_sites = 0;
        bamm_seqs_info(run.devs[d].shard, &ns, nullptr, nullptr, nullptr);
        bamm_sites* sites = nullptr;
        if (bamm_em_sites(er.ems[d], 0, ns, 0.3f, &sites) || bamm_sites_info(sites, &n_sites, nullptr)) die_abi("sites");
        const size_t at = hit_seq.size();
        hit_seq.resize(at + n_sites);
        hit_pos.resize(at + n_sites);
        if (n_sites && bamm_sites_get(sites, hit_seq.data() + at, hit_pos.data() + at, nullptr, n_sites)) die_abi("sites");
        bamm_sites_destroy(sites);
        for (size_t h = at; h < hit_seq.size(); h++) hit_seq[h] += seq_base;
        seq_base += ns;
    }
    if (positions_write_hits(run.o.out_dir, mbase, run.kept_headers(), run.kept_codes(), run.kept_off(), run.kept_len.size(), run.o.ss, W,
                             hit_seq.size(), hit_seq.data(), hit_pos.data(), err)) die(err);
    if (run.o.timing) std::cerr << "[timing-beside] .positions: " << hit_seq.size() << " sites, " << hit_seq.size() * 12 + run.kept_len.size() * 12
                                << " bytes of records and per-sequence arrays (computed: 12 per site + 12 per sequence; the call also reads 8 bytes per chunk)" << std::endl;
}

}  // namespace

void train_motif(Run& run, size_t n, Motif& motif, const std::string& mbase) {
    const Options& o = run.o;
    const size_t ndev = run.devs.size();
    const auto t0 = Clock::now();
    const bamm_em_params p = em_params(run, motif);
    EmRun er{std::vector<bamm_em*>(ndev, nullptr), std::vector<std::string>(ndev), std::vector<uint32_t>(ndev, 0)};
    for (size_t d = 0; d < run.plan.em_slots.size(); d++) {
        if (d > 0 && !run.plan.sharded) break;
        const Dev& dv = run.devs[d];
        if (bamm_em_create(dv.ctx, dv.shard, &p, run.bg.v.data(), motif.A.data(), motif.v.data(), nullptr, &er.ems[d])) die_abi("EM");
        if (dv.comm && bamm_em_set_comm(er.ems[d], dv.comm)) die_abi("EM communicator");
    }
    const auto t_created = Clock::now();
    run_ranks(run, er);
    bamm_em* em = er.ems[0];
    const uint32_t it = er.its[0];
    const auto t_optimized = Clock::now();
    if (bamm_em_get_v(em, motif.v.data())) die_abi("get_v");
    float q = 0;
    bamm_em_get_q(em, &q);
    motif.q = q;
    if (o.verbose) print_trace(o, em, it);
    motif_calculate_p(motif, run.bg);
    const auto t_done = Clock::now();
    std::cout << "\n--- Runtime for EM: " << seconds_between(t0, t_done) << " seconds ---\n";        // EM.cpp:134
    if (o.timing) std::cerr << "[timing-beside] EM of motif " << n + 1 << ": create " << seconds_between(t0, t_created)
                            << " s, " << (o.advanceEM ? "mask" : "optimize") << " " << seconds_between(t_created, t_optimized)
                            << " s (" << it << " passes), read-back + calculateP " << seconds_between(t_optimized, t_done) << " s" << std::endl;
    run.stage("EM (create + optimize + read-back)");
    if (o.saveBaMMs) {
        write_counts(o, em, motif, mbase);
        if (o.hostPositions) write_positions_dense(run, er, motif.W, mbase);
        else write_positions_sites(run, er, motif.W, mbase);
    }
    std::cout << "optimized q = " << q << std::endl;         // mainBaMM.cpp:147
    for (bamm_em* e : er.ems) bamm_em_destroy(e);
}

}  // namespace bammhost
