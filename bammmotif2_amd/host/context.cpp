// The run context of the BaMMmotif driver: the side threads and die(), the stage clock, the HIP warm-up, and prepare(),
// which builds what every later stage reads -- positives, background model, seeds, slot plan, the resident sets.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>

#include "driver.h"

namespace bammhost {

SideThreads g_threads;

[[noreturn]] void die(const std::string& msg) {
    std::cerr << msg << std::endl;
    for (std::thread* t : {&g_threads.hip_warmup, &g_threads.negatives, &g_threads.folds})
        if (t->joinable() && t->get_id() != std::this_thread::get_id()) t->join();
    exit(1);
}

[[noreturn]] void die_abi(const char* what) { die(std::string("Error: ") + what + ": " + bamm_last_error()); }

double epoch_seconds() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }

void Run::stage(const char* what) {
    if (!o.timing) return;
    const auto now = Clock::now();
    std::cerr << "[timing] " << what << ": " << seconds_between(t_stage, now) << " s" << std::endl;
    t_stage = now;
}

void WarmUp::start(int device_) {
    device = device_;
    g_threads.hip_warmup = std::thread(&WarmUp::body, this);
}

void WarmUp::body() {
    int n = 0;
    if (bamm_device_count(&n) == BAMM_OK && bamm_ctx_create(device, nullptr, &ctx) != BAMM_OK) ctx = nullptr;
}

bamm_ctx* WarmUp::take(int device_) {
    if (g_threads.hip_warmup.joinable()) g_threads.hip_warmup.join();
    bamm_ctx* c = nullptr;
    if (ctx && device_ == device) std::swap(c, ctx);
    return c;
}

namespace {

// The shape classes of profiles/score_slices_ab.txt in which the slices won (the call that downloads zoops and z, which is
// what this driver's scoring calls do; with the download of every window's score on top no class lost, tiny sets apart):
//   - a record beyond the length classes, whatever the set (h: 300 x 205 bp + one of 20 kb, 5.6x; e: 16 x 4 M, 204x): the
//     window-by-window scorer gives such a record to one workgroup
//   - sets from 30 000 x 205 bp on (g: 1.8x; a: 200 000 x 200 bp, 3.3x; b: K = 4, W = 40, 5.7x).  At 3 000 x 205 bp (f) the
//     two are level, at 300 x 205 bp (d, the size of the JunD example) two or three launches cost 0.07 ms more than one: the
//     threshold is g's size, the smallest measured set that wins
//   - up to order 5.  At order 6 (c: 50 000 x 200 bp, six slices of two columns) the slices' median was 1.4x ahead but
//     inside the parent's spread of that run: not shown, so order 6 keeps the window-by-window scorer
bool score_slices_pay(const Options& o, const FastaSet& pos) {
    constexpr size_t kMinBases = 30000u * 205u;
    const size_t longest = o.ss ? pos.max_len : 2 * pos.max_len + 1;
    return o.K <= 5 && (longest > BAMM_MAX_SEQ_POSITIONS || pos.codes.size() >= kMinBases);
}

}  // namespace

void Run::make_ctx(Dev& dv) {
    if (!dv.ctx) dv.ctx = warm.take(dv.device);             // the one the warm-up made
    if (!dv.ctx && bamm_ctx_create(dv.device, nullptr, &dv.ctx)) die_abi("no usable MI355X");
    // BAMM_NO_SCORE_TILES=1: long records window by window, as before the tiles -- for comparing this program with itself
    // (the library reads no environment: the driver turns the variable into the tuning key)
    if (const char* e = std::getenv("BAMM_NO_SCORE_TILES"); e && *e && *e != '0')
        if (bamm_ctx_set_tuning(dv.ctx, "score_tiles", 0)) die_abi("score_tiles");
    // log-odds tables beyond one CU's LDS (K = 4 from W = 40, K = 5 from W = 10, K = 6 from W = 3) a slice of columns per launch
    // through the register-resident scorer: off in the library by default, on here where profiles/score_slices_ab.txt shows
    // the slices ahead of the window-by-window scorer by more than that scorer's own spread; BAMM_NO_SCORE_SLICES=1 keeps the
    // window-by-window scorer everywhere, the same bytes in every output file
    const char* e = std::getenv("BAMM_NO_SCORE_SLICES");
    if (bamm_ctx_set_tuning(dv.ctx, "score_slices", !(e && *e && *e != '0') && score_slices_pay(o, pos) ? 1 : 0)) die_abi("score_slices");
}

namespace {

// prepare()'s steps hand each other: `off` [n+1], the positions of every positive record as packed; `keep`, whether a record
// is at least as long as the widest motif; `dseqs_all`, every positive record resident (packing, seeding, then EM)
void read_and_pack(Run& run, std::vector<uint64_t>& off, bamm_seqs*& dseqs_all) {
    const Options& o = run.o;
    FastaSet& pos = run.pos;
    std::string err;
    if (read_fasta(o.fasta, pos, err)) die(err);
    if (pos.size() < o.cvFold) die("Error: Input sequences are too few for training! \n");
    run.stage("read FASTA");
    run.devs.resize(o.need_gpu() ? o.device_list.size() : 1);
    for (size_t d = 0; d < run.devs.size(); d++) run.devs[d].device = o.device_list[d];
    // the stream stands at srand(42) (main(); nothing between draws from it): the N draws are taken on all host threads
    // (--seedKmers packs on the host: the w-mer counter needs to know where the unknown bases were, which a packed set
    // notes when bamm_pack_codes* makes it; bamm_seqs_from_codes does not)
    if (o.need_gpu() && !o.hostPacking && !o.seedKmers) {
        // Sequence::Sequence where the data will live (csrc/prep.hip): the same packed set, and the resident set with it
        run.make_ctx(run.devs[0]);
        if (bamm_seqs_from_codes(run.devs[0].ctx, pos.codes.data(), pos.off.data(), pos.size(), o.ss ? 1 : 0, 42u, &run.packed, &dseqs_all)) die_abi("packing sequences");
        run.stage("encode + 2-bit pack on the device, resident set (Sequence.cpp incl. rand() protocol)");
    } else {
        if (bamm_pack_codes_seeded(pos.codes.data(), pos.off.data(), pos.size(), o.ss ? 1 : 0, 42u, &run.packed)) die_abi("packing sequences");
        run.stage("encode + 2-bit pack (Sequence.cpp incl. rand() protocol)");
    }
    // (records beyond 8192 positions leave the register-resident kernels for the window-by-window path, csrc/long_seq.hip;
    // initFromPWM's pass and EM::mask keep their per-wave arrays in a global scratch region there: no limit on the length)
    off.assign(pos.size() + 1, 0);
    for (size_t n = 0; n < pos.size(); n++) off[n + 1] = off[n] + run.packed->len[n];
}

void background_model(Run& run, bamm_seqs* dseqs_all) {
    const Options& o = run.o;
    BgModel& bg = run.bg;
    std::string err;
    if (o.bg_file.empty()) {
        if (dseqs_all) {                                     // the counting pass over the resident set (BackgroundModel.cpp:26-42)
            bg.K = o.Kbg; bg.alpha = o.alpha_bg; bg.v.assign(bamm_bg_size(o.Kbg), 0.f);
            if (bamm_seqs_bg_model(run.devs[0].ctx, dseqs_all, o.Kbg, o.alpha_bg.data(), bg.v.data())) die_abi("background model");
        } else if (bg_learn(run.packed, o.Kbg, o.alpha_bg, bg)) die_abi("background model");
    } else if (bg_read(o.bg_file, bg, err)) {
        die(err);
    }
    if (bg_write(o.out_dir, o.basename, bg, err)) die(err);   // always saved (mainBaMM.cpp:51)
    run.stage("background model");
}

// --seedGaps: the same with the dyad tables of every gap asked for beside the contiguous one (one launch on the device), ranked
// together: a seed's PWM spans its gap, and the seed file carries it at that width.
void dyad_seed_file(Run& run, bamm_seqs*& dseqs_all) {
    const Options& o = run.o;
    const uint32_t w = o.seedKmers, lo = o.seedGapLo, hi = o.seedGapHi;
    const std::string gaps = "gaps " + std::to_string(lo) + ".." + std::to_string(hi);
    std::vector<uint64_t> counts((size_t(1) << (2 * w)) * (hi - lo + 1)), n_windows(hi - lo + 1, 0);
    if (o.need_gpu() && !o.hostSeedCounts) {
        run.make_ctx(run.devs[0]);
        if (!dseqs_all && bamm_seqs_upload(run.devs[0].ctx, run.packed, 0, run.packed->n_seqs, &dseqs_all)) die_abi("upload");
        if (bamm_kmer_counts_gapped(run.devs[0].ctx, dseqs_all, w, lo, hi, counts.data(), n_windows.data())) die_abi("dyad counts");
        run.stage(("dyad counts on the device (--seedKmers --seedGaps, " + gaps + ")").c_str());
    } else {
        if (bamm_kmer_counts_gapped_host(run.pos.codes.data(), run.pos.off.data(), run.pos.size(), o.ss ? 1 : 0, w, lo, hi, counts.data(), n_windows.data())) die_abi("dyad counts");
        run.stage(("dyad counts on the host (--seedKmers --seedGaps, " + gaps + ")").c_str());
    }
    std::vector<KmerSeed> seeds;
    std::string err;
    kmer_seeds_gapped(counts.data(), n_windows.data(), w, lo, hi, run.bg, o.maxPWM, o.ss, seeds);
    if (seeds.empty()) die("Error: --seedKmers found no " + std::to_string(w) + "-mer with " + gaps + " that is more frequent than the background model expects.");
    if (kmer_seeds_write(o.seed_file, w, seeds, err)) die(err);
    if (o.verbose)
        for (const KmerSeed& s : seeds) std::cout << "seed " << kmer_string(s.kmer, w, s.gap) << "  count " << s.count << "  z " << s.z << std::endl;
    run.stage(("rank dyads (" + gaps + "), write the seed file").c_str());
}

// --seedKmers: the exact w-mer table of the positives (on the device over the resident set, or with --hostSeedCounts / without
// a GPU stage on the host threads: the same integers), ranked against the background model (seeder.cpp), written as
// OUTDIR/<basename>_seeds.meme.  seed_models() then reads that file like any --PWMFile: there is no second seeding path.
void kmer_seed_file(Run& run, bamm_seqs*& dseqs_all) {
    const Options& o = run.o;
    const uint32_t w = o.seedKmers;
    if (o.seedGaps) return dyad_seed_file(run, dseqs_all);
    std::vector<uint64_t> counts(size_t(1) << (2 * w));
    uint64_t n_windows = 0;
    if (o.need_gpu() && !o.hostSeedCounts) {
        run.make_ctx(run.devs[0]);
        if (!dseqs_all && bamm_seqs_upload(run.devs[0].ctx, run.packed, 0, run.packed->n_seqs, &dseqs_all)) die_abi("upload");
        if (bamm_kmer_counts(run.devs[0].ctx, dseqs_all, w, counts.data(), &n_windows)) die_abi("w-mer counts");
        run.stage("w-mer counts on the device (--seedKmers)");
    } else {
        if (bamm_kmer_counts_host(run.pos.codes.data(), run.pos.off.data(), run.pos.size(), o.ss ? 1 : 0, w, counts.data(), &n_windows)) die_abi("w-mer counts");
        run.stage("w-mer counts on the host (--seedKmers)");
    }
    std::vector<KmerSeed> seeds;
    std::string err;
    kmer_seeds(counts.data(), n_windows, w, run.bg, o.maxPWM, o.ss, seeds);
    if (seeds.empty()) die("Error: --seedKmers found no " + std::to_string(w) + "-mer that is more frequent than the background model expects.");
    if (kmer_seeds_write(o.seed_file, w, seeds, err)) die(err);
    if (o.verbose)
        for (const KmerSeed& s : seeds) std::cout << "seed " << kmer_string(s.kmer, w) << "  count " << s.count << "  z " << s.z << std::endl;
    run.stage("rank w-mers, write the seed file");
}

void seed_models(Run& run, const std::vector<uint64_t>& off, bamm_seqs*& dseqs_all, std::vector<uint8_t>& keep) {
    const Options& o = run.o;
    const bamm_packed* packed = run.packed;
    const size_t N = run.pos.size();
    std::string err;
    if (o.seedKmers) kmer_seed_file(run, dseqs_all);
    SeedDevice seed_dev;
    std::vector<uint32_t> yK;
    if (o.need_gpu() && o.seed_tag == "PWM" && !o.hostSeeding) {
        // Motif::initFromPWM's pass over the sequences runs on the device: upload first
        run.make_ctx(run.devs[0]);
        if (!dseqs_all && bamm_seqs_upload(run.devs[0].ctx, packed, 0, packed->n_seqs, &dseqs_all)) die_abi("upload");
        seed_dev.ctx = run.devs[0].ctx; seed_dev.seqs = dseqs_all;
        run.stage("device context + upload of the positives");
    } else if (o.seed_tag == "PWM") {
        yK.resize(packed->total_len ? packed->total_len : 1);
        if (bamm_unpack_y(packed, o.K, yK.data())) die_abi("unpack");
    }
    // MotifSet hands Global::bgModelOrder and the model's v to every Motif (mainBaMM.cpp:60-70)
    if (load_seeds(o.seed_file, o.seed_tag, (uint32_t)o.extend[0], (uint32_t)o.extend[1], o.K, o.alpha, o.maxPWM, o.q, run.bg,
                   yK.empty() ? nullptr : yK.data(), off.data(), N, run.seeds, err, seed_dev.ctx ? &seed_dev : nullptr)) die(err);
    run.stage("seed models (initFromPWM / BaMM / sites)");

    // drop sequences shorter than the widest motif (mainBaMM.cpp:75-83)
    keep.assign(N, 1);
    for (size_t n = 0; n < N; n++) { keep[n] = packed->len[n] >= run.seeds.max_w; run.posN += keep[n]; }
    if (run.posN < o.cvFold) { std::cerr << "There are " << run.posN << " sequences longer than input motif. Exit!\n"; exit(1); }
}

// contexts of all slots, then the kept positives where the plan wants them: the full set where sequences are scored
// (slot 0) or folds are trained, a shard where the main EM run is sharded.  Returns the kept positives' own packing where
// a record was dropped (the caller frees it or hands it on), else null: run.packed is the kept set
bamm_packed* upload_positives(Run& run, const std::vector<uint64_t>& off, const std::vector<uint8_t>& keep, bamm_seqs* dseqs_all) {
    const SlotPlan& plan = run.plan;
    bamm_packed* const packed = run.packed;
    bamm_packed* filtered = nullptr;
    for (auto& dv : run.devs) run.make_ctx(dv);
    if (!run.kept_all()) {                                   // re-pack only the kept records; kmers are position-local
        std::vector<uint64_t> kept_off{0};
        std::vector<uint64_t> km;
        std::vector<uint32_t> y10(packed->total_len);
        bamm_unpack_y(packed, BAMM_MAX_ORDER, y10.data());
        for (size_t n = 0; n < run.pos.size(); n++)
            if (keep[n]) { for (uint64_t i = off[n]; i < off[n + 1]; i++) km.push_back(y10[i]); kept_off.push_back(km.size()); }
        if (bamm_pack_kmers(km.data(), kept_off.data(), kept_off.size() - 1, &filtered)) die_abi("re-pack");
    }
    const bamm_packed* use = filtered ? filtered : packed;
    if (dseqs_all && filtered) { bamm_seqs_destroy(dseqs_all); dseqs_all = nullptr; }
    for (size_t d = 0; d < run.devs.size(); d++) {
        Dev& dv = run.devs[d];
        const bool want_full = (plan.in_em_group(d) && !plan.sharded) || (d == 0 && run.o.score) || plan.runs_folds(d);
        if (want_full) {
            if (d == 0 && dseqs_all) dv.full = dseqs_all;   // nothing was dropped: the seeding copy is the training set
            else if (bamm_seqs_upload(dv.ctx, use, 0, use->n_seqs, &dv.full)) die_abi("upload");
        } else if (d == 0 && dseqs_all) {
            bamm_seqs_destroy(dseqs_all);
        }
        if (plan.sharded && plan.in_em_group(d)) {
            if (bamm_shard_range(use->len, use->n_seqs, run.seeds.max_w, (uint32_t)d, (uint32_t)plan.em_slots.size(), &dv.begin, &dv.end)) die_abi("shard range");
            if (bamm_seqs_upload(dv.ctx, use, dv.begin, dv.end, &dv.shard)) die_abi("upload of a shard");
        } else {
            dv.shard = dv.full; dv.begin = 0; dv.end = use->n_seqs;
        }
    }
    run.kept_len.assign(use->len, use->len + use->n_seqs);
    run.stage("device contexts + upload of the positives");
    return filtered;
}

void make_communicators(Run& run) {
    const SlotPlan& plan = run.plan;
    const size_t nc = plan.sharded ? plan.em_slots.size() : 1;
    std::vector<bamm_ctx*> ctxs;
    std::vector<bamm_comm*> comms(nc, nullptr);
    for (size_t d = 0; d < nc; d++) ctxs.push_back(run.devs[d].ctx);
    if (plan.distinct) {
        if (bamm_comm_init_all(ctxs.data(), (uint32_t)nc, comms.data())) die_abi("RCCL communicator");
    } else {                                                 // the largest buffer summed: the count table + 3, or EM::mask's histogram
        const uint64_t words = std::max<uint64_t>((uint64_t)run.seeds.max_w * (uint64_t(1) << (2 * (run.o.K + 1))) + 3, 2049);
        if (bamm_comm_init_local(ctxs.data(), (uint32_t)nc, words, comms.data())) die_abi("host-staged communicator");
    }
    for (size_t d = 0; d < nc; d++) run.devs[d].comm = comms[d];
    run.stage(plan.distinct ? "RCCL communicator over the GPUs" : "host-staged communicator over the contexts");
}

void copy_kept_records(Run& run, const std::vector<uint8_t>& keep) {
    const FastaSet& pos = run.pos;
    for (size_t n = 0; n < pos.size(); n++)
        if (keep[n]) {
            run.kept_headers_own.push_back(pos.headers[n]);
            run.kept_codes_own.insert(run.kept_codes_own.end(), pos.codes.begin() + pos.off[n], pos.codes.begin() + pos.off[n + 1]);
            run.kept_off_own.push_back(run.kept_codes_own.size());
        }
}

}  // namespace

void prepare(Run& run, NegativeSet& neg) {
    const Options& o = run.o;
    std::vector<uint64_t> off;
    std::vector<uint8_t> keep;
    bamm_seqs* dseqs_all = nullptr;
    bamm_packed* filtered = nullptr;
    read_and_pack(run, off, dseqs_all);
    if (o.verbose) std::cout << std::endl << "************************" << std::endl << "*   Background Model   *" << std::endl << "************************" << std::endl;
    background_model(run, dseqs_all);
    if (o.verbose) std::cout << std::endl << "***************************" << std::endl << "*   Initial Motif Model   *" << std::endl << "***************************" << std::endl;
    seed_models(run, off, dseqs_all, keep);
    if (o.verbose) std::cout << std::endl << "*********************" << std::endl << "*   BaMM Training   *" << std::endl << "*********************" << std::endl;
    run.plan = make_slot_plan(run.devs.size(), o.cvFold, o.EM, o.FDR, o.advanceEM && o.optimizeQ, o.device_list);
    if (o.timing && o.need_gpu()) print_slot_plan(std::cerr, run.plan, o.device_list, o.score);
    if (o.need_gpu()) {
        filtered = upload_positives(run, off, keep, dseqs_all);
        if (run.plan.sharded || o.forceComm) make_communicators(run);
    }
    if (o.score && !run.kept_all()) copy_kept_records(run, keep);
    if (o.score || o.FDR) {
        size_t mFold = o.mFold;
        const size_t minSeqN = 5000;
        if (run.posN < minSeqN) mFold = minSeqN / run.posN + (minSeqN % run.posN ? 1 : 0);
        run.negN = run.posN * mFold;
        neg.start(run, filtered ? filtered : run.packed, filtered, mFold);   // from here on `run` is read-only
    } else if (filtered) {
        bamm_packed_free(filtered);
    }
}

void print_statistics(const Run& run) {                     // Global::printStat (Global.cpp:346-392)
    const Options& o = run.o;
    const FastaSet& pos = run.pos;
    std::cout << std::endl << "******************" << std::endl << "*   Statistics   *" << std::endl << "******************" << std::endl;
    std::cout << "Alphabet type is ACGT";
    std::cout << "\nGiven initial model is " << base_name(o.seed_file) << ", BaMM order: " << o.K << ", bgmodel order: " << o.Kbg;
    std::cout << "\nBaMM is learned from " << (o.ss ? "single-stranded sequences." : "double-stranded sequences.");
    std::cout << "\nGiven positive sequence set is " << o.basename << ".\n	" << pos.size() << " sequences, max.length: " << pos.max_len
              << ", min.length: " << pos.min_len << "\n	base frequencies:";
    for (int i = 0; i < 4; i++) std::cout << ' ' << pos.base_freq[i] << "(" << "ACGT"[i] << ")";
    if (o.advanceEM) std::cout << "\n    " << o.f * 100 << "% of the sequences are used for EM after masking.";   // Global.cpp:370-372
    std::cout << "\nThe background model is generated based on cond.prob of " << o.sOrder << "-mers.";
    if (o.FDR) std::cout << "\nFolds for cross-validation (FDR estimation): " << o.cvFold;
    std::cout << std::endl << "------ Runtime: " << seconds_since(run.t0) << " seconds -------" << std::endl;
}

// Everything is written and closed.  What is left is giving memory back -- a dozen hipFree calls (each a device
// synchronisation), a hundred megabytes of host vectors, then the HIP runtime's own static destructors: 0.1 s of a
// 0.7 s command that ends anyway.  The process leaves here (no other thread is alive: the side threads were joined
// where their results were taken); --debug keeps the orderly teardown for leak checkers.
void leave(Run& run, NegativeSet& neg) {
    if (run.o.timing) fprintf(stderr, "[timing-abs] main left at %.4f\n", epoch_seconds());
    if (!run.o.debug) {
        // (every writer of the driver is a scoped std::ofstream / FILE closed where its stage ends; tests/test_cli_gpu.py compares
        // the files of a --debug run, which takes the orderly way out below, byte for byte with this one's)
        for (auto& dv : run.devs)
            if (dv.comm) { bamm_comm_destroy(dv.comm); dv.comm = nullptr; }      // peers of a sharded run are told, not left waiting
        std::cout.flush(); std::cerr.flush();
        fflush(nullptr);
        _exit(0);
    }
    for (size_t d = 0; d < run.devs.size(); d++) {
        Dev& dv = run.devs[d];
        if (dv.comm) bamm_comm_destroy(dv.comm);
        if (d == 0 && neg.all) bamm_seqs_destroy(neg.all);
        if (d < neg.cv.size() && neg.cv[d]) bamm_seqs_destroy(neg.cv[d]);
        if (dv.shard && dv.shard != dv.full) bamm_seqs_destroy(dv.shard);
        if (dv.full) bamm_seqs_destroy(dv.full);
        if (dv.ctx) bamm_ctx_destroy(dv.ctx);
    }
    bamm_packed_free(run.packed);
    if (run.o.timing) fprintf(stderr, "[timing-abs] teardown done at %.4f\n", epoch_seconds());
}

}  // namespace bammhost
