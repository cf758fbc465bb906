// Private header of the BaMMmotif driver (main.cpp and the units beside it): the state its stages share, who owns it, and the
// stages themselves.  Plain structs and free functions; every stage that takes a `Run&` runs on the main thread, a thread
// body sees a `const Run&`.
#pragma once
#include <chrono>
#include <iostream>
#include <thread>

#include "bamm_host.h"
#include "options.h"
#include "slot_plan.h"

namespace bammhost {

// ---- context.cpp: side threads, clocks, the run context ----
using Clock = std::chrono::high_resolution_clock;
inline double seconds_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
inline double seconds_since(Clock::time_point t) { return seconds_between(t, Clock::now()); }

// Threads beside main(): exit() runs the static destructors of the HIP runtime, the OpenMP runtime and this program under
// whatever is still running, so die() -- called on the main thread only; the side threads report through strings -- joins
// every one of them first.  All three do bounded work (no collective: the sharded ranks are joined where they start).
struct SideThreads {
    std::thread hip_warmup;                // brings the HIP runtime up while the FASTA file is read (WarmUp)
    std::thread negatives;                 // samples, packs and uploads the negatives beside the main run (NegativeSet)
    std::thread folds;                     // overlap mode: a motif's folds train while its main run does (Folds)
};
extern SideThreads g_threads;
struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } };
[[noreturn]] void die(const std::string& msg);
[[noreturn]] void die_abi(const char* what);      // + bamm_last_error() of the calling (main) thread

// one slot per GPU (a single one unless --gpus / --deviceList): context, resident positives, RCCL rank
struct Dev {
    int device = 0;
    bamm_ctx* ctx = nullptr;
    bamm_seqs* full = nullptr;         // every kept positive (scoring, fold replicas, single-GPU EM)
    bamm_seqs* shard = nullptr;        // this GPU's range of the kept positives (the full set with one GPU)
    bamm_comm* comm = nullptr;
    uint64_t begin = 0, end = 0;
};

// The HIP runtime takes 0.1-0.2 s to come up on first use: it does so on a thread of its own while the FASTA file is read,
// and the first slot's context (the runtime's first use of a device, its stream, the library's code objects) is created
// there as well.  `ctx` is written by the thread only and read by take(), which joins it first.
struct WarmUp {
    int device = 0;
    bamm_ctx* ctx = nullptr;
    Joiner join{g_threads.hip_warmup};
    void start(int device_);
    bamm_ctx* take(int device_);           // the warm-up's context if it is on this device, once
    void body();
};

// What the stages share: built by main() and prepare() on the main thread, which starts the sampler thread as prepare()'s
// last step.  From then on side threads read it and nobody writes it, with three exceptions, all on the main thread and
// none of them read by a side thread: the stage clock `t_stage`; the warm-up's context inside `warm` (taken by make_ctx(),
// whose last call precedes the sampler); and leave(), which destroys the communicators when every side thread is joined.
struct Run {
    const Clock::time_point t0 = Clock::now();
    Clock::time_point t_stage = t0;
    Options o;
    WarmUp warm;
    FastaSet pos;
    bamm_packed* packed = nullptr;         // every positive record
    BgModel bg;
    SeedSet seeds;
    SlotPlan plan;
    std::vector<Dev> devs;
    // the kept positives (at least as long as the widest motif, mainBaMM.cpp:75-83): lengths as the resident sets hold them;
    // FASTA codes / headers in the same order -- what --scoreSeqset's and --saveBaMMs' writers print; copies only where a
    // record was dropped (0.1 s at a million records otherwise, for nothing)
    size_t posN = 0, negN = 0;             // negN: negatives the reference would hold (all of them, sampled or not)
    std::vector<uint32_t> kept_len;
    std::vector<std::string> kept_headers_own;
    ByteVec kept_codes_own;
    std::vector<uint64_t> kept_off_own{0};
    bool kept_all() const { return posN == pos.size(); }
    const std::vector<std::string>& kept_headers() const { return kept_all() ? pos.headers : kept_headers_own; }
    const uint8_t* kept_codes() const { return (kept_all() ? pos.codes : kept_codes_own).data(); }
    const uint64_t* kept_off() const { return (kept_all() ? pos.off : kept_off_own).data(); }

    void stage(const char* what);          // --timing: wall time per stage on stderr (stdout stays the reference's)
    void make_ctx(Dev& dv);                // joins the warm-up and takes its context where the device matches
};
double epoch_seconds();

struct NegativeSet;
void prepare(Run& run, NegativeSet& neg);  // FASTA .. upload of the positives, communicators, start of the sampler
void print_statistics(const Run& run);     // Global::printStat
void leave(Run& run, NegativeSet& neg);    // _exit(0), or the orderly teardown under --debug

// ---- negatives.cpp ----
// The negative set sampled from the s-mer statistics of the kept positives (mainBaMM.cpp:97-116).  The sampler, the packing
// and the upload run on a thread of their own BESIDE the seeding and the main EM run, which need none of it.  From start()
// until ensure() has joined that thread, the thread alone touches the members below and the `filtered` packing it was
// handed: it is that packing's last reader and frees it.  ensure() runs on the main thread only, before each consumer
// (the overlapped folds, --scoreSeqset, the FDR stage).
struct NegativeSet {
    ByteVec codes;                         // FASTA codes (host sampler only: --saveLogOdds prints them)
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> len;             // all negatives: filled by ensure() for --scoreSeqset
    std::vector<uint32_t> cv_len;          // lengths of the folds' subset (every cvFold-th negative)
    bamm_seqs* all = nullptr;              // resident on slot 0, all of them (--scoreSeqset)
    std::vector<bamm_seqs*> cv;            // by slot: every cvFold-th negative -- all the folds of --FDR ever score (FDR.cpp:58-60)
    bool on_device = false;
    double t_sample = 0, t_pack = 0;
    std::string err;
    Joiner join{g_threads.negatives};

    void start(const Run& run, const bamm_packed* use, bamm_packed* filtered, size_t mFold);
    void ensure(Run& run);
    void body(const Run& run, const bamm_packed* use, bamm_packed* filtered, size_t mFold, size_t stride);
    void upload(const Run& run, const bamm_packed* npk, size_t stride);
    void upload_cv(const Run& run, const bamm_packed* pk);                  // the folds' subset, on every slot that runs folds
    void fail_abi(const char* what);                                        // err = what + bamm_last_error() of the sampler thread
};

// ---- em_run.cpp / score.cpp ----
bamm_em_params em_params(const Run& run, const Motif& m);
// the main EM run of motif n (mainBaMM.cpp:131-147): trains `motif` in place, writes .counts / .positions with --saveBaMMs
void train_motif(Run& run, size_t n, Motif& motif, const std::string& mbase);
// scorer over a resident set: MOPS scores (concatenated), ZOOPS maxima; non-zero with bamm_last_error() of the caller's thread
int score_set(const BgModel& bg, bamm_ctx* ctx, bamm_seqs* set, const std::vector<uint32_t>& lens, const Motif& m, std::vector<float>& mops,
              std::vector<float>& zoops, const uint8_t* subset = nullptr, bool want_mops = true, std::vector<uint64_t>* z_out = nullptr);
void score_seqset(Run& run, const NegativeSet& neg, const Motif& motif, const std::string& mbase);   // mainBaMM.cpp:171-236

// ---- folds.cpp ----
struct FoldOut { std::vector<float> posMax, negMax, posAll, negAll; float q = 0.f; std::string log, err; };
struct FdrPlanTimes { size_t slots = 0, runs = 0; double seal = 0, absorb = 0, merge = 0; };
// --FDR, per motif: every fold's scores, and with --mops the handle that holds the window scores on the device.
// run_motif(n) writes entry n of the three vectors and nothing else.  In overlap mode it runs on the fold thread
// (start(n); main()'s Joiner joins it before the next motif), otherwise on the main thread inside fdr_stage(), which is
// the only reader.  Messages of the ABI are taken on the thread whose call failed (FoldOut::err).
struct Folds {
    const Run& run;
    const NegativeSet& neg;
    const bool device_fdr;                 // --saveLogOdds (which prints the scores) and --hostFdr download them: host/fdr.cpp's path
    std::vector<std::vector<FoldOut>> results;
    std::vector<bamm_fdr*> handles;
    std::vector<FdrPlanTimes> times;
    Folds(const Run& run_, const NegativeSet& neg_);
    void start(size_t n);
    void run_motif(size_t n);
};
void fdr_stage(Run& run, Folds& folds);    // mainBaMM.cpp:243-265, FDR.cpp:28-145: merge in fold order, statistics, writers

}  // namespace bammhost
