// BaMMmotif OUTDIR FASTA [options] -- MI355X drop-in for the reference driver (src/refinement/mainBaMM.cpp, Global.cpp).
// The EM itself runs on the GPU through the C ABI (include/bamm_em.h); everything here is host plumbing with the reference's
// flags, defaults, messages and output files, including --scoreSeqset (.occurrence), --FDR (cross-validated .zoops.stats),
// --saveLogOdds and --advanceEM (EM::mask); --gpus N shards the sequences (--EM) and spreads the cross-validation folds
// (--FDR) over N GPUs.  --seedKmers w (an extension) needs no model file: the most enriched w-mers of the positives, counted
// on the device, become OUTDIR/<basename>_seeds.meme, which the run reads like a --PWMFile (--seedGaps: dyads as well, the w-mer's
// halves up to 16 - w positions apart).  Not ported (exit with a clear message): --CGS, non-STANDARD alphabets.
// main() is the sequence of stages, in mainBaMM.cpp's order; the stages and the state they share are in driver.h.
#include <cstdio>
#include <cstdlib>

#include "driver.h"

using namespace bammhost;

int main(int nargs, char* args[]) {
    Run run;                                                 // starts the wall clock
    std::cout << std::endl
              << "======================================" << std::endl
              << "=      Welcome to use BaMM!motif     =" << std::endl
              << "=                   Version 2.0      =" << std::endl
              << "=     MI355X build (bammmotif2_amd)  =" << std::endl
              << "======================================" << std::endl;
    srand(42);                                               // mainBaMM.cpp:22; nothing draws from the stream before the packing
    run.o = parse(nargs, args);
    const Options& o = run.o;
    if (o.timing) fprintf(stderr, "[timing-abs] main entered at %.4f\n", epoch_seconds() - seconds_since(run.t0));
    if (o.alphabet != "STANDARD") die("Error: this build supports --alphabet STANDARD only.");
    if (o.CGS) die("Error: --CGS (collapsed Gibbs sampling) is not part of the MI355X build.");
    if (o.K > BAMM_MAX_ORDER) die("Error: model order above 10 is not supported (kmer_ spans 11 bases).");
    if (o.need_gpu()) run.warm.start(o.device_list[0]);      // nothing is decided there: the contexts proper are created where they always were

    NegativeSet neg;
    prepare(run, neg);                                       // positives, background model, seeds, plan, resident sets; the sampler starts
    Folds folds(run, neg);
    std::string err;
    for (size_t n = 0; n < run.seeds.motifs.size(); n++) {
        Motif motif = run.seeds.motifs[n];                   // deep copy (mainBaMM.cpp:121)
        const std::string mbase = o.basename + "_motif_" + std::to_string(n + 1);
        if (o.saveInitial && motif_write(o.out_dir, o.basename + "_init_motif_" + std::to_string(n + 1), motif, err)) die(err);
        if (run.plan.overlap) {                              // this motif's folds train while its main run does
            neg.ensure(run);                                 // the folds score negatives
            folds.start(n);
        }
        Joiner fold_join{g_threads.folds};
        if (o.EM) train_motif(run, n, motif, mbase);
        else std::cout << "Note: the model is not optimized!\n";
        if (motif_write(o.out_dir, mbase, motif, err)) die(err);
        run.stage("write model (+ .counts/.positions)");
        if (o.score) {
            neg.ensure(run);
            score_seqset(run, neg, motif, mbase);
        }
    }
    neg.ensure(run);
    if (o.FDR) fdr_stage(run, folds);
    print_statistics(run);
    leave(run, neg);
    return 0;
}
