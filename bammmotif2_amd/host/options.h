// The command line of the BaMMmotif driver (options.cpp): the reference's flags and defaults and this build's extensions.
// Stands alone: nothing of the driver's state, threads or stages is needed to parse, or to read what was parsed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

namespace bammhost {

struct Options {                       // Global.cpp:6-96 defaults
    std::string out_dir, fasta, basename, neg_fasta, alphabet = "STANDARD";
    std::string seed_file, seed_tag, bg_file;
    bool ss = false, EM = false, CGS = false, FDR = false, score = false, verbose = false;
    bool optimizeQ = false, advanceEM = false, saveBaMMs = true, saveInitial = false, mops = false, zoops = true;
    bool genericNeg = false, savePRs = true, savePvalues = false, saveLogOdds = false;
    float pvalCutoff = 0.0001f;
    size_t maxPWM = std::numeric_limits<size_t>::max();
    uint32_t K = 2, Kbg = 2;
    std::vector<float> alpha{1.f, 1.f, 1.f}, alpha_bg{1.f, 1.f, 1.f};
    float beta = 7.0f, gamma = 3.0f, q = 0.3f, f = 0.05f, epsilon = 0.01f;
    std::vector<size_t> extend{0, 0};
    size_t cvFold = 4, mFold = 1, sOrder = 2, threads = 4;
    uint32_t max_iter = 1000;
    uint32_t seedKmers = 0;            // --seedKmers w: seeds from the w-mer counts of the positives (0 = a model file is given)
    bool seedGaps = false;             // --seedGaps [lo] hi: dyads as well, the halves of the w-mer seedGapLo..seedGapHi positions apart
    uint32_t seedGapLo = 0, seedGapHi = 0;
    int device = 0;
    bool timing = false, hostSeeding = false, hostPacking = false, hostSampler = false, hostPvalues = false, hostPositions = false, hostFdr = false, hostSeedCounts = false, forceComm = false, debug = false;
    size_t gpus = 1;                   // --gpus N: devices device .. device+N-1 (or --deviceList)
    std::vector<int> device_list;
    bool need_gpu() const { return EM || score || FDR; }
};
// exits on its own (no thread exists yet): 1 for a usage error or --help, -1 where OUTDIR cannot be created
Options parse(int nargs, char** args);

}  // namespace bammhost
