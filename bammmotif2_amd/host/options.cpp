// The command line of the BaMMmotif driver: the reference's flags and defaults (Global.cpp:142-341) and this build's
// extensions.  Nothing here depends on the rest of the driver (options.h; bamm_host.h for base_name and the host thread
// count): no thread exists yet, so every error leaves through exit().
#include <omp.h>
#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <iostream>
#include <sstream>

#include "bamm_host.h"
#include "options.h"

namespace bammhost {
namespace {

void print_help() {
    printf("\n==================================================================\n");
    printf("\n SYNOPSIS:  BaMMmotif OUTDIR SEQFILE [options] \n\n");
    printf("\t DESCRIPTION \n");
    printf("\t\t Learn Bayesian inhomogeneous Markov models (BaMMs) from sequence data (EM on an MI355X GPU).\n\n");
    printf("\t OUTDIR:  output directory for all results. \n");
    printf("\t SEQFILE: file with sequences from positive set in FASTA format\n\n");
    printf("\t OPTIONS (same names and defaults as the reference, Global.cpp:142-341):\n");
    printf("\t\t --basename <STRING> --negSeqFile <FILE> --ss --alphabet STANDARD\n");
    printf("\t\t --bindingSiteFile <FILE> | --PWMFile <FILE> | --BaMMFile <FILE> | --seedKmers <INT> (extension)   --maxPWM <INT>\n");
    printf("\t\t -k, --order <INT> (2)   -a, --alpha <FLOAT>..   -b, --beta <FLOAT> (7)   -r, --gamma <FLOAT> (3)\n");
    printf("\t\t --extend <INT> [<INT>]   --bgModelFile <FILE>   -K, --Order <INT> (2)   -A, --Alpha <FLOAT>..\n");
    printf("\t\t --EM   -q <FLOAT> (0.3)   --optimizeQ   --verbose   --saveBaMMs   --saveInitialBaMMs\n");
    printf("\t EXTENSIONS of this build:\n");
    printf("\t\t --maxEMIterations <INT> (1000)   -e, --epsilon <FLOAT> (0.01)   --device <INT> (0)\n");
    printf("\t\t --timing (wall time per stage on stderr)   --hostSeeding (initFromPWM's pass on the host)\n");
    printf("\t\t --hostPacking (Sequence.cpp's encoding and the background counts on the host instead of the device)\n");
    printf("\t\t --hostSampler (SeqGenerator's negative sampler on the host instead of the device)\n");
    printf("\t\t --hostPvalues (--scoreSeqset: ScoreSeqSet::calcPvalues on downloaded window scores instead of on the device)\n");
    printf("\t\t --hostPositions (--saveBaMMs: .positions from downloaded responsibilities instead of the sites found on the device)\n");
    printf("\t\t --hostFdr (--FDR --mops: the MOPS statistics from downloaded window scores instead of on the device)\n");
    printf("\t\t --seedKmers <INT> (6..8: no model file; the most enriched w-mers of SEQFILE, counted on the device, seed the run\n");
    printf("\t\t\t through OUTDIR/<basename>_seeds.meme; --maxPWM defaults to 4 here)\n");
    printf("\t\t --seedGaps <INT> [<INT>] (--seedKmers 6 or 8: dyads as well -- the two halves of the w-mer G positions apart, any bases\n");
    printf("\t\t\t between them; one value: gaps 0..G, two: lo..hi; w + gap <= 16.  A seed's PWM spans its gap: TGACnnnnGCAT)\n");
    printf("\t\t --hostSeedCounts (--seedKmers: the w-mer counts on the host instead of on the device)\n");
    printf("\t\t --gpus <INT> (1)   --deviceList <INT,INT,..>\n");
    printf("\t\t\t --EM: the sequences are sharded over the GPUs, one RCCL all-reduce of the count table per iteration;\n");
    printf("\t\t\t --FDR: cross-validation fold f runs on GPU f mod N (FDR.cpp:37 runs the folds on host threads).\n");
    printf("\t\t\t Output files do not depend on the number of GPUs.\n");
    printf("\n==================================================================\n");
}

// Tokeniser in the spirit of getopt_pp (src/getopt_pp/getopt_pp.cpp:71-141): "--long", "-s", combined
// short flags, values = following tokens that do not look like options (negative numbers do not).
struct Args {
    std::map<std::string, std::vector<std::string>> longs;
    std::map<char, std::vector<std::string>> shorts;
    std::set<std::string> used_long;
    std::set<char> used_short;

    static bool looks_like_option(const std::string& t) {
        if (t.size() < 2 || t[0] != '-') return false;
        if (isdigit((unsigned char)t[1]) || t[1] == '.') return false;      // -3, -.5 are values
        return true;
    }
    Args(int n, char** v) {
        std::vector<std::string>* cur = nullptr;
        for (int i = 1; i < n; i++) {
            std::string t = v[i];
            if (looks_like_option(t)) {
                if (t[1] == '-') {
                    cur = &longs[t.substr(2)];
                } else {
                    for (size_t c = 1; c < t.size(); c++) cur = &shorts[t[c]];
                }
            } else if (cur) {
                cur->push_back(t);
            }
        }
    }
    bool present(char s, const std::string& l) {
        bool p = false;
        if (s && shorts.count(s)) { used_short.insert(s); p = true; }
        if (!l.empty() && longs.count(l)) { used_long.insert(l); p = true; }
        return p;
    }
    const std::vector<std::string>* values(char s, const std::string& l) {
        if (s && shorts.count(s)) { used_short.insert(s); return &shorts[s]; }
        if (!l.empty() && longs.count(l)) { used_long.insert(l); return &longs[l]; }
        return nullptr;
    }
    template <class T>
    bool get(char s, const std::string& l, T& out) {
        const auto* v = values(s, l);
        if (!v || v->empty()) return false;
        std::stringstream ss((*v)[0]);
        T tmp;
        if (!(ss >> tmp)) { std::cerr << "Error: bad value for option " + (l.empty() ? std::string(1, s) : l) << std::endl; exit(1); }
        out = tmp;
        return true;
    }
    bool get_str(char s, const std::string& l, std::string& out) {
        const auto* v = values(s, l);
        if (!v || v->empty()) return false;
        out = (*v)[0];
        return true;
    }
    template <class T>
    bool get_vec(char s, const std::string& l, std::vector<T>& out) {
        const auto* v = values(s, l);
        if (!v) return false;
        for (const auto& t : *v) { std::stringstream ss(t); T x; if (ss >> x) out.push_back(x); }
        return true;
    }
    bool remain() const {
        for (auto& kv : longs) if (!used_long.count(kv.first)) return true;
        for (auto& kv : shorts) if (!used_short.count(kv.first)) return true;
        return false;
    }
};

template <class T>
void fit(std::vector<T>& v, size_t n) {     // Global.cpp:210-223: truncate or pad with the last value
    if (v.size() > n) v.resize(n);
    else if (v.size() < n) v.resize(n, v.empty() ? T(1) : v.back());
}

// the reference's flags, in Global.cpp's order
void parse_reference(Args& a, Options& o) {
    if (!a.get_str(0, "basename", o.basename)) o.basename = base_name(o.fasta);
    a.present(0, "maskPosSequenceSet");
    if (!a.get_str(0, "negSeqFile", o.neg_fasta)) o.neg_fasta = o.fasta;
    o.genericNeg = a.present(0, "genericNeg");
    a.get_str(0, "alphabet", o.alphabet);
    o.ss = a.present(0, "ss");
    { std::string tmp; a.get_str(0, "intensityFile", tmp); }
    if (a.present(0, "seedGaps") && !a.longs.count("seedKmers")) {
        fprintf(stderr, "Error: --seedGaps needs --seedKmers 6 or 8.\n");
        exit(1);
    }
    if (a.present(0, "seedKmers")) {
        // this build's fourth way to give the initial model: the seeds are found in SEQFILE itself and written to
        // OUTDIR/<basename>_seeds.meme, which the run then reads like any --PWMFile
        for (const char* file_flag : {"bindingSiteFile", "PWMFile", "BaMMFile"})
            if (a.longs.count(file_flag)) {
                fprintf(stderr, "Error: --seedKmers cannot be combined with --%s: give the initial model one way.\n", file_flag);
                exit(1);
            }
        if (!a.get(0, "seedKmers", o.seedKmers) || o.seedKmers < 6 || o.seedKmers > 8) {
            fprintf(stderr, "Error: --seedKmers takes a width from 6 to 8.\n");
            exit(1);
        }
        if (a.present(0, "seedGaps")) {
            // dyads: one value G means the gaps 0..G, two mean lo..hi
            std::vector<uint32_t> gaps;
            a.get_vec(0, "seedGaps", gaps);
            if (o.seedKmers == 7) { fprintf(stderr, "Error: --seedGaps needs --seedKmers 6 or 8.\n"); exit(1); }
            if (gaps.empty() || gaps.size() > 2 || gaps.size() != a.longs["seedGaps"].size()) { fprintf(stderr, "Error: --seedGaps takes one or two gaps.\n"); exit(1); }
            o.seedGaps = true;
            o.seedGapLo = gaps.size() == 2 ? gaps[0] : 0;
            o.seedGapHi = gaps.back();
            if (o.seedGapHi > 16 - o.seedKmers || o.seedGapLo > 16 - o.seedKmers) { fprintf(stderr, "Error: --seedGaps: w + gap may not exceed 16.\n"); exit(1); }
            if (o.seedGapLo > o.seedGapHi) { fprintf(stderr, "Error: --seedGaps: the first gap may not exceed the second.\n"); exit(1); }
        }
        o.seed_file = o.out_dir + '/' + o.basename + "_seeds.meme";
        o.seed_tag = "PWM";
    }
    else if (a.get_str(0, "bindingSiteFile", o.seed_file)) o.seed_tag = "bindingsites";
    else if (a.get_str(0, "PWMFile", o.seed_file)) o.seed_tag = "PWM";
    else if (a.get_str(0, "BaMMFile", o.seed_file)) o.seed_tag = "BaMM";
    else { fprintf(stderr, "Error: No initial model is provided.\n"); exit(1); }
    if (!a.get(0, "maxPWM", o.maxPWM) && o.seedKmers) o.maxPWM = 4;
    o.mops = a.present(0, "mops");
    a.get(0, "zoops", o.zoops);
    a.get('k', "order", o.K);
    if (a.present('a', "alpha")) {
        o.alpha.clear();
        a.get_vec('a', "alpha", o.alpha);
        fit(o.alpha, o.K + 1);
    } else {
        fit(o.alpha, o.K + 1);
        a.get('b', "beta", o.beta);
        a.get('r', "gamma", o.gamma);
        for (uint32_t k = 1; k <= o.K; k++) o.alpha[k] = o.beta * powf(o.gamma, (float)k);   // Global.cpp:227-232
    }
    if (a.present(0, "extend")) {
        o.extend.clear();
        a.get_vec(0, "extend", o.extend);
        if (o.extend.size() < 1 || o.extend.size() > 2) { fprintf(stderr, "--extend format error.\n"); exit(1); }
        if (o.extend.size() == 1) o.extend.resize(2, o.extend.back());
    }
    a.get_str(0, "bgModelFile", o.bg_file);
    a.get('K', "Order", o.Kbg);
    if (a.present('A', "Alpha")) {
        o.alpha_bg.clear();
        a.get_vec('A', "Alpha", o.alpha_bg);
        fit(o.alpha_bg, o.Kbg + 1);
    } else {
        fit(o.alpha_bg, o.Kbg + 1);
        for (uint32_t k = 1; k <= o.Kbg; k++) o.alpha_bg[k] = 10.0f;                           // Global.cpp:274-278
    }
    o.EM = a.present(0, "EM");
    if ((o.CGS = a.present(0, "CGS"))) {
        for (const char* n : {"noInitialZ", "noAlphaOpti", "GibbsMH", "dissample", "noZSampling", "noQSampling"}) a.present(0, n);
    }
    a.present(0, "debugAlphas");
    a.present(0, "generatePseudoSet");
    a.get('q', "", o.q);
    a.get('f', "", o.f);
    if ((o.FDR = a.present(0, "FDR"))) {
        a.get('m', "mFold", o.mFold);
        a.get('n', "cvFold", o.cvFold);
        a.get('s', "sOrder", o.sOrder);
    }
    o.score = a.present(0, "scoreSeqset");
    a.get(0, "pvalCutoff", o.pvalCutoff);
    o.verbose = a.present(0, "verbose");
    o.debug = a.present(0, "debug");
    o.saveBaMMs = a.present(0, "saveBaMMs");                  // presence overwrites the default (getopt_pp.h:497)
    o.saveInitial = a.present(0, "saveInitialBaMMs");
    a.get(0, "savePRs", o.savePRs);
    o.savePvalues = a.present(0, "savePvalues");
    o.saveLogOdds = a.present(0, "saveLogOdds");
    for (const char* n : {"saveBgModel", "makeMovie", "B2", "B3", "B3prime"}) a.present(0, n);
    o.optimizeQ = a.present(0, "optimizeQ");
    o.advanceEM = a.present(0, "advanceEM");
    a.get(0, "threads", o.threads);
    omp_set_num_threads((int)std::max<size_t>(1, o.threads));   // Global.cpp:331-333 (default 4)
    // packing, the negative sampler and the sorts give the same bytes however they are cut: all granted cores
    bamm_set_host_threads((uint32_t)std::max<size_t>(o.threads, (size_t)host_parallelism()));
}

// extensions of this build (the reference advertises but never parses the first two, Global.cpp:479-491)
void parse_extensions(Args& a, Options& o) {
    a.get(0, "maxEMIterations", o.max_iter);
    a.get('e', "epsilon", o.epsilon);
    a.get(0, "device", o.device);
    o.timing = a.present(0, "timing");
    o.hostSeeding = a.present(0, "hostSeeding");
    o.hostPacking = a.present(0, "hostPacking");
    o.hostSampler = a.present(0, "hostSampler");
    o.hostPvalues = a.present(0, "hostPvalues");
    o.hostPositions = a.present(0, "hostPositions");
    o.hostFdr = a.present(0, "hostFdr");
    o.hostSeedCounts = a.present(0, "hostSeedCounts");
    a.get(0, "gpus", o.gpus);
    {   // --deviceList 0,1,2: explicit devices (a device may appear twice for the fold replicas of --FDR; the
        // sharded --EM wants distinct ones, RCCL has one rank per GPU)
        std::string list;
        if (a.get_str(0, "deviceList", list)) {
            std::stringstream ss(list);
            std::string tok;
            while (std::getline(ss, tok, ',')) if (!tok.empty()) o.device_list.push_back(atoi(tok.c_str()));
            if (o.device_list.empty()) { fprintf(stderr, "--deviceList format error.\n"); exit(1); }
            o.gpus = o.device_list.size();
        }
    }
    if (o.gpus < 1) o.gpus = 1;
    if (o.device_list.empty()) for (size_t d = 0; d < o.gpus; d++) o.device_list.push_back(o.device + (int)d);
    o.forceComm = a.present(0, "forceComm");
}

}  // namespace

Options parse(int nargs, char** args) {
    if (nargs < 3) {
        std::cerr << "Error: Arguments are missing! \n" << std::endl;
        print_help();
        exit(1);
    }
    Options o;
    o.out_dir = args[1];
    struct stat st;
    if (stat(o.out_dir.c_str(), &st) != 0) {                 // utils.h:154-165
        std::cout << "New output directory is created automatically.\n";
        if (system(("mkdir -p " + o.out_dir).c_str()) != 0) {
            std::cerr << "Error: Directory " << o.out_dir << " could not be created." << std::endl;
            exit(-1);
        }
    }
    o.fasta = args[2];
    Args a(nargs - 2, args + 2);                              // the FASTA path plays argv[0] (Global.cpp:142)
    if (a.present('h', "help")) { print_help(); exit(1); }
    parse_reference(a, o);
    parse_extensions(a, o);
    if (a.remain()) {
        print_help();
        std::cerr << "Oops! Unknown option(s) remaining... \n\n";
        exit(1);
    }
    return o;
}

}  // namespace bammhost
