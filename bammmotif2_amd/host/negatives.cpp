// The negative set of --scoreSeqset / --FDR: sampler, packing and upload on a thread of their own (see NegativeSet in driver.h).
#include "driver.h"
#include "host_util.h"

namespace bammhost {

void NegativeSet::start(const Run& run, const bamm_packed* use, bamm_packed* filtered, size_t mFold) {
    // the folds of --FDR score every cvFold-th negative and nothing else (FDR.cpp:58-60): without --scoreSeqset
    // only those are generated, packed and uploaded (the others still consume their draws of the stream)
    const size_t stride = (run.o.FDR && !run.o.score) ? run.plan.fold_slot.size() : 0;
    cv.assign(run.devs.size(), nullptr);
    g_threads.negatives = std::thread(&NegativeSet::body, this, std::cref(run), use, filtered, mFold, stride);
}

void NegativeSet::body(const Run& run, const bamm_packed* use, bamm_packed* filtered, size_t mFold, size_t stride) {
    const Options& o = run.o;
    const std::vector<Dev>& devs = run.devs;
    const size_t ndev = devs.size(), n_pos = use->n_seqs;
    const auto t0 = Clock::now();
    bamm_packed* npk = nullptr;
    // the sampler on the device (csrc/negs.hip) where the kept positives are resident on slot 0 and the
    // negatives are wanted as a set of their own -- all of them, or the folds' subset; it declines (-s other than 2,
    // a libc that is not glibc, ...) with BAMM_ERR_UNSUPPORTED and the host path below takes over
    // (--scoreSeqset --saveLogOdds prints the negatives' text: the host path keeps their codes)
    size_t dfull = ndev;                                     // the first slot that holds every kept positive (with a sharded main
    for (size_t d = 0; d < ndev && dfull == ndev; d++) if (devs[d].full) dfull = d;   // run: a fold's slot)
    if (!o.hostSampler && dfull < ndev && (stride > 1 || !o.FDR) && !(o.score && o.saveLogOdds)) {
        const int rc = bamm_sample_negatives(devs[dfull].ctx, devs[dfull].full, (uint32_t)o.sOrder, mFold, o.genericNeg ? 1 : 0, stride, &npk, nullptr);
        if (rc != BAMM_OK && rc != BAMM_ERR_UNSUPPORTED) return fail_abi("negative sampler");
        if (rc == BAMM_OK) {
            on_device = true;
            if (filtered) bamm_packed_free(filtered);
            off = offsets_of(npk);
        }
    }
    if (!npk) {
        std::vector<uint32_t, DefaultInitAlloc<uint32_t>> ys(use->total_len ? use->total_len : 1);   // every cell is written
        const std::vector<uint64_t> uoff = offsets_of(use);
        std::string serr;
        const int rc = bamm_unpack_y(use, (uint32_t)o.sOrder, ys.data());
        if (filtered) bamm_packed_free(filtered);            // the thread is the last reader of the kept positives' packing
        if (rc) return fail_abi("unpack");
        if (sample_negatives(ys.data(), uoff.data(), n_pos, (uint32_t)o.sOrder, mFold, o.genericNeg, codes, off, serr, stride)) { err = serr; return; }
    }
    const auto t1 = Clock::now();
    t_sample = seconds_between(t0, t1);
    if (!npk && bamm_pack_codes(codes.data(), off.data(), off.size() - 1, 1, &npk)) return fail_abi("packing negatives");
    upload(run, npk, stride);
    bamm_packed_free(npk);
    t_pack = seconds_since(t1);
}

void NegativeSet::fail_abi(const char* what) { err = std::string("Error: ") + what + ": " + bamm_last_error(); }

void NegativeSet::upload_cv(const Run& run, const bamm_packed* pk) {
    for (size_t d = 0; d < run.devs.size(); d++)
        if (run.plan.runs_folds(d) && bamm_seqs_upload(run.devs[d].ctx, pk, 0, pk->n_seqs, &cv[d])) return fail_abi("upload negatives");
}

void NegativeSet::upload(const Run& run, const bamm_packed* npk, size_t stride) {
    const size_t cvF = run.plan.fold_slot.size();
    if (stride > 1) {                                        // what was sampled IS the folds' subset
        for (size_t n = 0; n + 1 < off.size(); n++) cv_len.push_back((uint32_t)(off[n + 1] - off[n]));
        return upload_cv(run, npk);
    }
    if (bamm_seqs_upload(run.devs[0].ctx, npk, 0, npk->n_seqs, &all)) return fail_abi("upload negatives");
    if (!run.o.FDR) return;
    std::vector<uint64_t> sub_off{0};                        // the folds' subset as a set of its own
    ByteVec sub_codes;
    for (size_t i = 0; i + cvF <= run.negN; i += cvF) {
        sub_codes.insert(sub_codes.end(), codes.begin() + (ptrdiff_t)off[i], codes.begin() + (ptrdiff_t)off[i + 1]);
        sub_off.push_back(sub_codes.size());
        cv_len.push_back((uint32_t)(off[i + 1] - off[i]));
    }
    bamm_packed* spk = nullptr;
    if (bamm_pack_codes(sub_codes.data(), sub_off.data(), sub_off.size() - 1, 1, &spk)) return fail_abi("packing negatives");
    upload_cv(run, spk);
    bamm_packed_free(spk);
}

// main thread only, before the first consumer of the negative set (the folds, --scoreSeqset)
void NegativeSet::ensure(Run& run) {
    if (!g_threads.negatives.joinable()) return;
    g_threads.negatives.join();
    if (!err.empty()) die(err);
    if (run.o.score) for (size_t n = 0; n + 1 < off.size(); n++) len.push_back((uint32_t)(off[n + 1] - off[n]));
    if (run.o.timing) std::cerr << "[timing-beside] negative set: sample (" << (on_device ? "device" : "host") << ", rand() stream of the reference) " << t_sample
                                << " s, pack + upload " << t_pack << " s, on a thread of their own beside the stages above" << std::endl;
    run.stage("negative set: wait for the sampler thread");
}

}  // namespace bammhost
