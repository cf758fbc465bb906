// The negative-set sampler's tables and sampling loops (seq_generator/SeqGenerator.cpp), for host/fdr.cpp's
// sample_negatives alone.  fp32 expression order and the order of the stream's draws are the reference's.
#pragma once
#include <omp.h>

#include <algorithm>
#include <cstdlib>

#include "bamm_host.h"
#include "host_util.h"
#include "../csrc/glibc_rand.h"
#include "../csrc/neg_layout.h"

namespace bammhost {

struct NegSampler {
    uint32_t s;
    std::vector<float> v, range_bar, v_seq;      // flat [k][y]
    std::vector<size_t> n, n_seq;
    std::vector<float> A;

    explicit NegSampler(uint32_t s_order) : s(s_order) {
        const size_t tot = bgoff(s + 1);
        v.assign(tot, 0.f); range_bar.assign(tot, 0.f); v_seq.assign(tot, 0.f);
        n.assign(tot, 0); n_seq.assign(tot, 0);
        A.assign(s + 1, 20.f);                    // SeqGenerator.cpp:29-32
    }

    void kmer_frequency(const uint32_t* y_s, const uint64_t* off, size_t n_seqs) {   // :63-110
        std::fill(n.begin(), n.end(), 0);
        // integer counts: a histogram per host thread, summed -- the same numbers however the sequences are cut
        const int T = std::max(1, std::min<int>(host_parallelism(), (int)(n_seqs / 4096 + 1)));
        std::vector<std::vector<size_t>> part((size_t)T, std::vector<size_t>(n.size(), 0));
#pragma omp parallel for schedule(static) num_threads(T)
        for (long i = 0; i < (long)n_seqs; i++) {
            std::vector<size_t>& mine = part[(size_t)omp_get_thread_num()];
            const size_t L = off[i + 1] - off[i];
            const uint32_t* km = y_s + off[i];
            for (uint32_t k = 0; k <= s; k++)
                for (size_t j = k; j < L; j++) mine[bgoff(k) + km[j] % ipow4(k + 1)]++;
        }
        for (auto& pt : part)
            for (size_t c = 0; c < n.size(); c++) n[c] += pt[c];
        bamm::neg_set_tables(n.data(), s, A.data(), v.data(), range_bar.data(), [](uint32_t k) { return bgoff(k); });   // shared with the device sampler
    }

    void rescale(const uint32_t* km, size_t L) {   // :112-186, written for s = 2
        std::fill(n_seq.begin(), n_seq.end(), 0);
        for (uint32_t k = 0; k <= s; k++)
            for (size_t j = k; j < L; j++) n_seq[bgoff(k) + km[j] % ipow4(k + 1)]++;
        float sum = 0.f;
        for (size_t y = 0; y < 4; y++) {
            v_seq[y] = v[y];
            sum += v_seq[y];
            range_bar[y] = sum;
        }
        {
            const uint32_t k = 1;
            const size_t o1 = bgoff(1), o0 = bgoff(0);
            for (size_t y = 0; y < 16; y++) {
                const size_t y2 = y % 4;
                v_seq[o1 + y] = v[o1 + y] * ((float)n_seq[o1 + y] + A[k - 1] * v[o0 + y2]) / v[o0 + y2] / ((float)L + A[k - 1]);
            }
            float norm[4] = {0.f, 0.f, 0.f, 0.f};
            for (size_t y = 0; y < 16; y++) {
                const size_t yk = y / 4;
                v_seq[o1 + y] = ((float)n_seq[o1 + y] + A[k] * v_seq[o1 + y]) / ((float)n_seq[o0 + yk] + A[k]);
                norm[yk] += v_seq[o1 + y];
            }
            for (size_t y = 0; y < 16; y++) v_seq[o1 + y] /= norm[y / 4];
            for (size_t y = 0; y < 16; y++) {
                if (y % 4 == 0) sum = 0.0f;
                sum += v_seq[o1 + y];
                range_bar[o1 + y] = sum;
            }
        }
        {
            const uint32_t k = 2;
            const size_t o2 = bgoff(2), o1 = bgoff(1);
            for (size_t y = 0; y < 64; y++) {
                const size_t y2 = y % 16, yk = y / 4;
                v_seq[o2 + y] = ((float)n_seq[o2 + y] + A[k] * v_seq[o1 + y2]) / ((float)n_seq[o1 + yk] + A[k]);
                if (y % 4 == 0) sum = 0.0f;
                sum += v_seq[o2 + y];
                range_bar[o2 + y] = sum;
            }
        }
    }

    // glibc's rand() restated (csrc/glibc_rand.h): used only after its first draws have been checked against
    // srand(42)/rand() of the running libc, otherwise the sampler stays on rand(); jump(n) lets every host thread
    // start in the middle of the one stream.  Every later rand() consumer reseeds (FDR.cpp:153).
    bamm::GlibcRandStream stream;
    float next_random() { return (float)stream.next() / (float)RAND_MAX; }

    // positions 0 .. min(s, L) - 1, from the bars of the orders below s; random(i) is position i's draw, asked for in
    // ascending i (:222-283 == :296-341, the same sampling loop)
    template <class Random>
    void first_bases(size_t L, uint8_t* seq, Random&& random) const {
        const float r0 = random(0);
        for (uint8_t y = 0; y < 4; y++)
            if (r0 <= range_bar[y]) { seq[0] = y + 1; break; }
        for (size_t i = 1; i < s && i < L; i++) {
            size_t yk = 0;
            for (size_t k = i; k > 0; k--) yk += (size_t)(seq[i - k] - 1) * ipow4(k);
            const float r = random(i);
            for (size_t y = yk, a = 1; y < yk + 4; y++, a++) {
                seq[i] = (uint8_t)a;
                if (r <= range_bar[bgoff(i) + y]) break;
            }
        }
    }
    // context of the first s bases (yk = sum_k (seq[i-k]-1) * 4^k), which next_base rolls forward
    size_t first_context(const uint8_t* seq) const {
        size_t ctx = 0;
        for (size_t k = s; k > 0; k--) ctx = ctx * 4 + (size_t)(seq[s - k] - 1);
        return ctx;
    }
    // the main step: the first base whose cumulative bar reaches `random`, the last one when none does; the bars (`bar`:
    // order s's) are running sums (non-decreasing), so counting the bars below is the same thing
    static uint8_t next_base(const float* bar, size_t ctx_mask, size_t& ctx, float random) {
        const float* b4 = bar + ctx * 4;
        const uint8_t a = (uint8_t)(1 + (random > b4[0]) + (random > b4[1]) + (random > b4[2]));
        ctx = (ctx * 4 + (size_t)(a - 1)) & ctx_mask;
        return a;
    }

    void draw(size_t L, uint8_t* seq) {
        first_bases(L, seq, [this](size_t) { return next_random(); });
        if (s >= L) return;
        const size_t ctx_mask = ipow4(s) - 1;
        const float* bar = range_bar.data() + bgoff(s);
        size_t ctx = first_context(seq);
        for (size_t i = s; i < L; i++) seq[i] = next_base(bar, ctx_mask, ctx, next_random());
    }

    // F sequences of the same length from the same tables, drawn one after the other from the
    // stream (sequence f consumes draws [f*L, (f+1)*L)) but advanced position by position together:
    // the per-base dependency chain (context -> bars -> base -> context) of one sequence overlaps
    // with those of the others.
    // keep (nullable): keep[f] == 0 -> sequence f still consumes its L draws of the stream but is not generated; the
    // kept ones are written one after the other (FDR.cpp:58-60 only ever scores every cvFold-th negative)
    void draw_many(size_t L, size_t F, uint8_t* seqs, std::vector<float>& rnd, std::vector<size_t>& ctx, const uint8_t* keep = nullptr) {
        if (s >= L || F == 1) {
            for (size_t f = 0; f < F; f++) {
                if (keep && !keep[f]) { for (size_t k = 0; k < L; k++) (void)stream.next(); continue; }
                draw(L, seqs);
                seqs += L;
            }
            return;
        }
        rnd.resize(F * L);
        for (size_t k = 0; k < F * L; k++) rnd[k] = next_random();
        ctx.assign(F, 0);
        std::vector<uint8_t*>& dst = dst_scratch;
        dst.assign(F, nullptr);
        for (size_t f = 0; f < F; f++) if (!keep || keep[f]) { dst[f] = seqs; seqs += L; }
        for (size_t f = 0; f < F; f++) {
            if (!dst[f]) continue;
            const float* r = rnd.data() + f * L;
            first_bases(L, dst[f], [r](size_t i) { return r[i]; });
            ctx[f] = first_context(dst[f]);
        }
        const size_t ctx_mask = ipow4(s) - 1;
        const float* bar = range_bar.data() + bgoff(s);
        for (size_t i = s; i < L; i++)
            for (size_t f = 0; f < F; f++)
                if (dst[f]) dst[f][i] = next_base(bar, ctx_mask, ctx[f], rnd[f * L + i]);
    }
    std::vector<uint8_t*> dst_scratch;
};

}  // namespace bammhost
