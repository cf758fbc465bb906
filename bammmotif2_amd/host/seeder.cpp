// De novo seeds from the exact w-mer table of the positives (bamm_kmer_counts / bamm_kmer_counts_host): every cell's
// z-score against the background model, the best cells that are no neighbours of each other, a PWM from each one's
// Hamming-1 neighbourhood, and the MEME file the driver then reads back like any --PWMFile.  The reference has no such
// stage.  Everything is double arithmetic on exact integers, in a fixed order: every machine gives the same seeds.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "bamm_host.h"
#include "host_util.h"

namespace bammhost {

namespace {

uint32_t revcomp(uint32_t y, uint32_t w) {
    uint32_t rc = 0;
    for (uint32_t i = 0; i < w; i++) { rc = (rc << 2) | (3u - (y & 3u)); y >>= 2; }
    return rc;
}

// P(y) under the background model: the product over the window's positions i = 0 .. w-1, oldest first, of the conditional
// probability of base i given the min(i, K) bases before it
double window_probability(uint32_t y, uint32_t w, const BgModel& bg) {
    double p = 1.0;
    for (uint32_t i = 0; i < w; i++) {
        const uint32_t k = std::min(i, bg.K);
        const uint32_t ctx = (y >> (2u * (w - 1u - i))) & (uint32_t)(ipow4(k + 1) - 1);   // the (k+1)-mer that ends at position i
        p *= (double)bg.v[bgoff(k) + ctx];
    }
    return p;
}

bool within_one(uint32_t a, uint32_t b, uint32_t w) {        // Hamming distance <= 1 between two w-mers
    uint32_t diff = 0;
    for (uint32_t x = a ^ b, i = 0; i < w; i++, x >>= 2) diff += (x & 3u) != 0u;
    return diff <= 1u;
}

}  // namespace

std::string kmer_string(uint32_t kmer, uint32_t w) {
    std::string s(w, 'A');
    for (uint32_t i = 0; i < w; i++) s[i] = "ACGT"[(kmer >> (2u * (w - 1u - i))) & 3u];
    return s;
}

void kmer_seeds(const uint64_t* counts, uint64_t n_windows, uint32_t w, const BgModel& bg, size_t max_seeds, bool ss,
                std::vector<KmerSeed>& out) {
    out.clear();
    const uint32_t cells = (uint32_t)ipow4(w);
    std::vector<double> p(cells), z(cells);
    for (uint32_t y = 0; y < cells; y++) p[y] = window_probability(y, w, bg);
    for (uint32_t y = 0; y < cells; y++) {
        const double e = ss ? (double)n_windows * p[y] : (double)n_windows * ((p[y] + p[revcomp(y, w)]) * 0.5);
        z[y] = e > 0.0 ? ((double)counts[y] - e) / std::sqrt(e) : 0.0;
    }
    std::vector<uint32_t> order(cells);
    for (uint32_t y = 0; y < cells; y++) order[y] = y;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return z[a] != z[b] ? z[a] > z[b] : a < b; });
    for (uint32_t y : order) {
        if (out.size() >= max_seeds || !(z[y] > 0.0)) break;
        const uint32_t rc = revcomp(y, w);
        bool near = false;
        for (const KmerSeed& s : out) near = near || within_one(y, s.kmer, w) || (!ss && within_one(rc, s.kmer, w));
        if (near) continue;
        KmerSeed s;
        s.kmer = y; s.count = counts[y]; s.z = z[y];
        s.pwm.assign(4 * (size_t)w, 0.f);
        // column j, base b: the counts of y and of its 3 w neighbours that carry b at j
        for (uint32_t j = 0; j < w; j++) {
            const uint32_t shift = 2u * (w - 1u - j), own = (y >> shift) & 3u;
            uint64_t n[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 4; b++)
                if (b != own) n[b] = counts[(y & ~(3u << shift)) | (b << shift)];
            n[own] = counts[y];
            for (uint32_t j2 = 0; j2 < w; j2++) {
                if (j2 == j) continue;
                const uint32_t sh2 = 2u * (w - 1u - j2), own2 = (y >> sh2) & 3u;
                for (uint32_t b = 0; b < 4; b++)
                    if (b != own2) n[own] += counts[(y & ~(3u << sh2)) | (b << sh2)];
            }
            const double total = (double)(n[0] + n[1] + n[2] + n[3]) + 4.0;
            for (uint32_t b = 0; b < 4; b++) s.pwm[b * w + j] = (float)(((double)n[b] + 1.0) / total);
        }
        out.push_back(std::move(s));
    }
}

int kmer_seeds_write(const std::string& path, uint32_t w, const std::vector<KmerSeed>& seeds, std::string& err) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { err = "Error: Cannot write the seed file: " + path; return 1; }
    fprintf(f, "MEME version 4\n\nALPHABET= ACGT\n\nBackground letter frequencies\nA 0.25 C 0.25 G 0.25 T 0.25\n");
    for (const KmerSeed& s : seeds) {
        // (nine significant digits bring every float back bit for bit)
        fprintf(f, "\nMOTIF %s count= %llu z= %.17g\n", kmer_string(s.kmer, w).c_str(), (unsigned long long)s.count, s.z);
        fprintf(f, "letter-probability matrix: alength= 4 w= %u nsites= %llu\n", w, (unsigned long long)s.count);
        for (uint32_t j = 0; j < w; j++)
            fprintf(f, "%.9g %.9g %.9g %.9g\n", s.pwm[0 * w + j], s.pwm[1 * w + j], s.pwm[2 * w + j], s.pwm[3 * w + j]);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { err = "Error: Cannot write the seed file: " + path; return 1; }
    return 0;
}

}  // namespace bammhost
