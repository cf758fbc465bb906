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

std::string kmer_string(uint32_t kmer, uint32_t w, uint32_t gap) {
    const std::string all = kmer_string(kmer, w);
    return gap ? all.substr(0, w / 2) + std::string(gap, 'n') + all.substr(w / 2) : all;
}

void kmer_seeds_gapped(const uint64_t* counts, const uint64_t* n_windows, uint32_t w, uint32_t gap_lo, uint32_t gap_hi,
                       const BgModel& bg, size_t max_seeds, bool ss, std::vector<KmerSeed>& out) {
    out.clear();
    const uint32_t cells = (uint32_t)ipow4(w), h = w / 2u, n_gaps = gap_hi - gap_lo + 1u, half_mask = (uint32_t)ipow4(h) - 1u;
    // P(y): the contiguous window's at gap 0; across a gap the halves are independent h-mers, the right one starting at order 0 again
    std::vector<double> p0, pg;
    if (gap_lo == 0) {
        p0.resize(cells);
        for (uint32_t y = 0; y < cells; y++) p0[y] = window_probability(y, w, bg);
    }
    if (gap_hi > 0) {
        std::vector<double> ph(ipow4(h));
        for (uint32_t x = 0; x <= half_mask; x++) ph[x] = window_probability(x, h, bg);
        pg.resize(cells);
        for (uint32_t y = 0; y < cells; y++) pg[y] = ph[y >> (2u * h)] * ph[y & half_mask];
    }
    std::vector<double> z((size_t)n_gaps * cells);
    for (uint32_t g = gap_lo; g <= gap_hi; g++) {
        const std::vector<double>& p = g ? pg : p0;
        const uint64_t* c = counts + (size_t)(g - gap_lo) * cells;
        const double nw = (double)n_windows[g - gap_lo];
        for (uint32_t y = 0; y < cells; y++) {
            const double e = ss ? nw * p[y] : nw * ((p[y] + p[revcomp(y, w)]) * 0.5);
            z[(size_t)(g - gap_lo) * cells + y] = e > 0.0 ? ((double)c[y] - e) / std::sqrt(e) : 0.0;
        }
    }
    // candidate i = (gap - gap_lo) * cells + cell: ascending i is the smaller gap, then the smaller cell
    std::vector<uint32_t> order((size_t)n_gaps * cells);
    for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return z[a] != z[b] ? z[a] > z[b] : a < b; });
    auto shares_half = [&](uint32_t a, uint32_t b) { return (a >> (2u * h)) == (b >> (2u * h)) || (a & half_mask) == (b & half_mask); };
    for (uint32_t i : order) {
        if (out.size() >= max_seeds || !(z[i] > 0.0)) break;
        const uint32_t g = gap_lo + i / cells, y = i % cells, rc = revcomp(y, w);
        const uint64_t* c = counts + (size_t)(g - gap_lo) * cells;
        bool near = false;
        for (const KmerSeed& s : out) {
            if (s.gap == g) near = near || within_one(y, s.kmer, w) || (!ss && within_one(rc, s.kmer, w));
            else near = near || shares_half(y, s.kmer) || (!ss && shares_half(rc, s.kmer));   // the shifted copies a dyad leaves at the neighbouring gaps
        }
        if (near) continue;
        KmerSeed s;
        s.kmer = y; s.gap = g; s.count = c[y]; s.z = z[i];
        const uint32_t width = w + g;
        s.pwm.assign(4 * (size_t)width, 0.25f);               // (the gap's columns stay at 0.25)
        // informative column j, base b: the counts of y and of its 3 w neighbours in this gap's table that carry b at j
        for (uint32_t j = 0; j < w; j++) {
            const uint32_t shift = 2u * (w - 1u - j), own = (y >> shift) & 3u, col = j < h ? j : j + g;
            uint64_t n[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 4; b++)
                if (b != own) n[b] = c[(y & ~(3u << shift)) | (b << shift)];
            n[own] = c[y];
            for (uint32_t j2 = 0; j2 < w; j2++) {
                if (j2 == j) continue;
                const uint32_t sh2 = 2u * (w - 1u - j2), own2 = (y >> sh2) & 3u;
                for (uint32_t b = 0; b < 4; b++)
                    if (b != own2) n[own] += c[(y & ~(3u << sh2)) | (b << sh2)];
            }
            const double total = (double)(n[0] + n[1] + n[2] + n[3]) + 4.0;
            for (uint32_t b = 0; b < 4; b++) s.pwm[b * width + col] = (float)(((double)n[b] + 1.0) / total);
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
        const uint32_t width = w + s.gap;                     // (a dyad's PWM spans its gap)
        fprintf(f, "\nMOTIF %s count= %llu z= %.17g", kmer_string(s.kmer, w, s.gap).c_str(), (unsigned long long)s.count, s.z);
        if (s.gap) fprintf(f, " gap= %u", s.gap);
        fprintf(f, "\nletter-probability matrix: alength= 4 w= %u nsites= %llu\n", width, (unsigned long long)s.count);
        for (uint32_t j = 0; j < width; j++)
            fprintf(f, "%.9g %.9g %.9g %.9g\n", s.pwm[0 * width + j], s.pwm[1 * width + j], s.pwm[2 * width + j], s.pwm[3 * width + j]);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { err = "Error: Cannot write the seed file: " + path; return 1; }
    return 0;
}

}  // namespace bammhost
