// Stand-alone check (own main, no GPU, no Python) of the two host rules every sequence set goes through:
//   * csrc/pack.cpp's packed sets: records of 15, 16, 17 and 33 positions through bamm_pack_kmers and
//     bamm_pack_codes (single strand), and an empty set -- word_off is the running sum of ceil(L / 16), the header agrees
//     with the lengths, min_len of the empty set is 0; every set is freed again;
//   * csrc/packed_set.h: the same lengths through packed_alloc + packed_set_lengths, in place as negs.cpp calls it;
//   * csrc/neg_layout.h: NegLayout against an enumeration of every negative index, lengths {1, 16, 17} x m_fold {1, 2, 7} x
//     keep_stride {0, 1, 2, 5, 40} (40 exceeds the total).
// Meant to run under the sanitizers (tests/test_host_cpu.py builds it so):
//   g++ -std=c++17 -fsanitize=address,undefined -static-libasan -static-libubsan -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/packed_layout_check.cpp bammmotif2_amd/csrc/pack.cpp
// Exit status 0 and no output: all is well; every mismatch is a line on stderr and exit status 1.
#include <cstdio>
#include <vector>

#include "../bammmotif2_amd/csrc/neg_layout.h"
#include "../bammmotif2_amd/csrc/packed_set.h"
#include "../include/bamm_em.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_bad++; fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static void check_header(const char* what, const bamm_packed* p, const std::vector<uint64_t>& lens) {
    uint64_t words = 0, total = 0, mx = 0, mn = lens.empty() ? 0 : UINT64_MAX;
    CHECK(p->n_seqs == lens.size(), "%s: n_seqs %llu", what, (unsigned long long)p->n_seqs);
    for (size_t n = 0; n < lens.size(); n++) {
        CHECK(p->len[n] == lens[n], "%s: len[%zu] = %u", what, n, p->len[n]);
        CHECK(p->word_off[n] == words, "%s: word_off[%zu] = %llu, want %llu", what, n, (unsigned long long)p->word_off[n], (unsigned long long)words);
        words += lens[n] / 16 + (lens[n] % 16 != 0);
        total += lens[n];
        if (lens[n] > mx) mx = lens[n];
        if (lens[n] < mn) mn = lens[n];
    }
    CHECK(p->word_off[lens.size()] == words && p->n_words == words, "%s: n_words %llu, want %llu", what, (unsigned long long)p->n_words, (unsigned long long)words);
    CHECK(p->total_len == total && p->max_len == mx && p->min_len == mn, "%s: total %llu max %u min %u", what, (unsigned long long)p->total_len, p->max_len, p->min_len);
    CHECK(p->exc_off[lens.size()] == p->n_exc, "%s: exc_off ends at %llu of %llu", what, (unsigned long long)p->exc_off[lens.size()], (unsigned long long)p->n_exc);
}

static void check_packing() {
    for (const std::vector<uint64_t>& lens : {std::vector<uint64_t>{15, 16, 17, 33}, std::vector<uint64_t>{}}) {
        std::vector<uint64_t> off{0}, kmer;
        std::vector<uint8_t> codes;
        for (uint64_t L : lens) {
            uint64_t roll = 0;
            for (uint64_t i = 0; i < L; i++) {
                const uint64_t base = (i + L) % 4;
                roll = ((roll << 2) | base) & ((1ull << 22) - 1);
                kmer.push_back(roll);
                codes.push_back((uint8_t)(base + 1));
            }
            off.push_back(kmer.size());
        }
        if (!codes.empty()) codes[off[2] + 3] = 0;           // one unknown base in the 17-position record: the exception arrays fill
        bamm_packed *a = nullptr, *b = nullptr;
        CHECK(bamm_pack_kmers(kmer.data(), off.data(), lens.size(), &a) == BAMM_OK && a, "bamm_pack_kmers: %s", bamm_last_error());
        CHECK(bamm_pack_codes(codes.data(), off.data(), lens.size(), 1, &b) == BAMM_OK && b, "bamm_pack_codes: %s", bamm_last_error());
        if (a) check_header("from kmers", a, lens);
        if (b) check_header("from codes", b, lens);
        if (a) CHECK(a->n_exc == 0, "from kmers: %llu exceptions", (unsigned long long)a->n_exc);
        bamm_packed_free(a);
        bamm_packed_free(b);
    }
}

static void check_packed_set() {
    for (const std::vector<uint64_t>& lens : {std::vector<uint64_t>{15, 16, 17, 33}, std::vector<uint64_t>{}}) {
        uint64_t words = 0;
        for (uint64_t L : lens) words += (L + 15) / 16;
        bamm::PackedPtr p;
        CHECK(bamm::packed_alloc(lens.size(), words, 0, &p) == BAMM_OK && p, "packed_alloc: %s", bamm_last_error());
        if (!p) continue;
        for (size_t n = 0; n < lens.size(); n++) p->len[n] = (uint32_t)lens[n];
        CHECK(bamm::packed_set_lengths(p.get(), p->len) == BAMM_OK, "packed_set_lengths: %s", bamm_last_error());
        check_header("packed_set.h", p.get(), lens);
    }
    bamm_packed head{};                                      // a bare header only counts; a length beyond 2^32 - 1 is refused
    head.n_seqs = 2;
    const uint64_t big[2] = {17, 1ull << 32};
    CHECK(bamm::packed_set_lengths(&head, big) == BAMM_ERR_ARG, "a length of 2^32 was accepted");
    head.n_seqs = 1;
    CHECK(bamm::packed_set_lengths(&head, big) == BAMM_OK && head.n_words == 2 && head.min_len == 17, "bare header: %llu words", (unsigned long long)head.n_words);
}

static void check_neg_layout() {
    const std::vector<uint64_t> lens{1, 16, 17};
    for (uint64_t m_fold : {1, 2, 7})
        for (uint64_t stride : {0, 1, 2, 5, 40}) {
            const bamm::NegLayout lay(lens.size(), [&](uint64_t i) { return lens[i]; }, m_fold, stride);
            // every negative index in the order the one stream serves them; the kept ones by stepping, not by the predicate
            const uint64_t total = lens.size() * m_fold;
            std::vector<char> keep(total, stride <= 1);
            if (stride > 1) for (uint64_t idx = 0; idx + stride <= total; idx += stride) keep[idx] = 1;
            uint64_t draw = 0, n_kept = 0;
            for (uint64_t idx = 0; idx < total; idx++) {
                const uint64_t i = idx / m_fold, f = idx % m_fold;
                if (f == 0) {
                    CHECK(lay.draw0[i] == draw, "m %llu stride %llu: draw0[%llu]", (unsigned long long)m_fold, (unsigned long long)stride, (unsigned long long)i);
                    CHECK(lay.first_kept[i] == n_kept, "m %llu stride %llu: first_kept[%llu]", (unsigned long long)m_fold, (unsigned long long)stride, (unsigned long long)i);
                }
                CHECK(lay.kept(i, f) == (bool)keep[idx], "m %llu stride %llu: kept(%llu)", (unsigned long long)m_fold, (unsigned long long)stride, (unsigned long long)idx);
                CHECK(bamm::neg_kept(idx, stride, total) == (bool)keep[idx], "m %llu stride %llu: neg_kept(%llu)", (unsigned long long)m_fold, (unsigned long long)stride, (unsigned long long)idx);
                draw += lens[i];
                n_kept += keep[idx];
                if (f + 1 == m_fold)
                    CHECK(lay.n_kept(i) == n_kept - lay.first_kept[i], "m %llu stride %llu: n_kept(%llu)", (unsigned long long)m_fold, (unsigned long long)stride, (unsigned long long)i);
            }
            CHECK(lay.draw0[lens.size()] == draw && lay.n_neg() == n_kept, "m %llu stride %llu: totals", (unsigned long long)m_fold, (unsigned long long)stride);
        }
}

int main() {
    check_packing();
    check_packed_set();
    check_neg_layout();
    return g_bad ? 1 : 0;
}
