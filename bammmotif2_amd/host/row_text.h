// Text rows of the output files: the buffered writer, the parallel row formatter and the one window row that
// .positions, .occurrence and .logOddsZoops share.  Internal to the host library (host/fdr.cpp).
#pragma once
#include <omp.h>

#include <algorithm>
#include <charconv>
#include <initializer_list>

#include "bamm_host.h"
#include "host_util.h"

namespace bammhost {

// rows of floats exactly as `ostream << float` prints them (printf %g at the stream's precision),
// collected in memory and written once: the reference ends every row with std::endl, i.e. one
// write() per line, which at 2.2 M rows costs more than computing the statistics
struct alignas(128) RowWriter {                          // a line of its own: the string's length changes with every number, and the threads' writers sit side by side
    std::string buf;
    int precision;
    explicit RowWriter(int prec = 6) : precision(prec) { buf.reserve(1 << 20); }
    void num(float x) {
        char tmp[48];
        buf.append(tmp, format_g(tmp, x, precision));
    }
    void count(uint64_t x) {
        char tmp[24];
        buf.append(tmp, (size_t)(std::to_chars(tmp, tmp + sizeof tmp, x).ptr - tmp));
    }
    void text(const std::string& s) { buf.append(s); }
    void ch(char c) { buf.push_back(c); }
    void tab() { buf.push_back('\t'); }
    void nl() { buf.push_back('\n'); }
    void flush_to(std::ofstream& f) { f.write(buf.data(), (std::streamsize)buf.size()); buf.clear(); }
    void maybe_flush(std::ofstream& f) { if (buf.size() > (1 << 20) - 256) flush_to(f); }
};

// rows [0, n) formatted by row(w, i) on every granted core -- rounds of one chunk per thread, the chunks written in
// order: the same bytes as one writer walking all rows (formatting 11 M numbers is most of what the files cost), and
// the threads' buffers are reused from round to round (fresh pages are slow to come by in a container)
template <class Row>
void write_rows(std::ofstream& f, size_t n, int precision, Row&& row) {
    constexpr size_t kChunk = 16384;
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)host_parallelism(), n / kChunk + 1));
    std::vector<RowWriter> part((size_t)T, RowWriter(precision));
    for (size_t base = 0; base < n; base += kChunk * (size_t)T) {
#pragma omp parallel for schedule(static, 1) num_threads(T)
        for (int t = 0; t < T; t++) {
            RowWriter& w = part[(size_t)t];
            const size_t a = std::min(n, base + kChunk * (size_t)t), b = std::min(n, a + kChunk);
            for (size_t i = a; i < b; i++) row(w, i);
        }
        for (auto& w : part) w.flush_to(f);
    }
}

// One window of one sequence as text -- header, shown length, strand, start..end (1-based), the window's bases
// (EM.cpp:585-601, ScoreSeqSet.cpp:262-288, :293-331) -- and the file of such rows.  Sequence::getSequence() is the
// forward strand and, where both strands are stored (`revcomp`), an N and the reverse complement behind it; a code
// outside 1..4 prints N on either.  `halve`: the length column shows (L - 1) / 2 of the stored length L, and the strand
// sign is taken against that.  With revcomp == halve (.positions, .occurrence: both are !ss) the shown length is the
// forward length in either case; .logOddsZoops halves whenever --ss is absent, also for sampled negatives (one strand).
struct WindowRows {
    const std::vector<std::string>& headers;
    const uint8_t* codes;
    const uint64_t* off;
    uint32_t W;
    bool revcomp, halve;
    std::ofstream f;
    RowWriter w{3};                                          // p, e and the zoops score print at setprecision(3)
    // <dir>/<file>, headed by the window's columns and the writer's own `columns` behind them
    bool open(const std::string& dir, const std::string& file, const char* columns, std::string& err) {
        if (!open_output(f, dir + '/' + file, dir, err)) return false;
        w.text("seq\tlength\tstrand\tstart..end\tpattern"); w.text(columns); w.nl();
        return true;
    }
    size_t full_length(size_t n) const { const size_t L0 = off[n + 1] - off[n]; return revcomp ? 2 * L0 + 1 : L0; }
    // everything up to and including the pattern of window i of sequence n
    void prefix(RowWriter& out, size_t n, size_t i) const {
        static const char B[] = "NACGT";
        const size_t L0 = off[n + 1] - off[n], L = full_length(n), shown = halve ? (L - 1) / 2 : L;
        const uint8_t* c = codes + off[n];
        out.text(headers[n]); out.tab(); out.count(shown); out.tab(); out.ch(i < shown ? '+' : '-'); out.tab();
        out.count(i + 1); out.ch('.'); out.ch('.'); out.count(i + W); out.tab();
        for (size_t m = i; m < i + W; m++) {
            char b = 'N';                                    // the junction, and anything behind the stored strands
            if (m < L0) b = B[c[m] <= 4 ? c[m] : 0];
            else if (m > L0 && m < L) { const uint8_t x = c[2 * L0 - m]; b = (x >= 1 && x <= 4) ? B[5 - x] : 'N'; }
            out.ch(b);
        }
    }
    // one row of the file: the window, then the writer's own columns
    void row(size_t n, size_t i, std::initializer_list<float> columns = {}) {
        prefix(w, n, i);
        for (const float x : columns) { w.tab(); w.num(x); }
        w.nl(); w.maybe_flush(f);
    }
    int close() { w.flush_to(f); return 0; }
};

}  // namespace bammhost
