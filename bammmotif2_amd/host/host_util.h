// Small helpers every unit of the host library spells the same way: table offsets, sequence offsets, output files.
#pragma once
#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/bamm_em.h"

namespace bammhost {

inline size_t ipow4(size_t e) { return size_t(1) << (2 * e); }
inline size_t bgoff(size_t k) { return (ipow4(k + 1) - 4) / 3; }           // order k's first cell in a flat [k][y] table
inline size_t voff(size_t k, size_t W) { return W * bgoff(k); }             // ... in a flat [k][y][j] table

// where every sequence of a packed set starts, [n_seqs + 1]
inline std::vector<uint64_t> offsets_of(const bamm_packed* p) {
    std::vector<uint64_t> off(p->n_seqs + 1, 0);
    for (uint64_t n = 0; n < p->n_seqs; n++) off[n + 1] = off[n] + p->len[n];
    return off;
}

// an output file of `dir`; false with the reference's message in `err`
inline bool open_output(std::ofstream& f, const std::string& path, const std::string& dir, std::string& err) {
    f.open(path);
    if (!f.is_open()) err = "Error: Cannot write into output directory: " + dir;
    return f.is_open();
}

}  // namespace bammhost
