// The positions-per-lane classes (kMClasses, common.h) as template arguments: what kernels.hip and scorer.hip instantiate
// their per-class kernels from.  Host-only; nothing here emits device code.
#pragma once
#include "common.h"

#include <type_traits>

#define BAMM_FOR_EACH_MCLASS(X) \
    X(0, 1, 1024) X(1, 2, 1024) X(2, 3, 1024) X(3, 4, 1024) X(4, 5, 1024) X(5, 6, 1024) X(6, 7, 1024) \
    X(7, 8, 1024) X(8, 10, 768) X(9, 12, 768) X(10, 14, 768) X(11, 16, 768) X(12, 20, 768)             \
    X(13, 24, 512) X(14, 28, 512) X(15, 32, 512) X(16, 40, 512) X(17, 48, 512) X(18, 56, 512) X(19, 64, 512) \
    X(20, 80, 256) X(21, 96, 256) X(22, 128, 256)

namespace bamm {
namespace {
// f(M, THREADS) with the class's values as std::integral_constant arguments
template <class F>
int with_mclass(int mclass, F&& f) {
    switch (mclass) {
#define X(idx, M, T) case idx: return f(std::integral_constant<int, M>(), std::integral_constant<int, T>());
        BAMM_FOR_EACH_MCLASS(X)
#undef X
        default: set_error("no kernel for M class %d", mclass); return BAMM_ERR_UNSUPPORTED;
    }
}
}  // namespace
}  // namespace bamm
