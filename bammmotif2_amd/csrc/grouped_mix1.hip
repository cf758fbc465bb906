// Mixed-row kernel (mixed_kernel.h) with ONE wide group (W mod 3 == 1, e.g. W = 19 = 3+3+3+3+3+4).
#include "mixed_kernel.h"

namespace bamm {

int launch_em_mix1(int mclass, bool accum, bool write_r, const GrpKernelArgs& a, uint32_t blocks, uint32_t threads, hipStream_t st) {
    return launch_mix<1>(mclass, accum, write_r, a, blocks, threads, st);
}

}  // namespace bamm
