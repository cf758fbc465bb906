// Mixed-row kernel (mixed_kernel.h) with TWO wide groups (W mod 3 == 2, e.g. W = 20 = 3+3+3+3+4+4): the
// instantiations for 4..10 positions per lane.  A translation unit of its own: it compiles next to the others.
#include "mixed_kernel.h"

namespace bamm {

int launch_em_mix(int mclass, bool accum, bool write_r, const GrpKernelArgs& a, uint32_t blocks, uint32_t threads, hipStream_t st) {
    return launch_mix<2>(mclass, accum, write_r, a, blocks, threads, st);
}

}  // namespace bamm

#ifdef BAMM_PHASE_CLOCK
// debug builds only: the phase clocks of the last k_em_mix launch of this translation unit ([256 blocks][16], 100 MHz ticks)
extern "C" int bamm_debug_phase_clock(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bamm::g_phase_clock), 256 * 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
#endif
