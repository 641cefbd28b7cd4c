/*
 * step_kernels.h -- the definition of ck::launch_step (step_launch.h), for the kernels_*.hip translation units alone: each of them
 * instantiates it explicitly for the forms of one model family (phys_batch.hip: the tables that name them).
 */
#ifndef CASSIE_STEP_KERNELS_H
#define CASSIE_STEP_KERNELS_H

#include "step_launch.h"

namespace ck {
template <int NVP, class TOPO, int FEAT, int MAXR, int NW, bool WALK, int WPS, int INROWS, int SERVE>
void launch_step(unsigned grid, hipStream_t s, const PhysIO &io) {
    hipLaunchKernelGGL((cassie_step_kernel<NVP, TOPO, FEAT, MAXR, NW, WALK, WPS, INROWS, SERVE>), dim3(grid), dim3(NW * WV_WAVE), 0, s, io);
}
}  // namespace ck
#endif
