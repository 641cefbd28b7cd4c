/*
 * step_launch.h -- how phys_batch.hip launches an instantiation of the step kernel: launch_step<...> launches
 * cassie_step_kernel<...> with a workgroup of NW wavefronts.  Only declared here; step_kernels.h defines it, and each
 * kernels_*.hip instantiates it explicitly for one model family's forms, so that the instantiations compile side by side (each
 * takes about a minute of hipcc time).  An instantiation that phys_batch.hip names and no kernels_*.hip provides fails the link.
 */
#ifndef CASSIE_STEP_LAUNCH_H
#define CASSIE_STEP_LAUNCH_H

#include <hip/hip_runtime.h>

#include "step_plan.h"

namespace ck {
using StepLauncher = void (*)(unsigned grid, hipStream_t s, const PhysIO &io);

template <int NVP, class TOPO, int FEAT = FEAT_ALL, int MAXR = MID_ROWS, int NW = 1, bool WALK = false, int WPS = NW, int INROWS = 0, int SERVE = FEAT_FULL>
void launch_step(unsigned grid, hipStream_t s, const PhysIO &io);
}  // namespace ck
#endif
