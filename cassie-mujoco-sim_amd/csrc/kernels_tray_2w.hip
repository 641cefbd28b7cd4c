/* cassie_tray_box.xml (BASELINE config 5), the fast instantiation (47 rows) in the two-wave form: two wavefronts per env, wave 1
 * running the mass-matrix stage group, the drive-level pass, the factorisations, the bias / passive stage and the stages behind
 * the solve beside wave 0's collision (box-box by the whole wave), velocity, constraint-row and solve stages (physics_kernel.h)
 * (a LEAN form, pk_stages.h, by half: without FEAT_PROF, WITH FEAT_READOUT.  The launcher never starts it with the read-out block or as
 * a forward pass either -- step_policy.h -- but without that code the register allocator of this 40-dof, 256-register kernel falls off
 * its cliff: 468 spilled vector registers and 1 388 B of scratch against 100 / 204 B with everything in and 55 / 180 B as shipped,
 * profiles/round7/lean_forms_resources.txt) */
#include "step_kernels.h"
namespace ck {
template void launch_step<40, TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2, false, 2, 0, FEAT_READOUT>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
