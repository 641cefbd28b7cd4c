/* cassie_hfield.xml: the fast instantiations WITH the stage stamps (FEAT_PROF; FORM_FAST_PROF / FORM_FAST_2W_PROF, step_plan.h) -- what a
 * stepping launch takes while the batch's profile buffer is on (step_policy.h: launch_forms), so that tools/stage_profile.py measures
 * the fast code and the forms the benchmark runs carry no stamp */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 1, false, 1, 0, FEAT_PROF>(unsigned, hipStream_t, const PhysIO &);
template void launch_step<32, TopoCassie32, FEAT_HFIELD, FAST_ROWS, 2, false, 2, 0, FEAT_PROF>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
