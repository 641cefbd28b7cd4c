/* plain cassie.xml, the 63-row instantiation in its two-wave form as the pass behind the two-wave fast kernel (step_plan.h): it
 * walks the list of envs the fast kernel handed over and hands on what needs more than 63 rows / 16 contacts.  There a workgroup
 * must be placeable wherever a fast kernel's is -- two waves of 256 registers, 40 KB of LDS -- or it waits for a SIMD to empty
 * while the other env range's kernel keeps every SIMD half full */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, MID_ROWS, 2, true>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
