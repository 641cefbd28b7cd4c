/* plain cassie.xml: the two-wave fast instantiation WITH the step-sums block (FEAT_SUMS, pk_stages.h) -- what a stepping launch takes
 * while the batch accumulates (phys_batch_step_sums_enable; step_policy.h: launch_forms, phys_batch.hip: the FEAT_SUMS table), so that
 * the lean form the benchmark runs carries none of that code.  The one-wave fast form has no such sibling: an accumulating launch of
 * a batch set to one wave per env takes the 63-row form alone (launch_forms) */
#include "step_kernels.h"
namespace ck {
template void launch_step<32, TopoCassie32, 0, FAST_ROWS, 2, false, 2, 0, FEAT_SUMS>(unsigned, hipStream_t, const PhysIO &);
}  // namespace ck
