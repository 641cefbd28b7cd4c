/*
 * expn.h -- the defined exponential the reward's EXP shape (reward_kernels.h) and the policy's activations (policy_kernels.h) share:
 * reward_expn, as include/cassie_phys.h defines it step by step.  Written with the wv:: primitives only; the wave emulator compiles the
 * same text.  (Moved here from reward_kernels.h without changing a bit of it.)
 */
#ifndef CASSIE_EXPN_H
#define CASSIE_EXPN_H

#include <cmath>

namespace ck {

/* expn(a) ~ exp(-a) for the a = k s of a shape, as cassie_phys.h defines it step by step: NaN -> NaN; a > 708 -> +0.0 (a < -708 -> +inf);
 * n = rint(a log2 e); rho = (a - n ln2_hi) - n ln2_lo (n ln2_hi is exact: ln2_hi ends in 21 zero bits and |n| <= 1022); p = the degree-13
 * Taylor polynomial of exp in -rho by Horner, one multiply and one add a step; p 2^-n, exact: 0.7 < p < 1.42 and the result is normal */
WV_DEVICE double reward_expn(double a) {
    using namespace wv;
    if (a != a) return a;
    if (a > 708.0) return 0.0;
    if (a < -708.0) return HUGE_VAL;
    const double nd = rint(mul_rn(a, 1.44269504088896338700e+00));
    const double x = -sub_rn(sub_rn(a, mul_rn(nd, 6.93147180369123816490e-01)), mul_rn(nd, 1.90821492927058770002e-10));   /* -rho */
    double p = 1.6059043836821613e-10;                       /* 1/13! ... 1/0!, each the nearest double */
    p = add_rn(mul_rn(p, x), 2.08767569878681e-09);
    p = add_rn(mul_rn(p, x), 2.505210838544172e-08);
    p = add_rn(mul_rn(p, x), 2.755731922398589e-07);
    p = add_rn(mul_rn(p, x), 2.7557319223985893e-06);
    p = add_rn(mul_rn(p, x), 2.48015873015873e-05);
    p = add_rn(mul_rn(p, x), 0.0001984126984126984);
    p = add_rn(mul_rn(p, x), 0.001388888888888889);
    p = add_rn(mul_rn(p, x), 0.008333333333333333);
    p = add_rn(mul_rn(p, x), 0.041666666666666664);
    p = add_rn(mul_rn(p, x), 0.16666666666666666);
    p = add_rn(mul_rn(p, x), 0.5);
    p = add_rn(mul_rn(p, x), 1.0);
    p = add_rn(mul_rn(p, x), 1.0);
    return ldexp(p, -(int)nd);
}

}  // namespace ck
#endif
