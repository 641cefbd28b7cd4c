/*
 * logn.h -- the defined natural logarithm the draw rows' Box-Muller radius reads (draw_kernels.h): logn, as include/cassie_phys.h
 * defines it step by step, beside expn.h's exponential and with its two constants.  Written with the wv:: primitives only; the wave
 * emulator compiles the same text.  No fused operation, no library call: the split of x is integer arithmetic on its bits.
 */
#ifndef CASSIE_LOGN_H
#define CASSIE_LOGN_H

#include <cmath>

namespace ck {

/* logn(x) ~ ln x for a finite x > 0, as cassie_phys.h defines it step by step.  x = m 2^e with m in [sqrt 1/2, sqrt 2): the exponent and
 * the mantissa are taken from the bits, a subnormal x after the exact product with 2^54, and an m >= the double nearest sqrt 2 is halved
 * (exact) with e + 1.  f = m - 1 is exact (Sterbenz).  s = f / (2 + f), z = s s, P = Horner in z on the doubles nearest 1/23, 1/21, ...,
 * 1/3; t = s + (s z) P; r = 2 t (exact); the result is e ln2_hi + (e ln2_lo + r): e ln2_hi is exact (ln2_hi ends in 21 zero bits and
 * |e| <= 1075).  |s| <= 0.1716, so what the polynomial leaves out is below 2^-65 of t.  At x = 1: f = s = 0 and the result is +0.0.
 * By selects, before anything else is looked at: a NaN gives that NaN; x < 0 (-inf included) gives NaN; +-0.0 gives -inf; +inf gives +inf.
 * (tests/test_draw.py measures the error.) */
WV_DEVICE double logn(double x) {
    using namespace wv;
    if (x != x) return x;
    if (x < 0.0) return NAN;
    if (x == 0.0) return -HUGE_VAL;
    if (x == HUGE_VAL) return x;
    const bool tiny = x < 2.2250738585072014e-308;                           /* below 2^-1022 */
    const double y = tiny ? mul_rn(x, 18014398509481984.0) : x;              /* 2^54: exact */
    unsigned long long bits;
    __builtin_memcpy(&bits, &y, sizeof bits);
    int e = (int)((bits >> 52) & 0x7ffull) - 1023 - (tiny ? 54 : 0);
    bits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    __builtin_memcpy(&m, &bits, sizeof m);                                   /* in [1, 2) */
    const bool upper = m >= 1.4142135623730951;
    m = upper ? mul_rn(m, 0.5) : m;
    e += upper ? 1 : 0;
    const double f = sub_rn(m, 1.0);
    const double s = div_rn(f, add_rn(2.0, f));
    const double z = mul_rn(s, s);
    double p = 0.043478260869565216;                        /* 1/23 ... 1/3, each the nearest double */
    p = add_rn(0.047619047619047616, mul_rn(z, p));
    p = add_rn(0.05263157894736842, mul_rn(z, p));
    p = add_rn(0.058823529411764705, mul_rn(z, p));
    p = add_rn(0.06666666666666667, mul_rn(z, p));
    p = add_rn(0.07692307692307693, mul_rn(z, p));
    p = add_rn(0.09090909090909091, mul_rn(z, p));
    p = add_rn(0.1111111111111111, mul_rn(z, p));
    p = add_rn(0.14285714285714285, mul_rn(z, p));
    p = add_rn(0.2, mul_rn(z, p));
    p = add_rn(0.3333333333333333, mul_rn(z, p));
    const double t = add_rn(s, mul_rn(mul_rn(s, z), p));
    const double r = mul_rn(2.0, t);
    const double ed = (double)e;
    return add_rn(mul_rn(ed, 6.93147180369123816490e-01), add_rn(mul_rn(ed, 1.90821492927058770002e-10), r));
}

}  // namespace ck
#endif
