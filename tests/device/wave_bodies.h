/*
 * wave_bodies.h -- TEST-ONLY bodies that exercise the wavefront primitives (wave.h) and the kernel's small numerical
 * helpers (pk_math.h, pk_factor_solve.h) one at a time, written against wv:: and ck:: exactly as the step kernel is.
 *
 * The same source is compiled twice: for gfx950 with the product's flags (wave_check.hip: one workgroup of one wave per
 * trial) and into the CPU wave emulator (tests/emu/emu_runtime.cpp: the body runs through the emulator's rendezvous
 * scheduler).  tests/wave_check.py loads either and tests/test_wave_primitives.py compares both with exact references.
 *
 * A body gets its trial's slice of the buffers: input k of lane l is in[64 k + l], output k of lane l is out[64 k + l].
 * WAVE_CHECK_BODIES lists every body as X(name, inputs per lane, outputs per lane).
 */
#ifndef CASSIE_WAVE_BODIES_H
#define CASSIE_WAVE_BODIES_H

#include <cstring>

#define WAVE_CHECK_BODIES(X) \
    X(wave_sum, 1, 1)        \
    X(wave_sum_f32, 1, 1)    \
    X(dpp_take, 2, 12)       \
    X(readlane, 2, 1)        \
    X(writelane, 3, 4)       \
    X(from_upper_half, 1, 1) \
    X(shfl, 3, 8)            \
    X(ballot, 1, 3)          \
    X(mfma1, 6, 4)           \
    X(mfma4, 12, 4)          \
    X(max_raw, 2, 1)         \
    X(estimates, 1, 2)       \
    X(fast_rcp, 1, 1)        \
    X(normalize4_fast, 4, 4) \
    X(normalize3_fast, 3, 4) \
    X(sincos, 1, 4)

namespace wc {

/* the wave-uniform sum, stored by every lane */
WV_DEVICE void wave_sum(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::wave_sum(in[l]);
}
/* ... in single precision (inputs and result are floats carried in doubles, which is exact) */
WV_DEVICE void wave_sum_f32(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = (double)wv::wave_sum_f32((float)in[l]);
}
/* each DPP move of the two sums, with the row mask the sum gives it: the doubles of input 0, then the floats of input 1 */
WV_DEVICE void dpp_take(const double *in, double *out) {
    const int l = wv::lane();
    const double v = in[l];
    const float f = (float)in[64 + l];
    out[0 * 64 + l] = wv::dpp_take<0xB1, 0xf>(v);
    out[1 * 64 + l] = wv::dpp_take<0x4E, 0xf>(v);
    out[2 * 64 + l] = wv::dpp_take<0x141, 0xf>(v);
    out[3 * 64 + l] = wv::dpp_take<0x140, 0xf>(v);
    out[4 * 64 + l] = wv::dpp_take<0x142, 0xa>(v);
    out[5 * 64 + l] = wv::dpp_take<0x143, 0xc>(v);
    out[6 * 64 + l] = (double)wv::dpp_take_f32<0xB1, 0xf>(f);
    out[7 * 64 + l] = (double)wv::dpp_take_f32<0x4E, 0xf>(f);
    out[8 * 64 + l] = (double)wv::dpp_take_f32<0x141, 0xf>(f);
    out[9 * 64 + l] = (double)wv::dpp_take_f32<0x140, 0xf>(f);
    out[10 * 64 + l] = (double)wv::dpp_take_f32<0x142, 0xa>(f);
    out[11 * 64 + l] = (double)wv::dpp_take_f32<0x143, 0xc>(f);
}
/* broadcast of lane src; src is read from memory (every lane holds the same value), so it is wave-uniform at run time
 * but no compile-time constant (the compiler takes it from the first lane: v_readfirstlane, then v_readlane) */
WV_DEVICE void readlane(const double *in, double *out) {
    const int l = wv::lane();
    const int src = (int)in[64 + l];
    out[l] = wv::readlane(in[l], src);
}
/* writelane into a value the instruction just before it wrote (v = x + y); s is wave-uniform (every lane holds it) */
WV_DEVICE void writelane(const double *in, double *out) {
    const int l = wv::lane();
    const double s = in[128 + l];
    const double v = in[l] + in[64 + l];
    out[0 * 64 + l] = wv::writelane<0>(v, s);
    out[1 * 64 + l] = wv::writelane<31>(v, s);
    out[2 * 64 + l] = wv::writelane<32>(v, s);
    out[3 * 64 + l] = wv::writelane<63>(v, s);
}
WV_DEVICE void from_upper_half(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::from_upper_half(in[l]);
}
/* shfl from a per-lane source (input 1), its integer form on input 2, shfl_xor with the masks 1 .. 32 */
WV_DEVICE void shfl(const double *in, double *out) {
    const int l = wv::lane();
    const double v = in[l];
    const int src = (int)in[64 + l];
    out[0 * 64 + l] = wv::shfl(v, src);
    out[1 * 64 + l] = (double)wv::shfl_i((int)in[128 + l], src);
    out[2 * 64 + l] = wv::shfl_xor(v, 1);
    out[3 * 64 + l] = wv::shfl_xor(v, 2);
    out[4 * 64 + l] = wv::shfl_xor(v, 4);
    out[5 * 64 + l] = wv::shfl_xor(v, 8);
    out[6 * 64 + l] = wv::shfl_xor(v, 16);
    out[7 * 64 + l] = wv::shfl_xor(v, 32);
}
/* ballot of (input != 0): the mask's two halves and popc64 of it */
WV_DEVICE void ballot(const double *in, double *out) {
    const int l = wv::lane();
    const unsigned long long m = wv::ballot(in[l] != 0.0);
    out[0 * 64 + l] = (double)(unsigned)(m & 0xffffffffull);
    out[1 * 64 + l] = (double)(unsigned)(m >> 32);
    out[2 * 64 + l] = (double)wv::popc64(m);
}
/* one matrix-core instruction: inputs a, b, c[0 .. 3] */
WV_DEVICE void mfma1(const double *in, double *out) {
    const int l = wv::lane();
    wv::mfma_acc acc;
    for (int v = 0; v < 4; ++v) acc.c[v] = in[(2 + v) * 64 + l];
    wv::mfma_f64_16x16x4(in[l], in[64 + l], acc);
    for (int v = 0; v < 4; ++v) out[v * 64 + l] = acc.c[v];
}
/* four dependent instructions on one accumulator: inputs a[0 .. 3], b[0 .. 3], c[0 .. 3] */
WV_DEVICE void mfma4(const double *in, double *out) {
    const int l = wv::lane();
    wv::mfma_acc acc;
    for (int v = 0; v < 4; ++v) acc.c[v] = in[(8 + v) * 64 + l];
    for (int s = 0; s < 4; ++s) wv::mfma_f64_16x16x4(in[s * 64 + l], in[(4 + s) * 64 + l], acc);
    for (int v = 0; v < 4; ++v) out[v * 64 + l] = acc.c[v];
}
WV_DEVICE void max_raw(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::max_raw(in[l], in[64 + l]);
}
/* the hardware seeds fast_rcp and the normalisations start from */
WV_DEVICE void estimates(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::rcp_estimate(in[l]);
    out[64 + l] = wv::rsq_estimate(in[l]);
}
WV_DEVICE void fast_rcp(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = ck::fast_rcp(in[l]);
}
WV_DEVICE void normalize4_fast(const double *in, double *out) {
    const int l = wv::lane();
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = in[i * 64 + l];
    ck::normalize4_fast(q);
    for (int i = 0; i < 4; ++i) out[i * 64 + l] = q[i];
}
/* the unit vector, then the returned norm */
WV_DEVICE void normalize3_fast(const double *in, double *out) {
    const int l = wv::lane();
    double a[3];
    for (int i = 0; i < 3; ++i) a[i] = in[i * 64 + l];
    const double n = ck::normalize3_fast(a);
    for (int i = 0; i < 3; ++i) out[i * 64 + l] = a[i];
    out[3 * 64 + l] = n;
}
/* sincos_reduced, then sincos_bounded: the kernel's choice, which takes the library's sincos for the whole wave as soon
 * as one lane is at or beyond 2^19 */
WV_DEVICE void sincos(const double *in, double *out) {
    const int l = wv::lane();
    double s, c;
    ck::sincos_reduced(in[l], s, c);
    out[0 * 64 + l] = s;
    out[1 * 64 + l] = c;
    ck::sincos_bounded(in[l], s, c);
    out[2 * 64 + l] = s;
    out[3 * 64 + l] = c;
}

}  // namespace wc

/* (host) inputs and outputs per lane of a body; -1 for a name that is not one */
extern "C" int wc_shape(const char *name, int *nin, int *nout) {
#define WC_SHAPE(n, i, o) if (!strcmp(name, #n)) { *nin = i; *nout = o; return 0; }
    WAVE_CHECK_BODIES(WC_SHAPE)
#undef WC_SHAPE
    return -1;
}
#endif
