/*
 * wave_check.hip -- TEST-ONLY: the bodies of wave_bodies.h as gfx950 kernels, built with the product's HIPFLAGS (the
 * contraction and the code generation must be the step kernel's).  One workgroup of one wave per trial.
 *
 * extern "C" int wc_<name>(const double *in, double *out, int ntrial): host buffers of ntrial * nin * 64 and
 * ntrial * nout * 64 doubles (tests/wave_check.py checks the sizes against wc_shape); returns the first HIP error, 0 if none.
 * A body of WAVE_CHECK_AUX_BODIES takes two more arguments, (const void *aux, unsigned long aux_bytes): a read-only block every
 * trial of the call shares, uploaded once.
 * The emulator library exports the same functions (tests/emu/emu_kernels.cpp).
 */
#include "physics_kernel.h"
#include "wave_bodies.h"

#define WC_KERNEL(name, nin, nout)                                                                  \
    __global__ __launch_bounds__(64) void wc_kernel_##name(const double *in, double *out) {       \
        const size_t t = blockIdx.x;                                                              \
        wc::name(in + t * (nin) * 64, out + t * (nout) * 64);                                      \
    }
WAVE_CHECK_BODIES(WC_KERNEL)
#define WC_AUX_KERNEL(name, nin, nout)                                                                          \
    __global__ __launch_bounds__(64) void wc_kernel_##name(const double *in, double *out, const void *aux) {  \
        const size_t t = blockIdx.x;                                                                          \
        wc::name(in + t * (nin) * 64, out + t * (nout) * 64, aux);                                             \
    }
WAVE_CHECK_AUX_BODIES(WC_AUX_KERNEL)

/* kernel: (in, out) or, with an auxiliary block, (in, out, aux) */
template <class... AUX>
static int wc_launch(void (*kernel)(const double *, double *, AUX...), const double *in, double *out, int ntrial, int nin, int nout,
                     const void *aux = nullptr, size_t aux_bytes = 0) {
    static_assert(sizeof...(AUX) <= 1, "at most the auxiliary block");
    if (ntrial <= 0) return 0;
    if (sizeof...(AUX) == 1 && (!aux || aux_bytes == 0)) return (int)hipErrorInvalidValue;
    const size_t bin = (size_t)ntrial * nin * 64 * sizeof(double), bout = (size_t)ntrial * nout * 64 * sizeof(double);
    double *din = nullptr, *dout = nullptr;
    void *daux = nullptr;
    hipError_t e = hipMalloc((void **)&din, bin);
    if (e == hipSuccess) e = hipMalloc((void **)&dout, bout);
    if (e == hipSuccess && sizeof...(AUX) == 1) e = hipMalloc(&daux, aux_bytes);
    if (e == hipSuccess) e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
    if (e == hipSuccess && sizeof...(AUX) == 1) e = hipMemcpy(daux, aux, aux_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xff, bout); /* (NaN: an output a body does not write shows) */
    if (e == hipSuccess) {
        if constexpr (sizeof...(AUX) == 1) hipLaunchKernelGGL(kernel, dim3((unsigned)ntrial), dim3(64), 0, 0, (const double *)din, dout, (const void *)daux);
        else hipLaunchKernelGGL(kernel, dim3((unsigned)ntrial), dim3(64), 0, 0, (const double *)din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (daux) (void)hipFree(daux);
    return (int)e;
}

#define WC_LAUNCHER(name, nin, nout) \
    extern "C" int wc_##name(const double *in, double *out, int ntrial) { return wc_launch(wc_kernel_##name, in, out, ntrial, nin, nout); }
WAVE_CHECK_BODIES(WC_LAUNCHER)
/* an auxiliary block smaller than the body's own struct is refused, not read past its end */
#define WC_AUX_LAUNCHER(name, nin, nout)                                                                                  \
    extern "C" int wc_##name(const double *in, double *out, int ntrial, const void *aux, unsigned long aux_bytes) {      \
        if (aux_bytes < sizeof(wc::FactorAux)) return (int)hipErrorInvalidValue;                                         \
        return wc_launch(wc_kernel_##name, in, out, ntrial, nin, nout, aux, aux_bytes);                                   \
    }
WAVE_CHECK_AUX_BODIES(WC_AUX_LAUNCHER)
