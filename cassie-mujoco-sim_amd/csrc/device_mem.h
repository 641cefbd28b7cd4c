/*
 * device_mem.h -- who owns the batch's memory (private to phys_batch.hip, which defines hip_ok): DevBuf<T>, a buffer in HBM the
 * batch allocated or one of the caller's it was bound to, and HostWords, pinned host words the device writes.  Both release what
 * they own when they go out of scope or are assigned over; a failing release is reported (last error + stderr), never dropped.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

static bool hip_ok(hipError_t e, const char *what);

template <class T>
class DevBuf {
    T *p_ = nullptr;
    bool owned_ = false;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), owned_(o.owned_) { o.p_ = nullptr; o.owned_ = false; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; owned_ = o.owned_; o.p_ = nullptr; o.owned_ = false; }
        return *this;
    }
    ~DevBuf() { reset(); }
    /* releases what it holds, then count elements of the batch's own, zeroed on request (blocking); on failure it holds nothing.
     * Errors read "hipMalloc(<what>)" / "hipMemset(<what>)". */
    bool alloc(size_t count, bool zero, const char *what) {
        reset();
        const size_t bytes = sizeof(T) * count;
        if (!hip_ok(hipMalloc((void **)&p_, bytes), (std::string("hipMalloc(") + what + ")").c_str())) { p_ = nullptr; return false; }
        owned_ = true;
        if (zero && !hip_ok(hipMemset((void *)p_, 0, bytes), (std::string("hipMemset(") + what + ")").c_str())) { reset(); return false; }
        return true;
    }
    /* releases what it holds, then stands for the caller's buffer, which it never frees */
    void borrow(T *p) { reset(); p_ = p; }
    /* (hipFree waits for the device by itself: launches already queued may still use the buffer) */
    void reset() {
        if (owned_ && p_) (void)hip_ok(hipFree((void *)p_), "hipFree");
        p_ = nullptr; owned_ = false;
    }
    T *get() const { return p_; }
    bool owned() const { return owned_; }
    operator T *() const { return p_; }
};

/* count ints of pinned host memory, zeroed and mapped into the device's address space: the host reads what kernels write there */
class HostWords {
    int *h_ = nullptr, *d_ = nullptr;
public:
    HostWords() = default;
    HostWords(const HostWords &) = delete;
    HostWords &operator=(const HostWords &) = delete;
    ~HostWords() { if (h_) (void)hip_ok(hipHostFree(h_), "hipHostFree"); }
    bool alloc(size_t count, const char *what) {
        if (!hip_ok(hipHostMalloc((void **)&h_, sizeof(int) * count, hipHostMallocMapped), (std::string("hipHostMalloc(") + what + ")").c_str())) { h_ = nullptr; return false; }
        memset(h_, 0, sizeof(int) * count);
        return hip_ok(hipHostGetDevicePointer((void **)&d_, h_, 0), "hipHostGetDevicePointer");
    }
    int *host() const { return h_; }
    int *dev() const { return d_; }
};
