// lsc_device_mem.hpp -- owners of the host layer's HBM and pinned host allocations.  Host side only; the one place of the product that
// calls the runtime's allocation and free functions.  An owner is move-only and frees in its destructor, so a struct of owners is
// released -- and left "nothing allocated" -- by assigning it a fresh value (lsc_abi.cpp groups them by lifetime that way).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace lsc {

struct HbmMem {
    static hipError_t allocate(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t allocate(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void release(void *p) { (void)hipHostFree(p); }
};

// n elements of T.  alloc / alloc_zero / upload free what was held first; a failed allocation leaves the owner empty.
template <class T, class Mem = HbmMem>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset()
    {
        if (p_) Mem::release(p_);
        p_ = nullptr; n_ = 0;
    }
    hipError_t alloc(size_t n)
    {
        reset();
        void *p = nullptr;
        const hipError_t e = Mem::allocate(&p, sizeof(T) * n);
        if (e == hipSuccess) { p_ = static_cast<T *>(p); n_ = n; }
        return e;
    }
    hipError_t alloc_zero(size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(p_, 0, sizeof(T) * n);
    }
    hipError_t upload(const T *src, size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice);
    }

    T *get() const { return p_; }
    operator T *() const { return p_; }       // (so that the argument blocks of the launches are filled as from plain pointers;
                                              //  next to a nullptr in a ?: write get(): not every compiler finds the common type)
    explicit operator bool() const { return p_ != nullptr; }
    size_t size() const { return n_; }        // elements

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <class T>
using PinnedBuf = DevBuf<T, PinnedMem>;       // staging buffers of the host-buffer ticks: alloc / reset / get only

}  // namespace lsc
