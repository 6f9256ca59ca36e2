// almpc_devbuf.h -- the one owner of device and pinned host memory of libalmpc.so (host code only).
//
// Every hipMalloc / hipHostMalloc / hipFree / hipHostFree of the library is in this file.  A DevBuf is move-only and frees in its
// destructor, so a buffer is named once (its member or local) and an early return cannot leak it.  It converts to T* and to nothing
// else: kernel arguments, Params fields, `buf + off` and `if (!buf)` read it like the raw pointer it replaces (.get() where a ternary
// or a template deduction needs the pointer type spelled out).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace almpc {

enum class Mem {
    Device,        // hipMalloc of count * sizeof(T) + 64 bytes
    DeviceTight,   // hipMalloc of exactly count * sizeof(T) bytes
    Pinned,        // hipHostMalloc, default flags, exactly count * sizeof(T) bytes
    PinnedMapped   // hipHostMalloc, mapped (the device's address of it: hipHostGetDevicePointer)
};

template <typename T, Mem M = Mem::Device>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }   // elements asked for by the allocation that is held (0: none)

    T* release() { T* p = p_; p_ = nullptr; n_ = 0; return p; }   // gives the allocation up without freeing it
    void reset() {
        if (p_) {
            if (M == Mem::Device || M == Mem::DeviceTight) (void)hipFree(p_);
            else (void)hipHostFree(p_);
        }
        p_ = nullptr; n_ = 0;
    }
    // Releases what is held, then allocates `count` elements.  Device memory gets 64 bytes of slack behind the last element, and needs
    // them: kernels read whole fragments / vectors and so run past the end of some operands (never write there).
    hipError_t alloc(size_t count) {
        reset();
        void* p = nullptr;
        const hipError_t e = M == Mem::Device        ? hipMalloc(&p, count * sizeof(T) + 64)
                             : M == Mem::DeviceTight ? hipMalloc(&p, count * sizeof(T))
                                                     : hipHostMalloc(&p, count * sizeof(T), M == Mem::PinnedMapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); n_ = count;
        return hipSuccess;
    }
    // The policies of a buffer that outlives one call (a third, exact -- kept only while the size asked for stays the same -- holds for
    // the four reference buffers together and is written out where they are made: almpc_set_reference, size()):
    hipError_t once(size_t count) { return p_ ? hipSuccess : alloc(count); }                   // allocated at first use, then kept
    hipError_t grow(size_t count) { return p_ && n_ >= count ? hipSuccess : alloc(count); }    // kept while it is large enough

    // A fresh buffer of count (at least one) elements holding src[0..count) (src null: left as allocated)
    hipError_t upload(const T* src, size_t count) {
        const hipError_t e = alloc(count ? count : 1);
        if (e != hipSuccess || !src || !count) return e;
        return hipMemcpy(p_, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload_async(const T* src, size_t count, hipStream_t st) {
        const hipError_t e = alloc(count ? count : 1);
        if (e != hipSuccess || !src || !count) return e;
        return hipMemcpyAsync(p_, src, count * sizeof(T), hipMemcpyHostToDevice, st);
    }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
using PinBuf = DevBuf<T, Mem::Pinned>;

}  // namespace almpc
