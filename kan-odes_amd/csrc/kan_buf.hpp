// kan_buf.hpp — owning buffers of the host code (host only).
//
// Buf<Policy> owns one allocation of its policy (device, pinned, pinned mapped coherent) and frees it once.
// reserve() is the only way to get memory: grow-only, contents not kept, and after a failure the buffer is
// empty (null, 0 bytes), so a size never outlives its pointer.  What an allocation means to its caller
// (draining the stream first, dropping a cached graph or upload, the error text) stays with the caller.
#pragma once
#include <stddef.h>

#include <tuple>
#include <utility>

#ifndef KAN_BUF_NO_HIP
#include <hip/hip_runtime.h>
#endif

namespace kan {

// Policy: error (a type), ok (its success value), error alloc(void**, size_t), void release(void*),
// void clear_error() (drops the runtime's sticky error of a failed alloc).  State of its own (MappedPolicy: the
// device address) goes with the allocation and is reached through policy().
template <class Policy>
class Buf {
  public:
    using error = typename Policy::error;
    Buf() = default;
    Buf(Buf&& o) noexcept { swap(o); }   // (move-only: the source is left empty)
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~Buf() { reset(); }
    void swap(Buf& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        std::swap(pol_, o.pol_);
    }

    void* ptr() const { return p_; }
    template <class T>
    T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    const Policy& policy() const { return pol_; }

    // at least `bytes` bytes; a buffer that has them keeps its pointer and contents, otherwise a fresh
    // allocation replaces it (contents not kept).  On failure: empty, and the sticky error cleared.
    error reserve(size_t bytes) {
        if (bytes <= bytes_) return Policy::ok;
        reset();
        const error e = pol_.alloc(&p_, bytes);
        if (e == Policy::ok) {
            bytes_ = bytes;
        } else {
            pol_.clear_error();
            p_ = nullptr;
            pol_ = Policy{};
        }
        return e;
    }
    void reset() {
        if (p_) pol_.release(p_);
        p_ = nullptr;
        bytes_ = 0;
        pol_ = Policy{};
    }

  private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
    Policy pol_{};
};

// Grow several buffers together and keep what they hold: fresh buffers of bytes[i] each are allocated first,
// copy(fresh...) fills them from the old ones (returning the policy's error type), then they are swapped in.
// A failure at any point frees the fresh ones and leaves the old buffers as they were; *failed is then the
// index of the allocation that failed, or the number of buffers when it was the copy.
template <class Copy, class First, class... Rest>
typename First::error grow_keep(const size_t (&bytes)[1 + sizeof...(Rest)], int* failed, Copy&& copy, Buf<First>& b0,
                                Buf<Rest>&... bs) {
    std::tuple<Buf<First>, Buf<Rest>...> fresh;
    typename First::error e = First::ok;
    int i = 0;
    auto one = [&](auto& f) {   // in order, stopping at the first failure
        if (e == First::ok && (e = f.reserve(bytes[i])) == First::ok) ++i;
    };
    std::apply([&](auto&... f) { (one(f), ...); }, fresh);
    if (e == First::ok) e = std::apply(copy, fresh);
    if (e != First::ok) {
        *failed = i;
        return e;
    }
    std::apply([&](auto& f0, auto&... f) { (b0.swap(f0), ..., bs.swap(f)); }, fresh);
    return e;
}

#ifndef KAN_BUF_NO_HIP
struct HipPolicyBase {
    using error = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static void clear_error() { (void)hipGetLastError(); }
};
struct DevicePolicy : HipPolicyBase {
    hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    void release(void* p) { (void)hipFree(p); }
};
struct PinnedPolicy : HipPolicyBase {
    hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
    void release(void* p) { (void)hipHostFree(p); }
};
// pinned, mapped and coherent, with the device address of the allocation; dev stays null where the runtime
// gives none (the caller then copies instead of having kernels write there)
struct MappedPolicy : HipPolicyBase {
    void* dev = nullptr;
    hipError_t alloc(void** p, size_t bytes) {
        const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess && hipHostGetDevicePointer(&dev, *p, 0) != hipSuccess) {
            (void)hipGetLastError();
            dev = nullptr;
        }
        return e;
    }
    void release(void* p) { (void)hipHostFree(p); }
};
using DevBuf = Buf<DevicePolicy>;
using PinnedBuf = Buf<PinnedPolicy>;
struct MappedBuf : Buf<MappedPolicy> {
    template <class T>
    T* dev() const { return static_cast<T*>(policy().dev); }
};
#endif

}  // namespace kan
