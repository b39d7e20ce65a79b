// The one owning type for memory that a handle grows lazily: a pointer, a capacity in elements, and a policy that says where the
// memory lives.  THE CONTRACT (stated here and nowhere else):
//   - grow(count) does nothing when count <= capacity().  Otherwise it releases the old block and allocates count elements.
//     Contents are never preserved.
//   - After a failed grow the buffer is empty: pointer null, capacity 0.  grow returns the policy's error value (hipError_t for the
//     HIP policies), and the policy has already read HIP's sticky last-error slot, so the next launch check sees nothing stale.
//   - The destructor and reset() free the block.  A moved-from buffer is empty.  Copying is deleted.
//   - bytes() reports what is held.
// The handles grow their buffers through ensure() (below), which synchronises the device before a live block is released, because
// a block may be in use on a caller's stream, and turns a failure into the handle's error string and VQHIP_ERR_NOMEM.  Only
// ensure_workspace calls grow itself, for its two-step sizing, and synchronises the same way.
//
// This part includes nothing of HIP: a policy is any type with  error_type, ok, alloc(void**, bytes) -> error_type, release(void*).
#pragma once

#include <cstddef>

template <typename T, typename Policy>
class Buffer {
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~Buffer() { reset(); }

    typename Policy::error_type grow(size_t count)
    {
        if (count <= cap_) return Policy::ok;
        reset();
        void* p = nullptr;
        const typename Policy::error_type e = Policy::alloc(&p, count * sizeof(T));
        if (e != Policy::ok) return e;
        p_ = static_cast<T*>(p), cap_ = count;
        return Policy::ok;
    }
    void reset()
    {
        if (p_) Policy::release(p_);
        p_ = nullptr, cap_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }   // a buffer stands where its raw pointer stood: kernel arguments, pointer arithmetic, null tests
    size_t capacity() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
};

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vqvdb_hip.h"

struct DevicePolicy {
    using error_type = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void** p, size_t bytes)
    {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) (void)hipGetLastError(), *p = nullptr;
        return e;
    }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedPolicy {
    using error_type = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void** p, size_t bytes)
    {
        const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) (void)hipGetLastError(), *p = nullptr;
        return e;
    }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <typename T>
using DevBuf = Buffer<T, DevicePolicy>;
template <typename T>
using PinBuf = Buffer<T, PinnedPolicy>;

namespace {
// Grows a handle's buffer to count elements.  A block that has to go is released only after hipDeviceSynchronize.  A failed
// allocation leaves the buffer empty and returns VQHIP_ERR_NOMEM with message(error) as the handle's error string.  (c is never
// null here, so the error goes straight into c->err, which is all that fail / v3_fail do with a handle.)
template <typename Handle, typename T, typename Policy, typename Message>
int ensure(Handle* c, Buffer<T, Policy>& b, size_t count, Message message)
{
    if (count <= b.capacity()) return VQHIP_OK;
    if (b) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            c->err = std::string("hipDeviceSynchronize before a buffer grows: ") + hipGetErrorString(e);
            return VQHIP_ERR_DEVICE;
        }
    }
    const hipError_t e = b.grow(count);
    if (e == hipSuccess) return VQHIP_OK;
    c->err = message(e);
    return VQHIP_ERR_NOMEM;
}
// ... with the message "cannot allocate <what> (<bytes> bytes): <HIP's error>"
template <typename Handle, typename T, typename Policy>
int ensure(Handle* c, Buffer<T, Policy>& b, size_t count, const char* what)
{
    return ensure(c, b, count, [&](hipError_t e) {
        return std::string("cannot allocate ") + what + " (" + std::to_string(count * sizeof(T)) + " bytes): " + hipGetErrorString(e);
    });
}
}  // namespace
#endif
