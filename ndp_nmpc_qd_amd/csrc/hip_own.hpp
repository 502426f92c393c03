// hip_own.hpp -- owners of what the HIP runtime hands out: device memory (DevBuf), page-locked host memory (PinnedBuf), events and
// streams.  Move-only; each releases in its destructor and is null-safe.  Host code only: a raw pointer / hipEvent_t / hipStream_t
// anywhere else in the library is a view into an owner's block or the caller's.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <utility>

namespace ndp {

// live objects of the four kinds in the process (ndp_debug_live_resources): +1 behind every successful acquisition, -1 behind every release
inline std::atomic<long> live_resources{0};

// one handle H of the runtime, given back through Free
template <class H, auto Free>
class Owned {
    H h_ = nullptr;

protected:
    template <class Make>
    hipError_t ensure_by(Make make)          // acquires through make(&handle) only if null
    {
        if (h_) return hipSuccess;
        H q = nullptr;
        const hipError_t e = make(&q);
        if (e != hipSuccess) return e;
        h_ = q;
        live_resources.fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }

public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    ~Owned() { reset(); }
    operator H() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    H get() const { return h_; }
    void reset()
    {
        if (!h_) return;
        (void)Free(h_);
        h_ = nullptr;
        live_resources.fetch_sub(1, std::memory_order_relaxed);
    }
};

// bytes of hipMalloc (Pinned false) or hipHostMalloc (true) memory, read as T[]
template <class T, bool Pinned>
struct OwnedBuf : Owned<T *, Pinned ? hipHostFree : hipFree> {
    hipError_t ensure(size_t bytes)          // allocates only if null
    {
        return this->ensure_by([&](T **q) {
            return Pinned ? hipHostMalloc(reinterpret_cast<void **>(q), bytes, hipHostMallocDefault) : hipMalloc(reinterpret_cast<void **>(q), bytes);
        });
    }
    hipError_t alloc(size_t bytes) { this->reset(); return ensure(bytes); }      // releases first; on failure the buffer is null
};
template <class T> using DevBuf = OwnedBuf<T, false>;
template <class T> using PinnedBuf = OwnedBuf<T, true>;

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t ensure(unsigned flags) { return ensure_by([&](hipEvent_t *q) { return hipEventCreateWithFlags(q, flags); }); }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {      // created only if null: with the device's default priority, or with the one given
    hipError_t ensure(unsigned flags) { return ensure_by([&](hipStream_t *q) { return hipStreamCreateWithFlags(q, flags); }); }
    hipError_t ensure(unsigned flags, int priority) { return ensure_by([&](hipStream_t *q) { return hipStreamCreateWithPriority(q, flags, priority); }); }
};

}  // namespace ndp
