// devbuf.h -- move-only owner of one device allocation, DevBuf<T>, and of one pinned host allocation,
// PinnedBuf<T>.  A member of this kind needs no line in a destructor or on an error path.  The current
// device at destruction must be one that can free the allocation (the owner's).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace acmmp {

template <typename T, bool PINNED = false>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // Frees what it held, then allocates `count` elements (at least one); holds nothing on failure.
    hipError_t alloc(size_t count) {
        reset();
        const size_t bytes = sizeof(T) * (count ? count : 1);
        void* p = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e == hipSuccess) p_ = static_cast<T*>(p);
        return e;
    }
    void reset() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
};

template <typename T>
using PinnedBuf = DevBuf<T, true>;

}  // namespace acmmp
