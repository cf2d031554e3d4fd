// devbuf.h -- move-only owner of one device allocation, DevBuf<T>, and of one pinned host allocation,
// PinnedBuf<T>, that remembers how many elements it holds.  A member of this kind needs no line in a
// destructor or on an error path.  The current device at destruction must be one that can free the
// allocation (the owner's).
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
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // Frees what it held, then allocates exactly `count` elements (room for one when count is 0); holds
    // nothing, count() == 0, on failure.
    hipError_t alloc(size_t count) {
        reset();
        const size_t bytes = sizeof(T) * (count ? count : 1);
        void* p = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e == hipSuccess) {
            p_ = static_cast<T*>(p);
            n_ = count;
        }
        return e;
    }
    // Grow-only: reallocates only when `count` exceeds count() (contents not kept).
    hipError_t reserve(size_t count) { return (p_ && count <= n_) ? hipSuccess : alloc(count); }
    // Grow-only with headroom, for buffers whose size follows the problem's scale: the next power of two of
    // `count`, at least `min_count`, so a pipeline's scales reuse one allocation -- a reallocation frees the
    // old buffer, and hipFree (hipHostFree too) waits for the whole device, other contexts' kernels included:
    // reallocating per problem serialised the pipeline's overlapped contexts.
    hipError_t reserve_pow2(size_t count, size_t min_count) {
        if (p_ && count <= n_) return hipSuccess;
        size_t n = min_count ? min_count : 1;
        while (n < count) n *= 2;
        return alloc(n);
    }
    void reset() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }   // elements held, 0 when empty

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
using PinnedBuf = DevBuf<T, true>;

}  // namespace acmmp
