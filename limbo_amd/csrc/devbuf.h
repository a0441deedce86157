// devbuf.h — DevBuf<T>: the one owner of a piece of device memory on the host side (engine.hip and the .hpp parts of it).
// A pointer and a capacity in elements; move-only; the destructor frees.  It converts to T*, so that a member of this type is
// passed to a launch wrapper, tested and offset like the raw pointer it replaces: only the sites that allocate or free name it.
// No pooling, no allocator parameter, no reference counting.  hipFree waits for the device; a site that must not free
// under a launch of ANOTHER stream's synchronises that stream itself, in front of reset().
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <stddef.h>
#include <stdint.h>

#define DEVBUF_LOCAL __attribute__((visibility("hidden"))) // (nothing of this header is part of the library's interface)

// buffers and bytes alive in this process (gpe_debug_live_buffers: a life cycle that returns to its count leaked nothing)
struct DEVBUF_LOCAL DevBufLive {
    static inline std::atomic<int64_t> count{0}, bytes{0};
};

template <class T> class DEVBUF_LOCAL DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0; // elements

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    void swap(DevBuf& o) noexcept
    {
        T* p = p_;
        const size_t n = cap_;
        p_ = o.p_, cap_ = o.cap_;
        o.p_ = p, o.cap_ = n;
    }
    // room for n elements: grows, never shrinks; what was there is NOT kept.  On failure the buffer is empty
    hipError_t reserve(size_t n)
    {
        if (n <= cap_)
            return hipSuccess;
        reset();
        const hipError_t e = hipMalloc(&p_, sizeof(T) * n);
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        cap_ = n;
        DevBufLive::count.fetch_add(1, std::memory_order_relaxed);
        DevBufLive::bytes.fetch_add((int64_t)(sizeof(T) * n), std::memory_order_relaxed);
        return hipSuccess;
    }
    void reset()
    {
        if (p_) {
            (void)hipFree(p_);
            DevBufLive::count.fetch_sub(1, std::memory_order_relaxed);
            DevBufLive::bytes.fetch_sub((int64_t)(sizeof(T) * cap_), std::memory_order_relaxed);
        }
        p_ = nullptr;
        cap_ = 0;
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
};
