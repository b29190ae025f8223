// buffers.h - the one owner of a device or pinned allocation (plain C++17, no HIP include: the tests compile it alone).
//
// Buf<Alloc, T> owns a pointer and its capacity in bytes; the two change only together.  Alloc supplies
//   static bool alloc(void** p, size_t bytes);   static void free(void* p);
// Move-only.  After a failed grow the buffer is {nullptr, 0}, so a later "is it large enough?" cannot pass on a stale size.
#pragma once
#include <cstddef>

template <class Alloc, class T = void>
class Buf {
    void* p_ = nullptr;
    size_t bytes_ = 0;

public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, bytes_ = o.bytes_;
            o.p_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    void reset() {
        if (p_) Alloc::free(p_);
        p_ = nullptr, bytes_ = 0;
    }
    // Nothing when the capacity covers need_bytes; otherwise the old block is freed, then alloc_bytes are allocated.
    // false: the allocation failed and the buffer is empty.
    bool grow(size_t need_bytes, size_t alloc_bytes) {
        if (bytes_ >= need_bytes) return true;
        reset();
        if (!Alloc::alloc(&p_, alloc_bytes)) {
            p_ = nullptr;
            return false;
        }
        bytes_ = alloc_bytes;
        return true;
    }
    bool grow(size_t bytes) { return grow(bytes, bytes); }

    size_t bytes() const { return bytes_; }
    T* get() const { return static_cast<T*>(p_); }
    operator T*() const { return get(); }  // (kernel arguments and KArgs take raw pointers)
    T* operator->() const { return get(); }
    template <class U>
    explicit operator U*() const { return static_cast<U*>(p_); }  // (a cast written out views the block as another type)
};
