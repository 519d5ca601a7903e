// dev_buf.h -- the one owner of a device array or of pinned host words, and the group form for arrays that are sized together.  A pure
// header: it makes no HIP call.  The including file supplies, before the #include, the error type and the two functions it allocates
// and frees through (graal_hip.hip: hipError_t, hipMalloc / hipHostMalloc and hipFree / hipHostFree; host_check.cpp: int and a counting
// host allocator that can be told to fail):
//     using devbuf_err = ...;                                      // its value-initialised value is success
//     devbuf_err devbuf_alloc(void** p, size_t bytes, bool pinned);
//     void devbuf_free(void* p, bool pinned);
//
// The owners' rule, kept by the type: a buffer's pointer is valid or null, never dangling; a buffer is released BEFORE its replacement is
// allocated (old and new are never held together: the contact queue alone is 320 MB at the 50k-fragment map); a group's size reads 0
// from the moment its members are released until every one of them is allocated again.  After a failed allocation every pointer is
// therefore valid or null and the size is 0: the next call releases the survivors once and starts again, and the destructor frees what
// is left, once.  Nothing is zero-filled here but pinned words; a device array's hipMemset stays with its caller.
#pragma once
#include <cstddef>
#include <cstring>
#include <type_traits>

// Not copyable, so it cannot be handed to a kernel; where a T* is wanted (a kernel argument, an argument struct, a hipMemcpy) it converts.
// count: the elements held (bytes for DevBuf<void>, the scratch of a hipCUB pass).  An element count of 0 holds nothing: the buffer is
// released, the pointer is null and the allocator is not called -- what hipMalloc of 0 bytes gave the call sites before.
template <class T, bool Pinned = false>
struct DevBuf {
    T* p = nullptr;
    size_t count = 0;
    static constexpr size_t elem_bytes = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), count(o.count) { o.p = nullptr; o.count = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; count = o.count; o.p = nullptr; o.count = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    operator T*() const { return p; }

    void release()
    {
        if (p) devbuf_free(p, Pinned);
        p = nullptr; count = 0;
    }
    // release, then allocate n elements
    devbuf_err alloc(size_t n)
    {
        release();
        if (n == 0) return devbuf_err{};
        void* q = nullptr;
        const devbuf_err e = devbuf_alloc(&q, n * elem_bytes, Pinned);
        if (e != devbuf_err{}) return e;
        if (Pinned) memset(q, 0, n * elem_bytes);
        p = (T*)q; count = n;
        return e;
    }
    // The two policies.  Exact: the per-layout arrays, keyed on n or S -- reallocated when the wanted count differs.  Grow-only: tables,
    // scratch, per-call arrays -- reallocated when the wanted count exceeds what is held, and then used below their allocation.
    devbuf_err reserve_exact(size_t n) { return n == count ? devbuf_err{} : alloc(n); }
    devbuf_err reserve_grow(size_t n) { return n <= count ? devbuf_err{} : alloc(n); }
};
template <class T> using PinBuf = DevBuf<T, true>;

inline void dev_release_each() {}
template <class B, class... R> void dev_release_each(B& b, size_t, R&&... rest) { b.release(); dev_release_each(rest...); }
inline devbuf_err dev_alloc_each() { return devbuf_err{}; }
template <class B, class... R> devbuf_err dev_alloc_each(B& b, size_t n, R&&... rest)
{
    const devbuf_err e = b.alloc(n);
    return e != devbuf_err{} ? e : dev_alloc_each(rest...);
}

// A group: arrays sized together, given as (buffer, element count) pairs.  group_alloc releases every member first, then allocates them
// in the order given.  Under a size field, group_realloc records the size only then (it reads 0 in between, and after a failure);
// group_exact / group_grow apply the two policies to the size field; a set keyed on more than one number (n and S) tests its keys
// itself and calls group_realloc.
template <class... M> devbuf_err group_alloc(M&&... members)
{
    dev_release_each(members...);
    return dev_alloc_each(members...);
}
template <class N, class... M> devbuf_err group_realloc(N& size, size_t want, M&&... members)
{
    size = 0;
    const devbuf_err e = group_alloc(members...);
    if (e == devbuf_err{}) size = (N)want;
    return e;
}
template <class N, class... M> devbuf_err group_exact(N& size, size_t want, M&&... members)
{
    return (size_t)size == want ? devbuf_err{} : group_realloc(size, want, members...);
}
template <class N, class... M> devbuf_err group_grow(N& size, size_t want, M&&... members)
{
    return want <= (size_t)size ? devbuf_err{} : group_realloc(size, want, members...);
}
