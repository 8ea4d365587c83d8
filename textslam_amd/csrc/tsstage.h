// tsstage.h -- how a one-call entry point (tsorb_match_*, tsorb_text_extract, tsloop_*, libtsframe's feature calls) stages its data.  Host only.
//
// Such a call keeps one pinned block and one device block on its context, grown on demand (grow_pinned / grow_device), and lays its
// sub-arrays [in | scratch | out] into them at aligned offsets: a Layout hands out Spans in the order of the call's layout comment.  A
// span's element count is written once, at its take(); the copy up (put), the pointer a kernel gets (at(device block)) and the copy down
// (get) all come from the span, so they cannot disagree.  Everything between two mark()s is one contiguous range: the copy up is
// [0, mark() after the inputs), the copy down starts at the first output's offset.  Where the outputs sit at different offsets in the two
// blocks (a pinned block of their own, or device scratch between inputs and outputs) they get a Layout of their own and two bases.
#pragma once
#include <cstddef>
#include <cstring>

// n elements of T at byte offset off of a block (the pinned block, the device block, or the pinned block's device alias)
template <class T> struct Span {
    size_t off = 0, n = 0;
    size_t bytes() const { return n*sizeof(T); }
    size_t end() const { return off + bytes(); }
    T *at(void *base) const { return (T *)((char *)base + off); }
    const T *at(const void *base) const { return (const T *)((const char *)base + off); }
    void put(void *base, const T *src) const { if (n && src) memcpy(at(base), src, bytes()); }          // copy up
    void get(const void *base, T *dst) const { if (n && dst) memcpy(dst, at(base), bytes()); }          // copy down; an array the caller omitted is skipped
};

// a running offset, rounded up to `align` after every take (16 in libtsorb, 256 in libtsloop and libtsframe, 4 for a packed block of 32-bit words); a copy of a Layout continues from the same offset on its own
struct Layout {
    explicit Layout(size_t align) : align_(align) {}
    template <class T> Span<T> take(size_t n) { const Span<T> s{cur_, n}; cur_ = (s.end() + align_ - 1)/align_*align_; return s; }
    size_t mark() const { return cur_; }                                // in_end, out_begin, total, ...
private:
    size_t align_, cur_ = 0;
};

#ifdef __HIPCC__
// room for `need` bytes in a block that only grows: freed and allocated again only when need > cap; p == nullptr, cap == 0 after a failure
static inline hipError_t grow_device(void *&p, size_t &cap, size_t need) {
    if (need <= cap) return hipSuccess;
    if (p) hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) cap = need; else p = nullptr;
    return e;
}
static inline hipError_t grow_pinned(void *&p, size_t &cap, size_t need) {
    if (need <= cap) return hipSuccess;
    if (p) hipHostFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
    if (e == hipSuccess) cap = need; else p = nullptr;
    return e;
}
#endif
