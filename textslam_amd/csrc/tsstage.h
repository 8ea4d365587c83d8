// tsstage.h -- how a one-call entry point (tsorb_match_*, tsorb_text_extract, tsloop_*, libtsframe's feature calls, libtsba's staged calls) stages its data.  Host only.
//
// Such a call keeps one pinned block and one device block on its context, grown on demand (Block::grow), and lays its
// sub-arrays [in | scratch | out] into them at aligned offsets: a Layout hands out Spans in the order of the call's layout comment.  A
// span's element count is written once, at its take(); the copy up (put), the pointer a kernel gets (at(device block)) and the copy down
// (get) all come from the span, so they cannot disagree.  Everything between two mark()s is one contiguous range: the copy up is
// [0, mark() after the inputs), the copy down starts at the first output's offset.  Where the outputs sit at different offsets in the two
// blocks (a pinned block of their own, or device scratch between inputs and outputs) they get a Layout of their own and two bases.
//
// A context's block that only grows is a Block member (DeviceBlock, PinnedBlock) and is owned by it alone: it has no capacity field beside it and
// no line in a destroy function, which sets the device, waits for the context's stream(s) and deletes the context; the blocks go with it.
// Deliberately outside, because they are not grow-only: libtsba's slabs, st_host, st_log and hprog (allocated once, or retired while in use);
// libtsorb's per-geometry allocs, h_img, h_out, h_fb and cv_geo (replaced when the geometry changes); libtsframe's map_xy / map_frac (swapped in
// only after the new pair is complete); the plane cache's ic.dev (replaced whole, with its bookkeeping, when the image geometry changes).
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

// a block that only grows, and its owner.  Mem has two static functions: alloc(void **p, size_t n), which returns an error value that compares equal to a
// value-initialised one on success (0), and release(void *p).  Not copyable: a copied context would free its blocks twice.
template <class Mem> struct Block {
    using Err = decltype(Mem::alloc((void **)nullptr, (size_t)0));
    Block() = default;
    Block(const Block &) = delete;
    Block &operator=(const Block &) = delete;
    ~Block() { if (p_) Mem::release(p_); }
    // room for `need` bytes: freed and allocated again, with max(need, room) bytes, only when need > cap(); holds nullptr and cap() == 0 after a failure.
    // The caller sees to it that nothing in flight uses the block when it may move.
    Err grow(size_t need, size_t room = 0) {
        if (need <= cap_) return Err{};
        if (p_) Mem::release(p_);
        p_ = nullptr; cap_ = 0;
        const size_t n = need > room ? need : room;
        const Err e = Mem::alloc(&p_, n);
        if (e == Err{}) cap_ = n; else p_ = nullptr;
        return e;
    }
    template <class T = void> T *as() const { return (T *)p_; }
    size_t cap() const { return cap_; }
private:
    void *p_ = nullptr; size_t cap_ = 0;
};

#ifdef __HIPCC__
struct DeviceMem { static hipError_t alloc(void **p, size_t n) { return hipMalloc(p, n); }  static void release(void *p) { hipFree(p); } };
struct PinnedMem { static hipError_t alloc(void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }  static void release(void *p) { hipHostFree(p); } };
using DeviceBlock = Block<DeviceMem>;
using PinnedBlock = Block<PinnedMem>;
#endif
