// The HIP-free half of textslam_amd/csrc/tsstage.h (Span, Layout, Block) on the CPU, no HIP header: built with -fsanitize=address,undefined by tests/test_stage_layout.py.
// Every check prints what failed and the program exits with 1; "stage layout host: ok" is the last line of a clean run.
#include "../../textslam_amd/csrc/tsstage.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); failures++; } } while (0)

struct F3 { float v[3]; };                  // 12 bytes: a 3-float point
struct Pose { double v[3]; };               // 24 bytes
static_assert(sizeof(F3) == 12 && sizeof(Pose) == 24, "element sizes");

struct Ext { size_t off, end; };
template <class T> static Ext ext(const Span<T> &s) { return Ext{s.off, s.off + s.bytes()}; }

// every byte of every element set from a counter, so a span that lands on another's bytes shows
template <class T> static std::vector<T> pattern(size_t n, unsigned seed) {
    std::vector<T> v(n);
    unsigned char *b = reinterpret_cast<unsigned char *>(v.data());
    for (size_t i = 0; i < n*sizeof(T); i++) b[i] = (unsigned char)(seed + 7*i + 1);
    return v;
}
template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size()*sizeof(T)) == 0);
}
template <class T> static void round_trip(const Span<T> &s, void *block, unsigned seed) {
    const std::vector<T> src = pattern<T>(s.n, seed);
    s.put(block, src.data());
    std::vector<T> dst(s.n);
    s.get(block, dst.data());
    CHECK(same(src, dst));
}

static void run(size_t align) {
    Layout L(align);
    CHECK(L.mark() == 0);
    // odd counts, element sizes 1, 4, 8, 12 and 24, zero-length spans first, in the middle and last
    const auto z0 = L.take<double>(0);
    const auto a = L.take<uint8_t>(17);
    const auto b = L.take<int32_t>(3);
    const auto c = L.take<double>(1);
    const size_t before_z1 = L.mark();
    const auto z1 = L.take<F3>(0);
    CHECK(L.mark() == before_z1);                                   // no room beyond what alignment already gave
    const auto d = L.take<F3>(17);
    const auto e = L.take<Pose>(3);
    const auto f = L.take<uint8_t>(1);
    const auto g = L.take<Pose>(1);
    const size_t before_z2 = L.mark();
    const auto z2 = L.take<int32_t>(0);
    CHECK(L.mark() == before_z2);
    const size_t tot = L.mark();

    CHECK(a.n == 17 && a.bytes() == 17 && b.bytes() == 12 && c.bytes() == 8 && d.bytes() == 12*17 && e.bytes() == 72 && g.bytes() == 24 && z1.bytes() == 0);
    const Ext x[] = { ext(z0), ext(a), ext(b), ext(c), ext(z1), ext(d), ext(e), ext(f), ext(g), ext(z2) };
    const size_t nx = sizeof(x)/sizeof(x[0]);
    for (size_t i = 0; i < nx; i++) {
        CHECK(x[i].off % align == 0);
        CHECK(x[i].end <= tot);
        if (i + 1 < nx) CHECK(x[i].end <= x[i + 1].off);            // taken in order, so no two overlap
    }
    CHECK(tot % align == 0);
    CHECK(z0.off == 0 && a.off == 0);                               // a zero-length span moves nothing

    // a copy of a Layout goes on from the same offset on its own
    Layout M = L;
    const auto m = M.take<int32_t>(3);
    CHECK(m.off == tot && L.mark() == tot && M.mark() > tot);

    // put then get through a heap block of exactly mark() bytes: AddressSanitizer sees a byte past either end
    unsigned char *block = (unsigned char *)malloc(tot);
    memset(block, 0xEE, tot);
    round_trip(a, block, 1); round_trip(b, block, 2); round_trip(c, block, 3); round_trip(d, block, 4); round_trip(e, block, 5); round_trip(f, block, 6); round_trip(g, block, 7);
    // all written: every array is still what was put (nothing wrote over a neighbour), and the padding between them is untouched
    { std::vector<uint8_t> ra(a.n); a.get(block, ra.data()); CHECK(same(ra, pattern<uint8_t>(a.n, 1)));
      std::vector<F3> rd(d.n); d.get(block, rd.data()); CHECK(same(rd, pattern<F3>(d.n, 4)));
      std::vector<Pose> re(e.n); e.get(block, re.data()); CHECK(same(re, pattern<Pose>(e.n, 5))); }
    for (size_t i = 0; i + 1 < nx; i++) for (size_t k = x[i].end; k < x[i + 1].off; k++) CHECK(block[k] == 0xEE);
    for (size_t k = x[nx - 1].end; k < tot; k++) CHECK(block[k] == 0xEE);

    // null source / destination and zero-length spans touch nothing, null pointers included
    std::vector<unsigned char> snap(block, block + tot);
    b.put(block, nullptr); d.put(block, nullptr);
    b.get(block, nullptr); e.get(block, nullptr);
    z1.put(block, nullptr); z1.get(block, nullptr);
    z2.put(nullptr, nullptr); z2.get(nullptr, nullptr);
    { const F3 one = {{1.f, 2.f, 3.f}}; F3 out = {{9.f, 9.f, 9.f}}; z1.put(block, &one); z1.get(block, &out); CHECK(out.v[0] == 9.f && out.v[2] == 9.f); }
    { int32_t out[3] = {5, 6, 7}; z2.get(block, out); CHECK(out[0] == 5 && out[2] == 7); }
    CHECK(memcmp(snap.data(), block, tot) == 0);

    // a second base (the device block): the same offset
    unsigned char *other = (unsigned char *)malloc(tot);
    CHECK((unsigned char *)d.at(other) - other == (unsigned char *)d.at(block) - block && (size_t)((unsigned char *)d.at(other) - other) == d.off);
    CHECK((const unsigned char *)g.at((const void *)other) - other == (ptrdiff_t)g.off);
    memcpy(other, block, tot);
    { std::vector<Pose> rg(g.n); g.get(other, rg.data()); CHECK(same(rg, pattern<Pose>(g.n, 7))); }
    free(other); free(block);
}

// ---- the owner of a block that only grows, over malloc / free; Mem counts what is live and fails on request
struct Mem {
    static int live, fail_next;
    static int alloc(void **p, size_t n) {
        if (fail_next) { fail_next = 0; *p = nullptr; return 7; }
        *p = malloc(n); if (!*p) return 7;
        live++; return 0;
    }
    static void release(void *p) { free(p); live--; }
};
int Mem::live = 0, Mem::fail_next = 0;
static_assert(!std::is_copy_constructible<Block<Mem>>::value && !std::is_copy_assignable<Block<Mem>>::value, "a copied context would free its blocks twice");
struct TwoBlocks { Block<Mem> a, b; int x = 0; };                          // a context: not copyable either
static_assert(!std::is_copy_constructible<TwoBlocks>::value, "a context with a block cannot be copied");

static void fill(Block<Mem> &b, unsigned char v) { memset(b.as<unsigned char>(), v, b.cap()); }           // every byte of the capacity: AddressSanitizer holds it to the size
static void run_blocks() {
    {
        Block<Mem> b;
        CHECK(b.as() == nullptr && b.cap() == 0 && Mem::live == 0);             // starts empty
        CHECK(b.grow(0) == 0 && b.as() == nullptr && Mem::live == 0);           // nothing needed: nothing allocated
        CHECK(b.grow(100) == 0 && b.as() != nullptr && b.cap() == 100 && Mem::live == 1);
        fill(b, 0x11);
        void *p0 = b.as();
        CHECK(b.grow(40) == 0 && b.as() == p0 && b.cap() == 100);               // a smaller request keeps pointer and capacity
        CHECK(b.grow(100, 4000) == 0 && b.as() == p0 && b.cap() == 100);        // room counts only when the block must move
        CHECK(b.as<unsigned char>()[99] == 0x11);
        CHECK(b.grow(101) == 0 && b.cap() == 101 && Mem::live == 1);            // larger: freed, then allocated again -- one block live
        fill(b, 0x22);
        CHECK(b.grow(300, 1000) == 0 && b.cap() == 1000 && Mem::live == 1);     // capacity == max(need, room)
        fill(b, 0x33);
        CHECK(b.grow(2000, 1500) == 0 && b.cap() == 2000 && Mem::live == 1);
        fill(b, 0x44);
        CHECK(b.as<int32_t>() == (int32_t *)b.as() && (const void *)b.as<const double>() == b.as());
        // a failed allocation: null and 0, the old block gone (freed first); the next grow works again
        Mem::fail_next = 1;
        CHECK(b.grow(5000) == 7 && b.as() == nullptr && b.cap() == 0 && Mem::live == 0);
        CHECK(b.grow(10) == 0 && b.as() != nullptr && b.cap() == 10 && Mem::live == 1);
        fill(b, 0x55);
        Mem::fail_next = 1;
        CHECK(b.grow(5) == 0 && b.cap() == 10 && Mem::fail_next == 1);          // (no allocation attempted)
        Mem::fail_next = 0;
        Block<Mem> never;                                                       // destroyed empty: nothing to free
        TwoBlocks *ctx = new TwoBlocks();
        CHECK(ctx->a.grow(64) == 0 && ctx->b.grow(1, 32) == 0 && ctx->b.cap() == 32 && Mem::live == 3);
        fill(ctx->a, 0x66); fill(ctx->b, 0x77);
        delete ctx;                                                             // the blocks go with the context
        CHECK(Mem::live == 1);
    }
    CHECK(Mem::live == 0);                      // destructors only; LeakSanitizer judges the same at exit
}

int main() {
    run(4);
    run(16);
    run(256);
    run_blocks();
    if (failures) { printf("stage layout host: %d check(s) failed\n", failures); return 1; }
    printf("stage layout host: ok\n");
    return 0;
}
