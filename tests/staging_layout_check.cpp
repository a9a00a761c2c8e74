// Stand-alone check of csrc/staging_layout.hpp (tests/test_staging_layout.py builds it with the address and undefined-behaviour
// sanitisers and runs it): every array of a layout is filled through ptr<T> in a host buffer of the reported size, then the
// offsets, the region bounds and the total are checked.  Exit status 0 and "ok" on stdout: all held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "staging_layout.hpp"

using qsp::StagingLayout;

struct B32 { uint8_t b[32]; };                    // an ORB descriptor
struct B56 { int32_t a[2]; double d[6]; };        // a per-frame record
static_assert(sizeof(B32) == 32 && sizeof(B56) == 56, "element sizes");

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);              \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

struct Arr { size_t off, elem, n; int region; };   // region 0 up, 1 scratch, 2 down

template <typename T>
static void take(StagingLayout& L, std::vector<Arr>& arrs, size_t n, int region) {
    arrs.push_back({L.take<T>(n), sizeof(T), n, region});
}

// every element written as a T through ptr<T> (a misaligned or out-of-range one trips a sanitiser), bytes = the array's tag
template <typename T>
static void fill(std::vector<char>& buf, const Arr& a, uint8_t tag) {
    T* p = qsp::ptr<T>(buf.data(), a.off);
    const T* cp = qsp::ptr<T>((const void*)buf.data(), a.off);
    CHECK((const void*)p == (const void*)cp);
    for (size_t i = 0; i < a.n; ++i) {
        T v;
        uint8_t* raw = reinterpret_cast<uint8_t*>(&v);
        for (size_t k = 0; k < sizeof(T); ++k) raw[k] = tag;
        p[i] = v;
    }
}

static void fill_any(std::vector<char>& buf, const Arr& a, uint8_t tag) {
    switch (a.elem) {
        case 1: fill<uint8_t>(buf, a, tag); break;
        case 4: fill<int32_t>(buf, a, tag); break;
        case 8: fill<double>(buf, a, tag); break;
        case 32: fill<B32>(buf, a, tag); break;
        case 56: fill<B56>(buf, a, tag); break;
        default: CHECK(false);
    }
}

static void check(const StagingLayout& L, const std::vector<Arr>& arrs) {
    size_t end = 0, first[3] = {0, 0, 0}, last[3] = {0, 0, 0};
    bool seen[3] = {false, false, false};
    int region = 0;
    for (const Arr& a : arrs) {
        CHECK(a.off % 16 == 0);
        CHECK(a.off >= end);                                     // in order and disjoint
        CHECK(a.region >= region);
        region = a.region;
        if (!seen[a.region]) { first[a.region] = a.off; seen[a.region] = true; }
        end = a.off + a.elem * a.n;
        last[a.region] = end;
    }
    // up, scratch and down are consecutive; the bounds are the first and the last arrays of each region
    CHECK(L.up_bytes() % 16 == 0 && L.down_begin() % 16 == 0 && L.up_bytes() <= L.down_begin());
    if (seen[0]) { CHECK(first[0] == 0); CHECK(last[0] <= L.up_bytes() && L.up_bytes() - last[0] < 16); }
    else CHECK(L.up_bytes() == 0);
    if (seen[1]) { CHECK(first[1] == L.up_bytes()); CHECK(last[1] <= L.down_begin() && L.down_begin() - last[1] < 16); }
    else CHECK(L.down_begin() == L.up_bytes());
    const size_t down_end = L.down_begin() + L.down_bytes();
    if (seen[2]) { CHECK(first[2] == L.down_begin()); CHECK(last[2] <= down_end && down_end - last[2] < 16); }
    else CHECK(L.down_bytes() == 0);
    CHECK(L.total() % 256 == 0 && L.total() >= end && L.total() >= down_end && L.total() - down_end < 256);
    for (const Arr& a : arrs)
        if (a.region == 2) CHECK(L.in_down(a.off) == a.off - L.down_begin());
    // fill every array, then read every array back: a shared byte would carry the later tag
    std::vector<char> buf(L.total());
    for (size_t i = 0; i < arrs.size(); ++i) fill_any(buf, arrs[i], (uint8_t)(i + 1));
    for (size_t i = 0; i < arrs.size(); ++i)
        for (size_t k = 0; k < arrs[i].elem * arrs[i].n; ++k) CHECK((uint8_t)buf[arrs[i].off + k] == (uint8_t)(i + 1));
}

int main() {
    {   // mixed element sizes, 0 / 1 / 15 / 16 / 17 elements, all three regions
        StagingLayout L;
        std::vector<Arr> a;
        take<uint8_t>(L, a, 17, 0); take<int32_t>(L, a, 0, 0); take<double>(L, a, 15, 0); take<B32>(L, a, 1, 0); take<B56>(L, a, 16, 0);
        take<int32_t>(L, a, 1, 0);
        L.begin_scratch();
        take<uint8_t>(L, a, 1, 1); take<B56>(L, a, 17, 1); take<int32_t>(L, a, 15, 1); take<double>(L, a, 16, 1); take<B32>(L, a, 0, 1);
        L.begin_down();
        take<double>(L, a, 0, 2); take<int32_t>(L, a, 16, 2); take<uint8_t>(L, a, 15, 2); take<B32>(L, a, 17, 2); take<double>(L, a, 1, 2);
        take<B56>(L, a, 1, 2); take<int32_t>(L, a, 17, 2); take<uint8_t>(L, a, 16, 2);
        check(L, a);
    }
    {   // no scratch: begin_down() closes UP
        StagingLayout L;
        std::vector<Arr> a;
        take<B56>(L, a, 15, 0); take<uint8_t>(L, a, 16, 0);
        L.begin_down();
        take<B32>(L, a, 16, 2); take<uint8_t>(L, a, 17, 2);
        check(L, a);
        CHECK(L.up_bytes() == L.down_begin());
    }
    {   // an empty region between two that are not, and an empty DOWN
        StagingLayout L;
        std::vector<Arr> a;
        take<int32_t>(L, a, 17, 0);
        L.begin_scratch();
        take<double>(L, a, 0, 1);
        L.begin_down();
        check(L, a);
        CHECK(L.down_bytes() == 0 && L.total() == 256);
    }
    {   // all empty: every array has the same offset, the block is empty
        StagingLayout L;
        std::vector<Arr> a;
        take<uint8_t>(L, a, 0, 0); take<B56>(L, a, 0, 0);
        L.begin_scratch();
        take<double>(L, a, 0, 1);
        L.begin_down();
        take<B32>(L, a, 0, 2); take<int32_t>(L, a, 0, 2);
        check(L, a);
        CHECK(L.up_bytes() == 0 && L.down_begin() == 0 && L.down_bytes() == 0 && L.total() == 0);
        StagingLayout none;
        check(none, {});
        CHECK(none.total() == 0);
    }
    std::puts("ok");
    return 0;
}
