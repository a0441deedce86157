// The typed scratch carver (limbo_amd/csrc/carve.h) alone, on the host: built with -fsanitize=address,undefined and run by
// tests/test_carve.py.  One list of regions is read by a counting Carver and by a placing one; every offset is a multiple of 16
// bytes, regions do not overlap, each holds its count, the total is the end of the last region, and writing every element of
// every region stays inside a malloc of exactly the counted size (AddressSanitizer is the witness).
#include "../../limbo_amd/csrc/carve.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct Odd { // 40 bytes: no multiple of 16 (as select.hip's state words, gemm.hip's launch items)
    double a, b, c;
    int64_t d;
    int32_t e, f;
};
static_assert(sizeof(Odd) == 40, "a struct whose size is no multiple of 16");

struct Region {
    const char* name;
    char* p;
    size_t count, elem;
};
struct Regions {
    double* d0 = nullptr;
    int* i_odd = nullptr;
    double* empty = nullptr;
    Odd* one = nullptr;
    int32_t* i32 = nullptr;
    long long* ll = nullptr;
    Odd* odd3 = nullptr;
    int64_t* i64 = nullptr;
    char* bytes = nullptr;
    double* last = nullptr;
};
static const size_t kCounts[10] = {5, 7, 0, 1, 13, 3, 3, 9, 1, 2};

// the one list: what a call hands to QueryScratch::carve
static void regions(Carver& cv, Regions& r)
{
    r.d0 = cv.take<double>(kCounts[0]);
    r.i_odd = cv.take<int>(kCounts[1]); // an odd count of 4-byte elements
    r.empty = cv.take<double>(kCounts[2]); // zero-length
    r.one = cv.take<Odd>(kCounts[3]);
    r.i32 = cv.take<int32_t>(kCounts[4]);
    r.ll = cv.take<long long>(kCounts[5]);
    r.odd3 = cv.take<Odd>(kCounts[6]);
    r.i64 = cv.take<int64_t>(kCounts[7]);
    r.bytes = cv.take<char>(kCounts[8]);
    r.last = cv.take<double>(kCounts[9]);
}

static int fails = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            printf("FAIL " __VA_ARGS__);     \
            printf("  [%s]\n", #cond);       \
            ++fails;                         \
        }                                    \
    } while (0)

template <class T> static void fill(T* p, size_t n, int tag)
{
    for (size_t i = 0; i < n; ++i)
        memset(&p[i], tag, sizeof(T));
}

int main()
{
    Carver count;
    Regions rc;
    regions(count, rc);
    CHECK(!rc.d0 && !rc.one && !rc.last, "a counting carver hands out nothing\n");
    CHECK(count.bytes % 16 == 0 && count.doubles() * sizeof(double) == count.bytes, "total %zu\n", count.bytes);

    char* base = (char*)malloc(count.bytes); // exactly the reported size: one byte past it is AddressSanitizer's to report
    CHECK(((uintptr_t)base & 15) == 0, "malloc's alignment\n");
    Carver place(base);
    Regions r;
    regions(place, r);
    CHECK(place.bytes == count.bytes, "placing %zu against counting %zu\n", place.bytes, count.bytes);

    const Region list[10] = {{"d0", (char*)r.d0, kCounts[0], sizeof(double)},     {"i_odd", (char*)r.i_odd, kCounts[1], sizeof(int)},
                             {"empty", (char*)r.empty, kCounts[2], sizeof(double)}, {"one", (char*)r.one, kCounts[3], sizeof(Odd)},
                             {"i32", (char*)r.i32, kCounts[4], sizeof(int32_t)},   {"ll", (char*)r.ll, kCounts[5], sizeof(long long)},
                             {"odd3", (char*)r.odd3, kCounts[6], sizeof(Odd)},     {"i64", (char*)r.i64, kCounts[7], sizeof(int64_t)},
                             {"bytes", r.bytes, kCounts[8], 1},                    {"last", (char*)r.last, kCounts[9], sizeof(double)}};
    CHECK(list[0].p == base, "the first region starts at the base\n");
    for (int i = 0; i < 10; ++i) {
        const Region& a = list[i];
        const size_t off = (size_t)(a.p - base), end = off + a.count * a.elem;
        CHECK(off % 16 == 0, "%s: offset %zu\n", a.name, off);
        CHECK(end <= count.bytes, "%s: ends at %zu of %zu\n", a.name, end, count.bytes);
        // holds its count, no overlap: the next region starts at or behind this one's end, less than 16 bytes behind it
        const size_t next = i + 1 < 10 ? (size_t)(list[i + 1].p - base) : count.bytes;
        CHECK(next >= end && next - end < 16, "%s: [%zu, %zu), the next at %zu\n", a.name, off, end, next);
    }
    CHECK(r.empty == (double*)r.one, "a zero-length region takes no room\n");

    // every element of every region written, then read back: no region reaches into another, none leaves the allocation
    fill(r.d0, kCounts[0], 1);
    fill(r.i_odd, kCounts[1], 2);
    fill(r.empty, kCounts[2], 3);
    fill(r.one, kCounts[3], 4);
    fill(r.i32, kCounts[4], 5);
    fill(r.ll, kCounts[5], 6);
    fill(r.odd3, kCounts[6], 7);
    fill(r.i64, kCounts[7], 8);
    fill(r.bytes, kCounts[8], 9);
    fill(r.last, kCounts[9], 10);
    const int tags[10] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    for (int i = 0; i < 10; ++i)
        for (size_t k = 0; k < list[i].count * list[i].elem; ++k)
            CHECK(list[i].p[k] == tags[i], "%s: byte %zu was overwritten\n", list[i].name, k);
    free(base);

    // an empty list
    Carver none;
    CHECK(none.bytes == 0 && none.doubles() == 0, "an empty list\n");
    if (fails)
        return 1;
    printf("carve ok: %zu bytes in 10 regions\n", count.bytes);
    return 0;
}
