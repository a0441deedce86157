// carve.h — Carver: the regions of one piece of scratch memory, declared once.  No HIP in here (tests/cpp/test_carve.cpp).
// A call lists its regions in a function of a Carver — one take<T>(n) per region — and that one list is read twice: by a counting
// Carver (no base: every take returns null) for the size to reserve, then by a placing one for the pointers (QueryScratch::carve,
// query.hpp).  A region cannot be handed out without having been counted, and no size is stated a second time.
// Every region starts 16-byte aligned relative to the base (double2 loads), whatever its element type and count.
#pragma once
#include <stddef.h>

struct Carver {
    char* base;       // null: counting only
    size_t bytes = 0; // the end of the last region = the total so far (a multiple of 16)
    explicit Carver(void* base_ = nullptr) : base((char*)base_) {}
    template <class T> T* take(size_t n)
    {
        T* p = base ? (T*)(base + bytes) : nullptr;
        bytes += (n * sizeof(T) + 15) / 16 * 16;
        return p;
    }
    size_t doubles() const { return bytes / sizeof(double); }
};
