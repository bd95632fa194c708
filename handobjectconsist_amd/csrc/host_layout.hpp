// host_layout.hpp -- what the host side of every entry point shares: the round-up, workspace carving, and the pointer /
// grid checks.  Plain C++17, no HIP include (tests/host/host_layout_check.cpp builds it with the host compiler alone).
//
// A workspace is laid out by ONE function that carves its regions in order and returns their offsets plus the total; the
// sizing entry point returns that total and the launcher adds the offsets to its base pointer, so the two cannot disagree.
#pragma once
#include <cstdint>
#include <initializer_list>

namespace mr {

// x rounded up to a multiple of `align` (a power of two).  constexpr: the device side of a HIP build may call it too.
constexpr int64_t round_up(int64_t x, int64_t align = 256) { return (x + (align - 1)) & ~(align - 1); }

// A running byte offset.  take() returns where the region starts and moves on by its size -- at least min_bytes -- rounded
// up to `align`, so that on an aligned base every region starts aligned.
struct Carve {
    int64_t at = 0;
    int64_t take(int64_t bytes, int64_t align = 256, int64_t min_bytes = 0) {
        const int64_t start = at;
        at += round_up(bytes > min_bytes ? bytes : min_bytes, align);
        return start;
    }
    int64_t total() const { return at; }
};

// true when any of the pointers has a bit of `mask` set (mask = alignment - 1); null pointers pass
inline bool misaligned(std::initializer_list<const void*> ptrs, uintptr_t mask) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & mask) != 0;
}

// a grid dimension the launch can take (x: 2^31 - 1 workgroups)
constexpr bool grid_ok(int64_t blocks) { return blocks <= 0x7fffffffLL; }

}  // namespace mr
