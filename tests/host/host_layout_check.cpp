// host_layout_check.cpp -- csrc/host_layout.hpp on its own, with a host compiler: Carve against offsets worked out by
// hand, the round-up, and the two predicates.  Exit status 0 = every check held; tests/test_host_layout_host.py builds and
// runs it.
#include "../../handobjectconsist_amd/csrc/host_layout.hpp"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

int main() {
    using namespace mr;
    // the round-up
    static_assert(round_up(0) == 0 && round_up(1) == 256 && round_up(256) == 256 && round_up(257) == 512, "256 by default");
    static_assert(round_up(5, 4) == 8 && round_up(8, 4) == 8 && round_up(7, 1) == 7 && round_up(17, 16) == 32, "other powers of two");
    CHECK(round_up((int64_t(1) << 40) + 1) == (int64_t(1) << 40) + 256);

    // default alignment: the owner list of a render backward at B = 3, F = 5 (flags | counter slot | counts | list | records)
    {
        Carve c;
        CHECK(c.total() == 0);
        CHECK(c.take(15) == 0);         // 15 flag bytes -> 256
        CHECK(c.take(256) == 256);      // the raw counter slot
        CHECK(c.take(60) == 512);       // 20 B
        CHECK(c.total() == 768);        // what a call clears
        CHECK(c.take(60) == 768);       // B F 4
        CHECK(c.take(480) == 1024);     // B F 32 -> 512
        CHECK(c.total() == 1536);
    }
    // zero-byte regions take no room and share their offset with the next region; a full slot is not padded further
    {
        Carve c;
        CHECK(c.take(0) == 0);
        CHECK(c.take(0) == 0);
        CHECK(c.take(512) == 0);
        CHECK(c.take(0) == 512);
        CHECK(c.take(1) == 512);
        CHECK(c.total() == 768);
    }
    // the minimum size: an empty region still gets a slot of its own (the pair step's 16-byte minimum)
    {
        Carve c;
        CHECK(c.take(0, 256, 16) == 0);
        CHECK(c.take(8, 256, 16) == 256);
        CHECK(c.take(300, 256, 16) == 512);
        CHECK(c.take(0, 16, 16) == 1024);
        CHECK(c.take(3, 16, 40) == 1040);   // min 40 -> 48
        CHECK(c.total() == 1088);
    }
    // non-default alignments: 16-byte regions, packed word arrays, bytes
    {
        Carve c;
        CHECK(c.take(3072, 16) == 0);
        CHECK(c.take(24, 16) == 3072);      // -> 32
        CHECK(c.take(40, 4) == 3104);
        CHECK(c.take(6, 4) == 3144);        // -> 8
        CHECK(c.take(5, 1) == 3152);
        CHECK(c.take(1) == 3157);           // (an unaligned start stays where it is: only sizes are rounded)
        CHECK(c.total() == 3157 + 256);
    }

    // pointer alignment over a list and a mask
    alignas(16) static char buf[64];
    CHECK(!misaligned({}, 15));
    CHECK(!misaligned({nullptr}, 15));
    CHECK(!misaligned({buf, buf + 16, nullptr, buf + 48}, 15));
    CHECK(misaligned({buf, buf + 8}, 15));
    CHECK(!misaligned({buf, buf + 8}, 7));
    CHECK(misaligned({buf + 4}, 7));
    CHECK(!misaligned({buf + 4, buf + 12}, 3));
    CHECK(misaligned({buf, buf + 16, buf + 33}, 3));
    CHECK(misaligned({buf + 2}, 3) && !misaligned({buf + 2}, 1) && !misaligned({buf + 1}, 0));

    // the grid limit: 2^31 - 1 workgroups
    static_assert(grid_ok(0) && grid_ok(1) && grid_ok(0x7fffffffLL), "within the limit");
    static_assert(!grid_ok(0x80000000LL) && !grid_ok(int64_t(1) << 40), "past the limit");

    if (failures == 0) std::printf("host_layout_check: ok\n");
    return failures == 0 ? 0 : 1;
}
