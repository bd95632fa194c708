// gt2d_record_main.cpp -- calls the entry point of csrc/gt2d/gt2d.hip on top of tests/host/hip_recorder.cpp and prints, case by
// case, what it asked of the runtime: obj_gt_record_main.cpp's arrangement for the next source with a driver of its own
// (build.NESTED_SOURCES; tests/test_gt2d_record_host.py builds and runs this).
//
//   gt2d_record <kernel argument table> [--stream HEX] [--stack-fill BYTE]
//
// --stream: the value every case passes as its mr_stream_t (NULL without it), announced to the recorder, which then reports
// every call on another stream.  Pointers are made up (argument k of a call sits at k << 40, nothing is ever dereferenced:
// the records are device memory and the entry point reads none of them).  After the cases: the kernels no case launched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshraster_hip.h"

extern "C" {
void rec_load_args(const char* path);
void rec_set_device(int device, int devices);
void rec_set_cus(int cus);
void rec_begin(void);
void rec_expect_stream(void* stream);
void rec_report_unlaunched(void);
}

namespace {

mr_stream_t g_stream = nullptr;
int g_stack_fill = 0;

template <typename T = float>
T* P(int k) { return reinterpret_cast<T*>(static_cast<uintptr_t>(k) << 40); }

// (the launcher's parameter block lives on the stack: a block with uninitialised padding hashes to this byte)
__attribute__((noinline)) void scrub_stack() {
    volatile char pad[96 * 1024];
    for (size_t i = 0; i < sizeof pad; i++) pad[i] = (char)g_stack_fill;
}

void begin(const char* name) {
    std::printf("# %s\n", name);
    rec_begin();
    scrub_stack();
}
void end(int rc) { std::printf("R %d\n", rc); }

// a bank of three models (1097 vertices), 5 x 778 hand vertices, 5 x 21 joints
int batch(int records, int64_t rows, int64_t capacity, bool bank = true, bool dense = true) {
    return mr_gt2d_batch(bank ? P(1) : nullptr, bank ? P<int32_t>(2) : nullptr, bank ? 3 : 0, bank ? 1097 : 0, dense ? P(3) : nullptr, dense ? 5 * 778 : 0,
                         dense ? P(4) : nullptr, dense ? 5 * 21 : 0, P<MrGt2dRecord>(5), records, rows, P(6), P(7), capacity, g_stream);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <kernel argument table> [--stream HEX] [--stack-fill BYTE]\n", argv[0]);
        return 2;
    }
    rec_load_args(argv[1]);
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "--stack-fill") && i + 1 < argc) g_stack_fill = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--stream") && i + 1 < argc) {
            g_stream = reinterpret_cast<mr_stream_t>(static_cast<uintptr_t>(std::strtoull(argv[++i], nullptr, 16)));
            rec_expect_stream(g_stream);
        }
    }
    rec_set_cus(256);
    rec_set_device(0, 1);
    // a step of five frames in two dicts, all three kinds: objects padded to 1031 and 65 rows, 778 hand vertices, 21 joints
    const int64_t rows = 3 * 1031 + 2 * 65 + 5 * 778 + 5 * 21;
    begin("gt2d_batch B5 three kinds");
    end(batch(15, rows, rows));
    // the joints alone: no bank, no camera-frame points
    begin("gt2d_batch B5 joints");
    end(mr_gt2d_batch(nullptr, nullptr, 0, 0, nullptr, 0, P(4), 5 * 21, P<MrGt2dRecord>(5), 5, 5 * 21, P(6), P(7), 5 * 21, g_stream));
    begin("gt2d_batch one row");
    end(batch(1, 1, 1, true, false));
    // nothing to do: no record; records without rows
    begin("gt2d_batch B0");
    end(batch(0, 0, 0));
    begin("gt2d_batch no rows");
    end(batch(15, 0, 0));
    // refused before any launch: a capacity one row short, rows without records, a bank without its vertices
    begin("gt2d_batch short capacity");
    end(batch(15, rows, rows - 1));
    begin("gt2d_batch B0 with rows");
    end(batch(0, rows, rows));
    begin("gt2d_batch bank without vertices");
    end(mr_gt2d_batch(nullptr, P<int32_t>(2), 3, 1097, nullptr, 0, nullptr, 0, P<MrGt2dRecord>(5), 5, 100, P(6), P(7), 100, g_stream));
    std::printf("# never launched\n");
    rec_report_unlaunched();
    return 0;
}
