// obj_gt_record_main.cpp -- calls the entry points of csrc/obj_gt.hip on top of tests/host/hip_recorder.cpp and prints, case by
// case, what each asked of the runtime: launch_record_main.cpp's arrangement for a source with a driver of its own
// (build.OWN_DRIVER_SOURCES; tests/test_objgt_record_host.py builds and runs this).
//
//   obj_gt_record <kernel argument table> [--stream HEX] [--stack-fill BYTE]
//
// --stream: the value every case passes as its mr_stream_t (NULL without it), announced to the recorder, which then reports
// every call on another stream.  Pointers are made up (argument k of a call sits at k << 40, nothing is ever dereferenced:
// the frame records are device memory and the entry points read none of them).  After the cases: the kernels no case launched.
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

// (the launchers' parameter blocks live on the stack: a block with uninitialised padding hashes to this byte)
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

int batch(int B, int64_t vrows, int64_t frows, int64_t vcap, int64_t fcap) {
    return mr_obj_gt_batch(P(1), P(5), P(4), P<int32_t>(6), P<int32_t>(2), 3, 1097, 2130, P<MrObjFrame>(7), B, vrows, frows, P(8), P(9), vcap,
                           P<int64_t>(10), fcap, P(11), P(12), g_stream);
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
    // a bank of three models (1031 + 65 + 1 vertices, 2000 + 129 + 1 faces), and no model at all
    begin("obj_bank_build models3");
    end(mr_obj_bank_build(P(1), P<int32_t>(2), 3, 1097, P(3), P(4), P(5), g_stream));
    begin("obj_bank_build models0");
    end(mr_obj_bank_build(P(1), P<int32_t>(2), 0, 0, P(3), P(4), P(5), g_stream));
    // a step of five frames in two dicts, padded to 1031 / 2000 and 65 / 129 rows; no frame at all
    const int64_t vrows = 3 * 1031 + 2 * 65, frows = 3 * 2000 + 2 * 129;
    begin("obj_gt_batch B5");
    end(batch(5, vrows, frows, vrows, frows));
    begin("obj_gt_batch B0");
    end(batch(0, 0, 0, 0, 0));
    // refused before any launch: a capacity one row short, rows without frames
    begin("obj_gt_batch B5 short capacity");
    end(batch(5, vrows, frows, vrows - 1, frows));
    begin("obj_gt_batch B0 with rows");
    end(batch(0, vrows, frows, vrows, frows));
    std::printf("# never launched\n");
    rec_report_unlaunched();
    return 0;
}
