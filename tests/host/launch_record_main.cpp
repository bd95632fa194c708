// launch_record_main.cpp -- calls the raster and warp entry points over a table of cases on top of tests/host/hip_recorder.cpp
// and prints, case by case, what each asked of the runtime: a device-free record of every launcher's decisions.
//
//   launch_record <kernel argument table> [--cus N] [--stack-fill BYTE] [--two-devices] [--stream HEX] [--unrecorded]
//
// --stream: the value every case passes as its mr_stream_t (NULL without it), announced to the recorder, which then reports
// every call on another stream; nothing else of the output changes.  --unrecorded: the recorded table in full, then the
// cases no golden file holds (every other entry point of every source the library is built from), a self-test of the stream check, and the
// kernels no case launched.  --kernel-names: the table's kernels under the names the L lines show.
//
// Pointers are made up (argument k of a call sits at k << 40, nothing is ever dereferenced), so the argument hashes are
// the same from run to run.  tests/golden/make_golden_launch_sequences.py builds and runs this; the cases are named by their
// arguments, and a name never changes meaning: new cases get new names.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <set>
#include <string>

#include "meshraster_hip.h"

extern "C" {
void rec_load_args(const char* path);
void rec_set_device(int device, int devices);
void rec_set_cus(int cus);
void rec_begin(void);
void rec_expect_stream(void* stream);
void rec_report_unlaunched(void);
void rec_print_kernel_names(void);
}

namespace {

// The stream every case hands to the entry point it calls: NULL as recorded, or the value of --stream (never dereferenced).
mr_stream_t g_stream = nullptr;

template <typename T = float>
T* P(int k) { return reinterpret_cast<T*>(static_cast<uintptr_t>(k) << 40); }

// The launchers' parameter blocks live on the stack.  A block whose padding bytes are not initialised hashes to whatever the
// stack held: --stack-fill sets that byte, and a record that differs between two fills (or two runs) names such a block.
int g_stack_fill = 0;
__attribute__((noinline)) void scrub_stack() {
    volatile char pad[96 * 1024];
    for (size_t i = 0; i < sizeof pad; i++) pad[i] = (char)g_stack_fill;
}

void begin(const char* fmt, ...) {
    char name[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    // (a field at its usual value is left out of the name)
    static const char* const usual[] = {"fl0", "tb-1", "eps0.001", "tx24", "ok1", "crit0", "hw0x0", "ws-0", "bs-0", "cap+0", "cj3", "dt0/0", "dt0",
                                        "work1", "fg1", "vid1", "gf1", "ts2", "fb1", "out1", "stored1", "hit1"};
    std::string shown;
    for (char* tok = std::strtok(name, " "); tok; tok = std::strtok(nullptr, " ")) {
        bool skip = false;
        for (const char* u : usual) skip = skip || !std::strcmp(tok, u);
        if (!skip) shown += (shown.empty() ? "" : " ") + std::string(tok);
    }
    std::printf("# %s\n", shown.c_str());
    rec_begin();
    scrub_stack();
}
void end(int rc) { std::printf("R %d\n", rc); }  // (a refused call shows as a status with no line in front of it)

constexpr float NEAR = 0.1f, FAR = 100.0f, EPS = 1e-3f;
const int BATCHES[] = {0, 1, 2, 16, 64, 128};
const int FACES[] = {0, 255, 1538, 7104};
const int RASTERS[] = {36, 256, 480, 640, 9000};  // (9000: 282 x 1125 tiles, more than the bins a workgroup counts: ysh > 0)
const int FWD_FLAGS[] = {0, MR_FLAG_REFERENCE_ALGO, MR_FLAG_TILE_PER_WORKGROUP, MR_FLAG_ONE_WORKGROUP_PER_IMAGE, MR_FLAG_FORCE_PARTS,
                         MR_FLAG_PARTS_IN_ONE_LAUNCH, MR_FLAG_FORCE_PARTS | MR_FLAG_PARTS_IN_ONE_LAUNCH, MR_FLAG_PLAIN_DIVISIONS};

// ---- forward renders -------------------------------------------------------------------------------------------------
struct Fwd {
    int B = 2, V = 2000, F0 = 1538, fill = 1, is = 256, flags = 0, tile_bound = 0;
    bool inv_map = false, records = false, vid = true, zero_fill = false, lut = false;
    int64_t ws_short = 0;
    float eps = EPS;
    int bg_stride = 3, texel = MR_TEXEL_LAYOUT_DEFAULT, ts = 2;
};

int render_forward(const Fwd& c) {
    const int64_t ws = mr_render_workspace_bytes(c.B, c.F0, c.is) - c.ws_short;
    return mr_render_forward(P(1), P(2), P(3), c.bg_stride, P(4), P(5), P(6), P<int32_t>(7), P(8), c.inv_map ? P(9) : nullptr, P<void>(10), ws,
                             c.B, c.F0, c.is, c.ts, NEAR, FAR, c.eps, 1, 1, 1, c.flags, g_stream);
}
int render_vc_forward(const Fwd& c) {
    const int64_t ws = mr_render_workspace_bytes(c.B, c.fill ? 2 * c.F0 : c.F0, c.is) - c.ws_short;
    return mr_render_vc_forward(P(1), P<int32_t>(2), P(3), P(4), c.bg_stride, P(5), P(6), P(7), P<int32_t>(8), P(9), P<void>(10), ws, c.B, c.V,
                                c.F0, c.fill, c.is, NEAR, FAR, c.eps, 1, 1, 1, c.flags, c.texel, g_stream);
}
int render_flow_forward(const Fwd& c) {
    const int64_t ws = mr_render_workspace_bytes(c.B, c.fill ? 2 * c.F0 : c.F0, c.is) - c.ws_short;
    const bool hit = (c.flags & MR_FLAG_SPARSE_TILES) != 0;
    return mr_render_flow_forward(P(1), P<int32_t>(2), P(3), P(4), c.bg_stride, c.lut ? P(5) : nullptr, c.lut ? 4 : 0, 0.5f, P(6), P(7), P(8),
                                  P(9), P(10), P<int32_t>(11), hit ? P<uint8_t>(12) : nullptr, P<void>(13), ws, c.B, c.V, c.F0, c.fill, c.is,
                                  NEAR, FAR, c.eps, c.flags, c.vid ? P<int32_t>(14) : nullptr, c.tile_bound, P<uint32_t>(15),
                                  c.zero_fill ? P(16) : nullptr, c.zero_fill ? (int64_t)c.B * c.V * 3 : 0, c.texel, g_stream);
}

void fwd_case(const char* which, const Fwd& c) {
    // (the sweeps below cross at some shapes: a case is recorded where it comes up first)
    static std::set<std::string> seen;
    char key[128];
    std::snprintf(key, sizeof key, "%s %d %d %d %d %x %d %d %d", which, c.B, c.F0, c.fill, c.is, (unsigned)c.flags, c.tile_bound, (int)c.inv_map,
                  (int)c.zero_fill);
    if (!seen.insert(key).second) return;
    begin("%s B%d F%d fb%d is%d fl%x tb%d%s%s", which, c.B, c.F0, c.fill, c.is, (unsigned)c.flags, c.tile_bound, c.inv_map ? " inv" : "",
          c.zero_fill ? " zf" : "");
    end(which[0] == 'r' ? render_forward(c) : which[0] == 'v' ? render_vc_forward(c) : render_flow_forward(c));
}

void forward_cases(bool all) {
    const int SPARSE = MR_FLAG_SPARSE_TILES | MR_FLAG_TILE_LIST_CLEARED;
    // the listed flow render with the per-face pass inside the binning pass -- the training path, and the one launch whose parts
    // follow batch, mesh and device: every batch x mesh at the metric raster, the larger rasters where the parts change
    for (int B : BATCHES)
        for (int F0 : FACES)
            for (int fill = 1; fill >= 0; fill--) {
                if (!fill && F0 != 1538 && F0 != 7104) continue;
                Fwd c; c.B = B; c.F0 = F0; c.fill = fill; c.flags = SPARSE; c.tile_bound = -1;
                fwd_case("flow", c);
            }
    for (int is : {480, 640})
        for (int B : {1, 16, 64})
            for (int one_launch = 0; one_launch < 2; one_launch++) {
                Fwd c; c.B = B; c.F0 = 7104; c.is = is; c.flags = SPARSE | (one_launch ? MR_FLAG_PARTS_IN_ONE_LAUNCH : 0); c.tile_bound = -1;
                fwd_case("flow", c);
            }
    // the dense launches: their binning pass takes parts only where the bins are many (640 x 640) or the caller forces them
    for (const char* which : {"render", "vc", "flow"}) {
        const bool generic = which[0] == 'r';
        for (int B : BATCHES)
            for (int F0 : FACES) {
                if (!all && (F0 == 0 || F0 == 255 || B == 0)) continue;
                Fwd c; c.B = B; c.F0 = F0; c.fill = generic ? 0 : 1;
                if (all || !generic) fwd_case(which, c);
                if ((B == 16 || B == 64) && F0 == 7104) { c.is = 640; fwd_case(which, c); }
            }
    }
    for (const char* which : {"vc", "flow"})
        for (int B : {2, 16}) {
            Fwd c; c.B = B; c.F0 = 7104; c.is = 480; c.flags = MR_FLAG_FORCE_PARTS;
            fwd_case(which, c);
            c.flags |= MR_FLAG_PARTS_IN_ONE_LAUNCH; fwd_case(which, c);
        }
    if (!all) return;
    for (const char* which : {"render", "vc", "flow"}) {
        const bool flow = which[0] == 'f', generic = which[0] == 'r';
        for (int is : RASTERS)
            for (int B : {1, 16}) {
                if (is == 256 || (is == 9000 && B != 1)) continue;
                Fwd c; c.B = B; c.F0 = 1538; c.is = is; c.fill = generic ? 0 : 1;
                fwd_case(which, c);
                if (flow) { c.flags = SPARSE; c.tile_bound = -1; fwd_case(which, c); }
            }
        for (int flags : FWD_FLAGS)
            for (int is : {36, 480}) {
                Fwd c; c.B = 16; c.F0 = 7104; c.is = is; c.flags = flags; c.fill = generic ? 0 : 1;
                if (flags != 0) fwd_case(which, c);
                if (flow && !(flags & MR_FLAG_REFERENCE_ALGO)) { c.flags = flags | SPARSE; c.tile_bound = -1; fwd_case(which, c); }
            }
    }
    // the sparse-tile launch of the flow render: without a bound (no list), with the caller's bound, header cleared or not
    for (int B : {2, 64})
        for (int tb : {0, -1, 100, 5, 1 << 30})
            for (int cleared : {0, 1}) {
                Fwd c; c.B = B; c.is = 480; c.flags = MR_FLAG_SPARSE_TILES | (cleared ? MR_FLAG_TILE_LIST_CLEARED : 0); c.tile_bound = tb;
                fwd_case("flow", c);
            }
    { Fwd c; c.flags = MR_FLAG_TILE_LIST_CLEARED; fwd_case("flow", c); }
    { Fwd c; c.zero_fill = true; c.flags = SPARSE; c.tile_bound = -1; fwd_case("flow", c); }
    { Fwd c; c.zero_fill = true; c.B = 0; fwd_case("flow", c); }
    { Fwd c; c.F0 = 0; c.flags = MR_FLAG_SPARSE_TILES; c.tile_bound = -1; fwd_case("flow", c); }
    // a mesh whose boxes do not fit LDS: the per-face pass stays a launch of its own
    { Fwd c; c.F0 = 20000; fwd_case("vc", c); c.flags = SPARSE; c.tile_bound = -1; fwd_case("flow", c); c.B = 128; fwd_case("flow", c); }
    { Fwd c; c.inv_map = true; fwd_case("render", c); }
    { Fwd c; c.fill = 0; c.B = 65536; c.F0 = 1; c.is = 8; fwd_case("vc", c); }
}

void forward_refusals() {
    Fwd ok;
    auto refuse = [&](const char* which, const char* why, Fwd c) {
        begin("%s refused: %s", which, why);
        end(which[0] == 'r' ? render_forward(c) : which[0] == 'v' ? render_vc_forward(c) : render_flow_forward(c));
    };
    for (const char* which : {"render", "vc", "flow"}) {
        Fwd c = ok; c.B = -1; refuse(which, "negative batch", c);
        c = ok; c.is = 16385; refuse(which, "raster past 16384", c);
        c = ok; c.is = 0; refuse(which, "raster 0", c);
        c = ok; c.ws_short = 1; refuse(which, "workspace one byte short", c);
        c = ok; c.bg_stride = 1; refuse(which, "background stride", c);
    }
    Fwd c = ok; c.ts = 1; refuse("render", "texture size 1", c);
    c = ok; c.eps = 1e-7f; refuse("vc", "eps below 1e-6", c);
    c = ok; c.eps = 1e-7f; refuse("flow", "eps below 1e-6", c);
    c = ok; c.texel = 0x3f; refuse("vc", "texel layout", c);
    c = ok; c.texel = 0x3f; refuse("flow", "texel layout", c);
    c = ok; c.B = 65536; c.F0 = 1; c.is = 8; refuse("flow", "batch past 65535", c);
    begin("flow refused: sparse tiles without coverage bytes");
    end(mr_render_flow_forward(P(1), P<int32_t>(2), P(3), P(4), 3, nullptr, 0, 0.5f, P(6), P(7), P(8), P(9), P(10), P<int32_t>(11), nullptr,
                               P<void>(13), mr_render_workspace_bytes(2, 3076, 256), 2, 2000, 1538, 1, 256, NEAR, FAR, EPS,
                               MR_FLAG_SPARSE_TILES, nullptr, -1, nullptr, nullptr, 0, MR_TEXEL_LAYOUT_DEFAULT, g_stream));
    begin("flow refused: vertex ids without weights");
    end(mr_render_flow_forward(P(1), P<int32_t>(2), P(3), P(4), 3, nullptr, 0, 0.5f, P(6), P(7), P(8), P(9), nullptr, P<int32_t>(11), nullptr,
                               P<void>(13), mr_render_workspace_bytes(2, 3076, 256), 2, 2000, 1538, 1, 256, NEAR, FAR, EPS, 0,
                               P<int32_t>(14), 0, nullptr, nullptr, 0, MR_TEXEL_LAYOUT_DEFAULT, g_stream));
    begin("flow refused: lookup table without entries");
    end(mr_render_flow_forward(P(1), P<int32_t>(2), P(3), P(4), 3, P(5), 0, 0.5f, P(6), P(7), P(8), P(9), P(10), P<int32_t>(11), nullptr,
                               P<void>(13), mr_render_workspace_bytes(2, 3076, 256), 2, 2000, 1538, 1, 256, NEAR, FAR, EPS, 0, nullptr, 0,
                               nullptr, nullptr, 0, MR_TEXEL_LAYOUT_DEFAULT, g_stream));
    begin("flow refused: zero fill without a buffer");
    end(mr_render_flow_forward(P(1), P<int32_t>(2), P(3), P(4), 3, nullptr, 0, 0.5f, P(6), P(7), P(8), P(9), P(10), P<int32_t>(11), nullptr,
                               P<void>(13), mr_render_workspace_bytes(2, 3076, 256), 2, 2000, 1538, 1, 256, NEAR, FAR, EPS, 0, nullptr, 0,
                               nullptr, nullptr, 5, MR_TEXEL_LAYOUT_DEFAULT, g_stream));
    begin("render refused: no face index map");
    end(mr_render_forward(P(1), P(2), P(3), 3, P(4), P(5), P(6), nullptr, P(8), nullptr, P<void>(10), mr_render_workspace_bytes(2, 10, 36), 2, 10,
                          36, 2, NEAR, FAR, EPS, 1, 1, 1, 0, g_stream));
    begin("render refused: alpha without an image");
    end(mr_render_forward(P(1), P(2), P(3), 3, P(4), nullptr, P(6), P<int32_t>(7), P(8), nullptr, P<void>(10),
                          mr_render_workspace_bytes(2, 10, 36), 2, 10, 36, 2, NEAR, FAR, EPS, 1, 1, 1, 0, g_stream));
    begin("vc refused: depth without an image");
    end(mr_render_vc_forward(P(1), P<int32_t>(2), P(3), P(4), 3, P(5), P(6), nullptr, P<int32_t>(8), P(9), P<void>(10),
                             mr_render_workspace_bytes(2, 20, 36), 2, 30, 10, 1, 36, NEAR, FAR, EPS, 1, 1, 1, 0, MR_TEXEL_LAYOUT_DEFAULT, g_stream));
    begin("vc refused: no vertices");
    end(mr_render_vc_forward(nullptr, P<int32_t>(2), P(3), P(4), 3, P(5), P(6), P(7), P<int32_t>(8), P(9), P<void>(10),
                             mr_render_workspace_bytes(2, 20, 36), 2, 30, 10, 1, 36, NEAR, FAR, EPS, 1, 1, 1, 0, MR_TEXEL_LAYOUT_DEFAULT, g_stream));
}

// ---- the pair step ---------------------------------------------------------------------------------------------------
MrPairStep pair_step(int B, int va, int vb, int fh, int fo, int is, int flags, int criterion, int reserved) {
    MrPairStep s;
    std::memset(&s, 0, sizeof s);
    s.batch_size = B; s.num_verts_a = va; s.num_verts_b = vb; s.num_hand_faces = fh; s.num_obj_faces = fo; s.hand_faces_batched = 0;
    s.fill_back = 1; s.image_size = is; s.height = is; s.width = is; s.jitter_channels = 3; s.cam_batched = 1;
    s.n_lut = 0; s.bg_stride = 0; s.texel_layout = MR_TEXEL_LAYOUT_DEFAULT; s.want_grad = 1; s.mean_of = 0; s.flags = flags;
    s.criterion = criterion; s.reserved = reserved;
    s.orig_size = 256.0f; s.near_ = NEAR; s.far_ = FAR; s.eps = EPS; s.alpha_thresh = 0.5f; s.distance_thresh = 0.05f; s.warp_thresh = 1.0f;
    s.pair_thresh = 0.5f;
    s.verts1a = P(1); s.verts1b = P(2); s.verts2a = P(3); s.verts2b = P(4); s.K1 = P(5); s.K2 = P(6); s.R = P(7); s.t = P(8);
    s.dist_coeffs = P(9); s.hand_faces = P<int64_t>(10); s.obj_faces = P<int64_t>(11); s.keep_lut = nullptr; s.background = P(12);
    s.image_ref = P(13); s.image = P(14); s.jitter_ref = P(15); s.jitter = P(16); s.scratch = P<void>(17); s.saved = P<void>(18);
    int64_t th = 0;
    if (mr_pair_step_sizes(&s, &s.scratch_bytes, &s.saved_bytes, &th) != MR_OK) { s.scratch_bytes = 0; s.saved_bytes = 0; }
    s.flows = P(19); s.losses = P(20); s.tile_count_out = P<uint32_t>(21); s.tile_bound = 0;
    s.grad_loss_fwd = P(22); s.grad_loss_bwd = P(23); s.grad_loss_sum = nullptr; s.grad_mean = nullptr;
    s.grad_verts1a = P(24); s.grad_verts1b = P(25); s.grad_verts2a = P(26); s.grad_verts2b = P(27);
    return s;
}

void pair_step_cases(bool all) {
    struct Mesh { int va, vb, fh, fo; };
    // the metric mesh (prologue inside the binning pass), one of one side only, and one whose vertices do not fit LDS next
    // to the boxes (prologue as a launch of its own)
    const Mesh meshes[] = {{778, 1000, 1538, 2000}, {778, 8, 1538, 12}, {0, 3, 0, 1}, {778, 1782, 1538, 9000}};
    const int dtypes[] = {0, MR_DTYPE_BF16 | MR_DTYPE_U8 << 8, MR_DTYPE_BF16 | MR_DTYPE_F32 << 8};
    auto both = [&](const char* what, MrPairStep s) {
        begin("pair_step_forward %s B%d V%d+%d F%d+%d is%d fl%x crit%d dt%x tb%lld", what, s.batch_size, s.num_verts_a, s.num_verts_b,
              s.num_hand_faces, s.num_obj_faces, s.image_size, (unsigned)s.flags, s.criterion, (unsigned)s.reserved, (long long)s.tile_bound);
        end(mr_pair_step_forward(&s, g_stream));
        begin("pair_step_backward %s B%d V%d+%d F%d+%d is%d fl%x crit%d dt%x", what, s.batch_size, s.num_verts_a, s.num_verts_b, s.num_hand_faces,
              s.num_obj_faces, s.image_size, (unsigned)s.flags, s.criterion, (unsigned)s.reserved);
        end(mr_pair_step_backward(&s, g_stream));
    };
    for (const Mesh& m : meshes)
        for (int B : {0, 1, 8, 32, 64})
            for (int is : {256, 480, 640})
                for (int flags : {MR_PAIR_STEP_LIST_CLEAN, 0}) {
                    const bool metric = &m == &meshes[0];
                    if (!flags && (B != 8 || is == 640 || !all)) continue;
                    if (!metric && (!all || B == 0 || B == 32 || is == 480)) continue;
                    if (!all && B == 0) continue;
                    both("", pair_step(B, m.va, m.vb, m.fh, m.fo, is, flags, MR_CRITERION_L1, 0));
                }
    if (!all) return;
    for (int flags : {MR_PAIR_STEP_SEPARATE_LAUNCHES, MR_PAIR_STEP_SEPARATE_LAUNCHES | MR_PAIR_STEP_LIST_CLEAN, MR_PAIR_STEP_GRAD_BUFFER_USED})
        for (int B : {8, 64}) both("", pair_step(B, 778, 1000, 1538, 2000, 256, flags, MR_CRITERION_L1, 0));
    for (int crit : {MR_CRITERION_L1, MR_CRITERION_L2})
        for (int dt : dtypes) both("", pair_step(16, 778, 1000, 1538, 2000, 256, MR_PAIR_STEP_LIST_CLEAN, crit, dt));
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.tile_bound = 1000; both("bound", s); }
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.want_grad = 0; both("no gradient", s); }
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.grad_loss_fwd = nullptr; s.grad_loss_bwd = nullptr; s.grad_mean = P(28);
      s.mean_of = 8; both("mean", s); }
    // (a loss that uses loss_bwd alone: the backward call is made with that one incoming gradient, and launches)
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.grad_loss_fwd = nullptr; both("bwd-only", s); }
    // one argument off each (named by what is off: the forward and the backward call do not refuse the same ones)
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.scratch_bytes -= 1; both("scratch-1", s); }
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.saved_bytes -= 1; both("saved-1", s); }
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.image = nullptr; s.K1 = nullptr; both("no-image-no-K1", s); }
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.orig_size = 0.0f; both("orig_size-0", s); }
    { MrPairStep s = pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, 0); s.eps = 0.0f; both("eps-0", s); }
    both("criterion-2", pair_step(8, 778, 1000, 1538, 2000, 256, 0, 2, 0));
    both("f32-image-u8-mask", pair_step(8, 778, 1000, 1538, 2000, 256, 0, 0, MR_DTYPE_F32 | MR_DTYPE_U8 << 8));
    both("raster-258", pair_step(8, 778, 1000, 1538, 2000, 258, 0, 0, 0));
    both("vertices-2778", pair_step(8, 778, 2000, 1538, 2000, 256, 0, 0, 0));
    both("batch--1", pair_step(-1, 778, 1000, 1538, 2000, 256, 0, 0, 0));
    begin("pair_step_forward refused: null block");
    end(mr_pair_step_forward(nullptr, g_stream));
    begin("pair_step_backward refused: null block");
    end(mr_pair_step_backward(nullptr, g_stream));
}

// ---- the generic backward ---------------------------------------------------------------------------------------------
struct Bwd {
    int B = 2, F = 1538, is = 256, ts = 2, rr = 1, ra = 1, rd = 1, flags = 0;
    bool tex = true, grad_faces = true;
    int ws = 2;  // 0 none, 1 list-sized, 2 full
    float eps = EPS;
};
int render_backward(const Bwd& c) {
    const int64_t ws = c.ws == 2 ? mr_render_backward_workspace_bytes(c.B, c.F, c.is) : c.ws == 1 ? mr_render_backward_list_workspace_bytes(c.B, c.F) : 0;
    return mr_render_backward(P(1), P(2), P<int32_t>(3), P(4), P(5), P(6), P(7), P(8), c.grad_faces ? P(9) : nullptr, c.tex ? P(10) : nullptr,
                              c.ws ? P<void>(11) : nullptr, ws, c.B, c.F, c.is, c.ts, NEAR, FAR, c.eps, c.rr, c.ra, c.rd, c.flags, g_stream);
}
void bwd_case(const Bwd& c) {
    begin("render_backward B%d F%d is%d ts%d rgb%d a%d d%d tex%d gf%d ws%d fl%x eps%g", c.B, c.F, c.is, c.ts, c.rr, c.ra, c.rd, (int)c.tex,
          (int)c.grad_faces, c.ws, (unsigned)c.flags, (double)c.eps);
    end(render_backward(c));
}
void backward_cases() {
    for (int rr = 0; rr < 2; rr++)
        for (int ra = 0; ra < 2; ra++)
            for (int rd = 0; rd < 2; rd++)
                for (int tex = 0; tex < 2; tex++)
                    for (int ws = 0; ws < 3; ws++) {
                        Bwd c; c.rr = rr; c.ra = ra; c.rd = rd; c.tex = tex != 0; c.ws = ws;
                        bwd_case(c);
                    }
    for (int ws = 0; ws < 3; ws++)
        for (int rd = 1; rd >= (ws == 2 ? 0 : 1); rd--) {
            Bwd c; c.ws = ws; c.rd = rd;
            c.ts = 4; bwd_case(c);
            c.ts = 2; c.eps = 1e-7f; bwd_case(c);
            c.eps = 1e-6f; bwd_case(c);
            c.eps = EPS; c.flags = MR_FLAG_REFERENCE_ALGO; bwd_case(c);
            c.flags = MR_FLAG_COUNT_PIXEL_MAP_TERMS; bwd_case(c);
            c.flags = 0; c.grad_faces = false; bwd_case(c);
        }
    // rasters: a pixel or two, one no multiple of four, the strips' three line counts, one whose lines do not fit LDS
    for (int is : {1, 2, 3, 36, 480, 640, 1024, 2048, 4096, 8192, 16384})
        for (int ws : {0, 2})
            for (int rd = 1; rd >= (ws == 2 && is <= 36 ? 0 : 1); rd--) {
                Bwd c; c.is = is; c.ws = ws; c.rd = rd; c.B = is > 2048 ? 1 : 2; c.F = is > 2048 ? 255 : 1538;
                bwd_case(c);
            }
    for (int B : {0, 1, 16, 128})
        for (int F : {0, 255, 7104}) {
            Bwd c; c.B = B; c.F = F;
            bwd_case(c);
        }
    { Bwd c; c.B = 1; c.F = 1 << 24; c.is = 8; bwd_case(c); }  // owner numbers past 24 bits: no strips
    { Bwd c; c.B = -1; bwd_case(c); }
    { Bwd c; c.is = 0; bwd_case(c); }
    { Bwd c; c.ts = 1; bwd_case(c); }
    begin("render_backward refused: no faces");
    end(mr_render_backward(nullptr, P(2), P<int32_t>(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10), nullptr, 0, 2, 10, 36, 2, NEAR, FAR, EPS, 1, 1, 1, 0, g_stream));

    for (int rr = 0; rr < 2; rr++)
        for (int ra = 0; ra < 2; ra++)
            for (int is : {1, 2, 36, 256, 480, 8192}) {
                begin("backward_pixel_map B2 F1538 is%d rgb%d a%d", is, rr, ra);
                end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), P(7), 2, 1538, is, EPS, rr, ra, g_stream));
            }
    for (int B : {0, 16})
        for (int F : {0, 7104}) {
            begin("backward_pixel_map B%d F%d is256 rgb1 a1", B, F);
            end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), P(7), B, F, 256, EPS, 1, 1, g_stream));
        }
    begin("backward_pixel_map refused: no gradient array");
    end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), nullptr, 2, 10, 36, EPS, 1, 1, g_stream));
    begin("backward_pixel_map refused: rgb without its maps");
    end(mr_backward_pixel_map(P(1), P<int32_t>(2), nullptr, P(4), P(5), P(6), P(7), 2, 10, 36, EPS, 1, 1, g_stream));
    begin("backward_pixel_map refused: alpha without its maps");
    end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), nullptr, P(7), 2, 10, 36, EPS, 1, 1, g_stream));
    begin("backward_pixel_map refused: raster 0");
    end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), P(7), 2, 10, 0, EPS, 1, 1, g_stream));
}

// ---- the vertex-colour and tile-scatter backwards ----------------------------------------------------------------------
void vc_backward_cases() {
    auto run = [&](int B, int V, int F0, int is, int flags, bool stored, float eps, int texel, bool out) {
        begin("render_vc_backward B%d V%d F%d is%d fl%x stored%d eps%g tx%x out%d", B, V, F0, is, (unsigned)flags, (int)stored, (double)eps,
              (unsigned)texel, (int)out);
        end(mr_render_vc_backward(P(1), P<int32_t>(2), P<int32_t>(3), stored ? P(4) : nullptr, stored ? P(5) : nullptr, P(6), out ? P(7) : nullptr, B,
                                  V, F0, 1, is, eps, flags, texel, g_stream));
    };
    const int T = MR_TEXEL_LAYOUT_DEFAULT;
    for (int V : {0, 1, 2000, 2560, 2561, 5000})  // (2560 vertices: the last table inside the LDS limit)
        for (int flags : {0, MR_FLAG_FORCE_GATHER})
            for (int stored = 0; stored < 2; stored++) run(2, V, 1538, 256, flags, stored != 0, EPS, T, true);
    for (int B : {0, 1, 64})
        for (int is : {36, 480, 640}) run(B, 2000, 1538, is, 0, true, EPS, T, true);
    run(2, 2000, 0, 256, 0, true, EPS, T, true);
    run(2, 5000, 1538, 8193, 0, true, EPS, T, true);  // the gather's 13-bit box offsets
    run(2, 5000, 1538, 8192, 0, true, EPS, T, true);
    run(-1, 2000, 1538, 256, 0, true, EPS, T, true);
    run(2, 2000, 1538, 256, 0, true, EPS, 0, true);     // (code 0: the default layout)
    run(2, 2000, 1538, 256, 0, true, EPS, 0x3f, true);  // (no permutation: refused)
    run(2, 2000, 1538, 256, 0, true, 1e-7f, T, true);
    run(2, 2000, 1538, 256, 0, true, EPS, T, false);
}

void scatter_cases() {
    const int T = MR_TEXEL_LAYOUT_DEFAULT;
    struct S { int B = 4, V = 2000, F0 = 1538, is = 256, flags = 0, H = 0, W = 0, crit = 0; bool vid = true, flowgrad = true, work = true, ok = true;
               float eps = EPS; int texel = MR_TEXEL_LAYOUT_DEFAULT; };
    auto name = [&](const char* which, const S& c) {
        begin("%s B%d V%d F%d is%d fl%x vid%d fg%d work%d crit%d hw%dx%d ok%d eps%g tx%x", which, c.B, c.V, c.F0, c.is, (unsigned)c.flags, (int)c.vid,
              (int)c.flowgrad, (int)c.work, c.crit, c.H, c.W, (int)c.ok, (double)c.eps, (unsigned)c.texel);
    };
    auto flow_backward = [&](S c) {
        name("render_flow_backward", c);
        const int H = c.H ? c.H : c.is, W = c.W ? c.W : c.is;
        end(mr_render_flow_backward(c.ok ? P(1) : nullptr, P<int32_t>(2), P<int32_t>(3), P<uint32_t>(4), P(5), c.ok ? P(6) : nullptr,
                                    c.flowgrad ? nullptr : P(7), P(8), P(9), P(10), P(11), c.B / 2, P(12), H, W, P(13), c.B, c.V, c.F0, 1, c.is, c.eps,
                                    c.flags, c.vid ? P<int32_t>(14) : nullptr, c.texel, P(15), g_stream));
    };
    auto pair_tiles = [&](S c, bool crit_entry) {
        name(crit_entry ? "flow_pair_backward_tiles_crit" : "flow_pair_backward_tiles", c);
        const int H = c.H ? c.H : c.is, W = c.W ? c.W : c.is;
        if (crit_entry)
            end(mr_flow_pair_backward_tiles_crit(P<int32_t>(1), P<uint32_t>(2), P(3), c.vid ? P<int32_t>(4) : nullptr, c.ok ? P(5) : nullptr, P(6), P(7),
                                                 P(8), P(9), 3, P(10), P(11), P(12), P(13), P(14), P(15), P(16), P(17), H, W, P(18), c.B, c.V, c.F0, 1,
                                                 c.is, c.eps, 0.5f, c.flags, c.texel, g_stream, c.crit));
        else
            end(mr_flow_pair_backward_tiles(P<int32_t>(1), P<uint32_t>(2), P(3), c.vid ? P<int32_t>(4) : nullptr, c.ok ? P(5) : nullptr, P(6), P(7), P(8),
                                            P(9), 3, P(10), P(11), P(12), P(13), P(14), P(15), P(16), P(17), H, W, P(18), c.B, c.V, c.F0, 1, c.is,
                                            c.eps, 0.5f, c.flags, c.texel, g_stream));
    };
    auto unit_tiles = [&](S c) {
        name("flow_pair_backward_unit_tiles", c);
        const int H = c.H ? c.H : c.is, W = c.W ? c.W : c.is;
        end(mr_flow_pair_backward_unit_tiles(P<int32_t>(1), P<uint32_t>(2), P(3), c.vid ? P<int32_t>(4) : nullptr, c.ok ? P(5) : nullptr, P(6), P(7),
                                             P(8), P(9), H, W, P(10), c.B, c.V, c.F0, 1, c.is, c.eps, c.flags, c.texel,
                                             c.work ? P<void>(11) : nullptr, g_stream));
    };
    for (int is : {256, 480, 640})
        for (int vid = 0; vid < 2; vid++)
            for (int flags : {0, MR_FLAG_OUTPUT_ZEROED}) {
                S c; c.is = is; c.vid = vid != 0; c.flags = flags;
                flow_backward(c);
                if (!flags) { c.flowgrad = false; flow_backward(c); c.flowgrad = true; }
                if (!flags && is == 256) pair_tiles(c, false);
                c.crit = flags ? 1 : 0; pair_tiles(c, true); c.crit = 0;
                unit_tiles(c);
                if (!flags) { c.work = false; unit_tiles(c); }
            }
    for (int is : {32, 128, 1024}) {  // one tile row, 64 tiles, the most tiles the covered-tile list holds
        S c; c.is = is; c.B = 64;
        flow_backward(c); pair_tiles(c, true); unit_tiles(c);
    }
    for (int B : {0, 2, 128}) {
        S c; c.B = B;
        flow_backward(c); pair_tiles(c, true); unit_tiles(c);
    }
    { S c; c.V = 0; flow_backward(c); pair_tiles(c, true); unit_tiles(c); }
    { S c; c.F0 = 0; flow_backward(c); pair_tiles(c, true); unit_tiles(c); c.flags = MR_FLAG_OUTPUT_ZEROED; unit_tiles(c); }
    { S c; c.V = 3840; flow_backward(c); c.flowgrad = false; flow_backward(c); c.V = 2561; flow_backward(c); }  // the table's limit, two and three sums
    // refusals
    { S c; c.B = 3; pair_tiles(c, true); unit_tiles(c); c.B = -2; flow_backward(c); }
    { S c; c.is = 258; flow_backward(c); pair_tiles(c, true); unit_tiles(c); }
    { S c; c.is = 1056; flow_backward(c); pair_tiles(c, true); unit_tiles(c); }
    { S c; c.V = 3841; flow_backward(c); pair_tiles(c, true); unit_tiles(c); }
    { S c; c.ok = false; flow_backward(c); pair_tiles(c, true); unit_tiles(c); c.vid = false; flow_backward(c); }
    { S c; c.eps = 1e-7f; flow_backward(c); pair_tiles(c, true); unit_tiles(c); }
    { S c; c.texel = 0x3f; flow_backward(c); pair_tiles(c, true); unit_tiles(c); }
    { S c; c.H = 300; flow_backward(c); pair_tiles(c, true); unit_tiles(c); c.H = 0; c.W = 1; pair_tiles(c, true); unit_tiles(c); }
    { S c; c.crit = 2; pair_tiles(c, true); }
    begin("flow_pair_backward_unit_tiles refused: no loss gradient");
    end(mr_flow_pair_backward_unit_tiles(P<int32_t>(1), P<uint32_t>(2), P(3), P<int32_t>(4), P(5), P(6), P(7), nullptr, P(9), 256, 256, P(10), 4, 2000,
                                         1538, 1, 256, EPS, 0, T, nullptr, g_stream));
    begin("render_flow_backward refused: no output");
    end(mr_render_flow_backward(P(1), P<int32_t>(2), P<int32_t>(3), P<uint32_t>(4), P(5), P(6), nullptr, P(8), P(9), P(10), P(11), 2, P(12), 256, 256,
                                nullptr, 4, 2000, 1538, 1, 256, EPS, 0, P<int32_t>(14), T, P(15), g_stream));
}

// ---- the warp half: listed forward launches, occlusion, pair loss ---------------------------------------------------------
struct Pair {
    int B = 4, is = 256, H = 0, W = 0, crit = 0, idt = 0, mdt = 0, Cj = 3;
    int64_t tile_bound = -1, cap_off = 0, ws_short = 0, bstride_short = 0;
    bool ok = true;
};
int64_t pair_cap(const Pair& c) { return 2LL * c.B * ((c.is + 31) / 32) * ((c.is + 7) / 8) + c.cap_off; }

void pair_forward_cases() {
    auto name = [&](const char* which, const Pair& c) {
        begin("%s B%d is%d hw%dx%d crit%d dt%d/%d cj%d tb%lld cap%+lld ws-%lld bs-%lld ok%d", which, c.B, c.is, c.H, c.W, c.crit, c.idt, c.mdt, c.Cj,
              (long long)c.tile_bound, (long long)c.cap_off, (long long)c.ws_short, (long long)c.bstride_short, (int)c.ok);
    };
    // which: 0 tiles, 1 tiles_crit, 2 tiles_typed, 3 grad_tiles, 4 grad_tiles_crit, 5 grad_tiles_typed
    auto forward = [&](int which, Pair c) {
        static const char* names[] = {"flow_pair_forward_tiles", "flow_pair_forward_tiles_crit", "flow_pair_forward_tiles_typed",
                                      "flow_pair_forward_grad_tiles", "flow_pair_forward_grad_tiles_crit", "flow_pair_forward_grad_tiles_typed"};
        name(names[which], c);
        const int H = c.H ? c.H : c.is, W = c.W ? c.W : c.is;
        const int64_t bs = 3LL * c.is * c.is - c.bstride_short, ws = mr_pair_consist_tiles_workspace_bytes(c.B, c.is) - c.ws_short, cap = pair_cap(c);
        float* f12 = c.ok ? P(3) : nullptr;
#define FWD_HEAD P(1), P(2), f12, P(4), bs, P(5), P(6), P(7), P(8), P(9), P(10), P<uint8_t>(11), P<uint8_t>(12)
#define FWD_TAIL c.Cj, P<void>(17), ws, P(18), P(19), P(20), c.B, c.is, H, W, 0.05f, 1.0f, 0.5f, P<void>(21), P<void>(22), cap, c.tile_bound
        switch (which) {
        case 0: end(mr_flow_pair_forward_tiles(FWD_HEAD, P(13), P(14), P(15), P(16), FWD_TAIL, g_stream)); break;
        case 1: end(mr_flow_pair_forward_tiles_crit(FWD_HEAD, P(13), P(14), P(15), P(16), FWD_TAIL, g_stream, c.crit)); break;
        case 2: end(mr_flow_pair_forward_tiles_typed(FWD_HEAD, P<void>(13), P<void>(14), P<void>(15), P<void>(16), FWD_TAIL, g_stream, c.crit, c.idt, c.mdt)); break;
        case 3: end(mr_flow_pair_forward_grad_tiles(FWD_HEAD, P(13), P(14), P(15), P(16), FWD_TAIL, P(23), P(24), P(25), P<void>(26), g_stream)); break;
        case 4: end(mr_flow_pair_forward_grad_tiles_crit(FWD_HEAD, P(13), P(14), P(15), P(16), FWD_TAIL, P(23), P(24), P(25), P<void>(26), g_stream, c.crit)); break;
        default: end(mr_flow_pair_forward_grad_tiles_typed(FWD_HEAD, P<void>(13), P<void>(14), P<void>(15), P<void>(16), FWD_TAIL, P(23), P(24), P(25),
                                                           P<void>(26), g_stream, c.crit, c.idt, c.mdt)); break;
        }
#undef FWD_HEAD
#undef FWD_TAIL
    };
    for (int which = 0; which < 6; which++) {
        for (int crit = 0; crit < 2; crit++) {
            if (crit && (which == 0 || which == 3)) continue;
            for (int dt = 0; dt < 3; dt++) {
                if (dt && which != 2 && which != 5) continue;
                Pair c; c.crit = crit; c.idt = dt ? MR_DTYPE_BF16 : MR_DTYPE_F32; c.mdt = dt == 1 ? MR_DTYPE_U8 : MR_DTYPE_F32;
                forward(which, c);
            }
        }
        { Pair c; c.ok = false; forward(which, c); }
        if (which != 2 && which != 5) continue;  // (the other four names forward to these two)
        for (int B : {0, 1, 64})
            for (int is : {36, 480}) {
                Pair c; c.B = B; c.is = is;
                forward(which, c);
            }
        for (long long tb : {0LL, 1LL, 100LL, 1LL << 40}) { Pair c; c.tile_bound = tb; forward(which, c); }
        { Pair c; c.H = 200; c.W = 180; c.Cj = 1; forward(which, c); }
        // refusals
        { Pair c; c.cap_off = 1; forward(which, c); }
        { Pair c; c.ws_short = 1; forward(which, c); }
        { Pair c; c.bstride_short = (int64_t)256 * 256 + 1; forward(which, c); }
        { Pair c; c.Cj = 2; forward(which, c); }
        { Pair c; c.W = 1; forward(which, c); }
        { Pair c; c.H = 257; forward(which, c); }
        { Pair c; c.B = -1; forward(which, c); }
        { Pair c; c.crit = 2; forward(which, c); }
        { Pair c; c.idt = MR_DTYPE_F32; c.mdt = MR_DTYPE_U8; forward(which, c); }
        { Pair c; c.idt = MR_DTYPE_U8; forward(which, c); }
        { Pair c; c.idt = MR_DTYPE_BF16; c.mdt = MR_DTYPE_BF16; forward(which, c); }
    }
    begin("flow_pair_forward_grad_tiles refused: no unit gradient");
    end(mr_flow_pair_forward_grad_tiles(P(1), P(2), P(3), P(4), 3 * 65536, P(5), P(6), P(7), P(8), P(9), P(10), P<uint8_t>(11), P<uint8_t>(12), P(13),
                                        P(14), P(15), P(16), 3, P<void>(17), mr_pair_consist_tiles_workspace_bytes(4, 256), P(18), P(19), P(20), 4, 256,
                                        256, 256, 0.05f, 1.0f, 0.5f, P<void>(21), P<void>(22), 2048, -1, nullptr, P(24), P(25), P<void>(26), g_stream));

    // occlusion over the list, and the pair loss's own entry points (plane form and listed form, both criteria)
    auto occlusion = [&](Pair c) {
        name("occlusion_flow_tiles", c);
        const int H = c.H ? c.H : c.is, W = c.W ? c.W : c.is;
        end(mr_occlusion_flow_tiles(P(1), P(2), c.ok ? P(3) : nullptr, P(4), 3LL * c.is * c.is - c.bstride_short, P(5), P(6), P(7), P(8), P(9), P(10),
                                    P<uint8_t>(11), P<uint8_t>(12), c.B, c.is, H, W, 0.05f, 1.0f, P<void>(13), P<void>(14), pair_cap(c), c.tile_bound,
                                    g_stream));
    };
    auto consist = [&](Pair c, bool listed, bool hit) {
        const int H = c.H ? c.H : c.is, W = c.W ? c.W : c.is;
        const uint8_t *h1 = hit ? P<uint8_t>(21) : nullptr, *h2 = hit ? P<uint8_t>(22) : nullptr;
        float* f12 = c.ok ? P(1) : nullptr;
        if (listed) {
            name("pair_consist_forward_tiles_crit", c);
            end(mr_pair_consist_forward_tiles_crit(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P<void>(7), mr_pair_consist_tiles_workspace_bytes(c.B, c.is) - c.ws_short,
                                                   P(8), P(9), P(10), c.B, H, W, 0.5f, P<uint8_t>(21), P<uint8_t>(22), c.is, P<void>(23), P<void>(24), pair_cap(c),
                                                   c.tile_bound, g_stream, c.crit));
            name("pair_consist_backward_tiles_crit", c);
            end(mr_pair_consist_backward_tiles_crit(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P(8), P(9), P(10), P(11), P(12), c.B, H, W, 0.5f, P<uint8_t>(21),
                                                    P<uint8_t>(22), c.is, P(13), P<void>(23), P<void>(24), pair_cap(c), c.tile_bound, g_stream, c.crit));
            if (c.crit == 0) {
                name("pair_consist_forward_tiles", c);
                end(mr_pair_consist_forward_tiles(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P<void>(7), mr_pair_consist_tiles_workspace_bytes(c.B, c.is) - c.ws_short,
                                                  P(8), P(9), P(10), c.B, H, W, 0.5f, P<uint8_t>(21), P<uint8_t>(22), c.is, P<void>(23), P<void>(24), pair_cap(c),
                                                  c.tile_bound, g_stream));
                name("pair_consist_backward_tiles", c);
                end(mr_pair_consist_backward_tiles(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P(8), P(9), P(10), P(11), P(12), c.B, H, W, 0.5f, P<uint8_t>(21),
                                                   P<uint8_t>(22), c.is, P(13), P<void>(23), P<void>(24), pair_cap(c), c.tile_bound, g_stream));
            }
            return;
        }
        begin("pair_consist_forward_crit B%d hw%dx%d is%d crit%d cj%d hit%d ws-%lld ok%d", c.B, H, W, c.is, c.crit, c.Cj, (int)hit, (long long)c.ws_short, (int)c.ok);
        end(mr_pair_consist_forward_crit(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P<void>(7), mr_pair_consist_workspace_bytes(c.B, H, W) - c.ws_short, P(8), P(9),
                                         P(10), P<uint8_t>(11), P<uint8_t>(12), P(13), P(14), P(15), P(16), P(17), P(18), c.B, H, W, 0.5f, h1, h2, c.is, g_stream,
                                         c.crit));
        begin("pair_consist_backward_crit B%d hw%dx%d is%d crit%d cj%d hit%d ws-%lld ok%d", c.B, H, W, c.is, c.crit, c.Cj, (int)hit, (long long)c.ws_short, (int)c.ok);
        end(mr_pair_consist_backward_crit(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P(8), P(9), P(10), P(11), P(12), c.B, H, W, 0.5f, h1, h2, c.is, P(13), g_stream,
                                          c.crit));
        if (c.crit == 0) {
            begin("pair_consist_forward B%d hw%dx%d is%d cj%d hit%d ws-%lld ok%d", c.B, H, W, c.is, c.Cj, (int)hit, (long long)c.ws_short, (int)c.ok);
            end(mr_pair_consist_forward(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P<void>(7), mr_pair_consist_workspace_bytes(c.B, H, W) - c.ws_short, P(8), P(9), P(10),
                                        P<uint8_t>(11), P<uint8_t>(12), P(13), P(14), P(15), P(16), P(17), P(18), c.B, H, W, 0.5f, h1, h2, c.is, g_stream));
            begin("pair_consist_backward B%d hw%dx%d is%d cj%d hit%d ws-%lld ok%d", c.B, H, W, c.is, c.Cj, (int)hit, (long long)c.ws_short, (int)c.ok);
            end(mr_pair_consist_backward(f12, P(2), P(3), P(4), P(5), P(6), c.Cj, P(8), P(9), P(10), P(11), P(12), c.B, H, W, 0.5f, h1, h2, c.is, P(13), g_stream));
        }
    };
    for (int B : {0, 4, 64})
        for (int is : {36, 480})
            for (long long tb : {-1LL, 100LL}) {
                if (tb > 0 && (B != 4 || is != 480)) continue;
                Pair c; c.B = B; c.is = is; c.tile_bound = tb;
                occlusion(c);
                for (int crit = 0; crit < 2; crit++) {
                    if (crit && B != 4) continue;
                    c.crit = crit;
                    consist(c, true, true);
                    if (tb < 0) { consist(c, false, true); if (B == 4) consist(c, false, false); }
                }
            }
    { Pair c; c.H = 200; c.W = 180; c.Cj = 1; occlusion(c); consist(c, true, true); consist(c, false, true); }
    for (int k = 0; k < 7; k++) {
        Pair c;
        if (k == 0) c.ok = false;
        if (k == 1) c.cap_off = -1;
        if (k == 2) c.ws_short = 1;
        if (k == 3) c.Cj = 2;
        if (k == 4) c.W = 1;
        if (k == 5) c.H = 257;
        if (k == 6) c.crit = 2;
        if (k != 2 && k != 3 && k != 6) occlusion(c);
        consist(c, true, true);
        if (k != 1) consist(c, false, true);
    }
    { Pair c; c.bstride_short = 256 * 256 + 1; occlusion(c); }
}

// ---- run, not recorded: every other entry point that takes a stream (--unrecorded) -----------------------------------------
// No golden file holds these cases' launch geometry; tests/test_stream_record_host.py runs them with --stream and asks that
// every runtime call they make is on that stream, and that between them and the recorded table every kernel is launched.
void unrecorded_cases() {
    const float E5 = 1e-5f;
    // the sources the recorded table does not touch
    for (int full = 0; full < 2; full++)
        for (int center : {-1, 9, 17}) {
            if (!full && center == 17) continue;
            const int64_t ws = full ? mr_mano_full_workspace_floats(3) : mr_mano_workspace_floats(3);
            begin("unrecorded mano_forward full%d center%d ws%lld", full, center, (long long)ws);
            if (full)
                end(mr_mano_forward_full(P(1), P(2), center == 9 ? P(20) : nullptr, P(3), P(4), P(5), P(6), P(7), P(8), P(9), P<int32_t>(10), P<int32_t>(11),
                                         P<int32_t>(12), center == 17 ? MR_MANO_POSE_AXISANG : MR_MANO_POSE_PCA, 30, center, 0.001f,
                                         center == 17 ? P(21) : nullptr, center == 17 ? P(22) : nullptr, center == 17 ? P(23) : nullptr, P(13), P(14), P(15), 3,
                                         g_stream));
            else
                end(mr_mano_forward(P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), P<int32_t>(10), P<int32_t>(11), P<int32_t>(12), 30, center, P(13),
                                    P(14), P(15), 3, g_stream));
            begin("unrecorded mano_backward full%d center%d", full, center);
            if (full)
                end(mr_mano_backward_full(P(3), P(4), P(5), P(6), P(7), P(8), P(9), P<int32_t>(10), P<int32_t>(11), P<int32_t>(12),
                                          center == 17 ? MR_MANO_POSE_AXISANG : MR_MANO_POSE_PCA, 30, center, P(13), P(16), P(17), P(18), P(19),
                                          center == 9 ? P(24) : nullptr, 3, g_stream));
            else
                end(mr_mano_backward(P(3), P(4), P(5), P(6), P(7), P(8), P(9), P<int32_t>(10), P<int32_t>(11), P<int32_t>(12), 30, center, P(13), P(16), P(17),
                                     P(18), P(19), 3, g_stream));
        }
    for (int B : {0, 3}) {
        begin("unrecorded meshreg_post_forward B%d", B);
        end(mr_meshreg_post_forward(P(1), P(2), P(3), P(4), P(5), P(6), 100.0f, 0.0001f, 0.4f, 256.0f, 256.0f, P(7), P(8), P(9), P(10), P(11), B, 778, 21,
                                    1002, g_stream));
        begin("unrecorded meshreg_post_backward B%d", B);
        end(mr_meshreg_post_backward(P(1), P(2), P(3), P(4), P(5), P(6), 100.0f, 0.0001f, 0.4f, 256.0f, 256.0f, P(7), P(8), P(9), P(10), P(11), P(12), P(13),
                                     P(14), P(15), P(16), B, 778, 21, 1002, g_stream));
    }
    for (int dt = 0; dt < 2; dt++)
        for (int cl = 0; cl < 2; cl++)
            for (int res = 0; res < 2; res++)
                for (int relu = 0; relu < 2; relu++)
                    for (int plane : {49, 3136}) {
                        begin("unrecorded bn_act_forward dt%d cl%d res%d relu%d plane%d", dt, cl, res, relu, plane);
                        end(mr_bn_act_forward(P<void>(1), res ? P<void>(2) : nullptr, P(3), P(4), P(5), P(6), E5, relu, dt, cl, P<void>(7), 2, 64, plane, g_stream));
                        for (int params = 0; params < 2; params++) {
                            begin("unrecorded bn_act_backward dt%d cl%d res%d relu%d plane%d params%d", dt, cl, res, relu, plane, params);
                            end(mr_bn_act_backward(P<void>(8), res ? P<void>(9) : nullptr, P<void>(1), res ? P<void>(2) : nullptr, P(3), P(4), P(5), P(6), E5, relu,
                                                   dt, cl, P<void>(10), res ? P<void>(11) : nullptr, params ? P(12) : nullptr, params ? P(13) : nullptr,
                                                   P<void>(14), mr_bn_act_backward_workspace_bytes(2, 64), 2, 64, plane, g_stream));
                        }
                    }
    for (int dt = 0; dt < 2; dt++)
        for (int plane : {49, 784}) {
            begin("unrecorded bn_add_bn_act_forward dt%d plane%d", dt, plane);
            end(mr_bn_add_bn_act_forward(P<void>(1), P<void>(2), P(3), P(4), P(5), P(6), E5, P(7), P(8), P(9), P(10), E5, dt, P<void>(11), 2, 128, plane,
                                         g_stream));
            for (int params = 0; params < 2; params++) {
                begin("unrecorded bn_add_bn_act_backward dt%d plane%d params%d", dt, plane, params);
                end(mr_bn_add_bn_act_backward(P<void>(12), params ? P<void>(13) : nullptr, P<void>(1), P<void>(2), P(3), P(4), P(5), P(6), E5, P(7), P(8), P(9),
                                              P(10), E5, dt, P<void>(14), P<void>(15), params ? P(16) : nullptr, params ? P(17) : nullptr,
                                              params ? P(18) : nullptr, params ? P(19) : nullptr, P<void>(20),
                                              mr_bn_add_bn_act_backward_workspace_bytes(2, 128), 2, 128, plane, g_stream));
            }
        }
    for (int dt = 0; dt < 2; dt++)
        for (int layout = 0; layout < 3; layout++)
            for (int hw : {13, 112}) {
                begin("unrecorded stem_pool_forward dt%d layout%d hw%d", dt, layout, hw);
                end(mr_stem_pool_forward(P<void>(1), P(2), P(3), P(4), P(5), E5, dt, layout, P<void>(6), layout ? P<unsigned char>(7) : nullptr, 2, 64, hw, hw,
                                         g_stream));
                for (int params = 0; params < 2; params++) {
                    begin("unrecorded stem_pool_backward dt%d layout%d hw%d params%d", dt, layout, hw, params);
                    end(mr_stem_pool_backward(P<void>(8), params ? P<void>(9) : nullptr, layout == 2 ? nullptr : P<void>(1),
                                              layout ? P<unsigned char>(7) : nullptr, P(2), P(3), P(4), P(5), E5, dt, layout, P<void>(10),
                                              params ? P(11) : nullptr, params ? P(12) : nullptr, P<void>(13),
                                              mr_stem_pool_backward_workspace_bytes(2, 64, hw, hw), 2, 64, hw, hw, g_stream));
                }
                if (layout != 2) continue;
                begin("unrecorded stem_pool_param_grads dt%d hw%d", dt, hw);
                end(mr_stem_pool_param_grads(P<void>(8), P<void>(9), P<unsigned char>(7), P(2), P(3), P(4), P(5), E5, dt, P(11), P(12), P<void>(13),
                                             mr_stem_pool_backward_workspace_bytes(2, 64, hw, hw), 2, 64, hw, hw, g_stream));
            }
    for (int wcl = 0; wcl < 2; wcl++)
        for (int hw : {26, 224}) {
            begin("unrecorded stem_conv_wrw wcl%d hw%d", wcl, hw);
            end(mr_stem_conv_wrw(P(1), wcl ? P(2) : nullptr, P<unsigned char>(3), P(4), P(5), P(6), P(7), E5, P(8), P(9), wcl, P<void>(10),
                                 mr_stem_conv_wrw_workspace_bytes(2, 64, hw, hw), 2, 64, hw, hw, 3, 7, 2, 3, g_stream));
        }
    for (int idt : {MR_DTYPE_F32, MR_DTYPE_BF16})
      for (int mdt : {MR_DTYPE_F32, MR_DTYPE_U8})
        for (int mc : {0, 1, 3}) {
            begin("unrecorded frames_to_batch_typed dt%d/%d mc%d", idt, mdt, mc);
            end(mr_frames_to_batch_typed(P<uint8_t>(1), P<double>(2), mc == 1 ? nullptr : P<uint8_t>(3), 0.5f, 0.5f, 0.5f, 1.0f, 1.0f, 1.0f, P<void>(4),
                                         mr_frames_to_batch_workspace_bytes(3, 64, 48), P<void>(5), mc ? P<void>(6) : nullptr, mc ? mc : 3, 3, 90, 120, 64, 48,
                                         g_stream, idt, mdt));
        }
    begin("unrecorded frames_to_batch");
    end(mr_frames_to_batch(P<uint8_t>(1), P<double>(2), P<uint8_t>(3), 0.5f, 0.5f, 0.5f, 1.0f, 1.0f, 1.0f, P<void>(4), mr_frames_to_batch_workspace_bytes(3, 64, 48),
                           P(5), P(6), 3, 3, 90, 120, 64, 48, g_stream));
    {
        // (the plans are host arrays, read before the call returns: blur or none, every op, a frame with no op at all)
        const uint8_t flip[3] = {0, 1, 0};
        const float radius[3] = {0.0f, 1.5f, 6.0f};
        const int codes[12] = {MR_COLOR_OP_BRIGHTNESS, MR_COLOR_OP_SATURATION, MR_COLOR_OP_HUE, MR_COLOR_OP_CONTRAST,
                               MR_COLOR_OP_CONTRAST, MR_COLOR_OP_HUE, MR_COLOR_OP_NONE, MR_COLOR_OP_NONE,
                               MR_COLOR_OP_NONE, MR_COLOR_OP_NONE, MR_COLOR_OP_NONE, MR_COLOR_OP_NONE};
        const float values[12] = {1.25f, 0.5f, 17.0f, 1.5f, 0.75f, -30.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int in_place = 0; in_place < 2; in_place++) {
            begin("unrecorded frames_color_augment in_place%d", in_place);
            end(mr_frames_color_augment(P<uint8_t>(1), in_place ? P<uint8_t>(1) : P<uint8_t>(2), in_place ? nullptr : flip, radius, codes, values, P<void>(3),
                                        mr_frames_color_augment_workspace_bytes(3, 90, 120), 3, 90, 120, g_stream));
        }
    }
    for (int geo = 0; geo < 4; geo++) {
        const int comps = geo ? 3 : 1, lh = geo >= 2 ? 2 : 1, lv = geo == 3 ? 2 : 1;
        begin("unrecorded jpeg_reconstruct c%d %dx%d", comps, lh, lv);
        end(mr_jpeg_reconstruct(P<unsigned char>(1), 3, 61, 45, comps, lh, lv, P<unsigned char>(2), P<void>(3),
                                mr_jpeg_reconstruct_workspace_bytes(3, 61, 45, comps, lh, lv), g_stream));
    }
    for (int ch = 1; ch <= 4; ch++) {
        begin("unrecorded png_unfilter ch%d", ch);
        end(mr_png_unfilter(P<unsigned char>(1), 3, 61, 45, ch, P<unsigned char>(2), nullptr, g_stream));
    }

    for (int center : {-1, 9}) {
        begin("unrecorded mano_adapt_forward center%d", center);
        end(mr_mano_adapt_forward(P(1), P(2), center, P(3), P(4), 3, 778, 21, g_stream));
        for (int which = 0; which < 3; which++) {  // both incoming gradients and the weight's; g_verts alone; g_joints alone
            begin("unrecorded mano_adapt_backward center%d which%d", center, which);
            end(mr_mano_adapt_backward(P(1), P(2), center, which != 2 ? P(5) : nullptr, which != 1 ? P(6) : nullptr, P(7), P(8),
                                       which == 0 ? P(9) : nullptr, 3, 778, 21, g_stream));
        }
    }
    {
        // (the jobs are a host array, read before the call returns)
        auto job = [](int k, int mode, int dims, bool affine, int center) {
            MrEvalJob j{};
            j.pred = P(4 * k + 1); j.target = mode == MR_EVAL_POINTS ? nullptr : P(4 * k + 2); j.affine = affine ? P(4 * k + 3) : nullptr;
            j.out = P(4 * k + 4); j.num_points = mode == MR_EVAL_PER_SAMPLE_SUM ? 5000 : 21; j.dims = dims; j.center = center; j.mode = mode;
            j.affine_target = affine && mode == MR_EVAL_PER_SAMPLE_SUM;
            return j;
        };
        for (int mode : {MR_EVAL_PER_POINT, MR_EVAL_PER_SAMPLE_SUM, MR_EVAL_POINTS})
            for (int affine = 0; affine < 2; affine++) {
                const MrEvalJob one = job(0, mode, affine ? 2 : 3, affine != 0, affine ? -1 : 0);
                begin("unrecorded eval_feed mode%d affine%d", mode, affine);
                end(mr_eval_feed(&one, 1, 3, g_stream));
            }
        MrEvalJob eight[MR_EVAL_MAX_JOBS];
        for (int k = 0; k < MR_EVAL_MAX_JOBS; k++) eight[k] = job(k, k % 3, k & 1 ? 2 : 3, (k & 3) == 1, k % 3 == 0 ? 9 : -1);
        begin("unrecorded eval_feed jobs%d", MR_EVAL_MAX_JOBS);
        end(mr_eval_feed(eight, MR_EVAL_MAX_JOBS, 64, g_stream));
    }
    for (int nt : {0, 20}) {
        begin("unrecorded eval_measures thresholds%d", nt);
        end(mr_eval_measures(P(1), 1000, 21, nt ? P(2) : nullptr, nt, P<double>(3), nt ? P<unsigned>(4) : nullptr, P(5), P<unsigned>(6), P(7), g_stream));
    }
    // the horizontal taps of the five instantiations: 3 (an enlargement), 5, 7, 9 (reductions up to 2, 3, 4), any count (by 5)
    for (int dst_w : {1280, 480, 256, 160, 128}) {
        begin("unrecorded frames_resize 640x480 to %dx%d taps%d", dst_w, dst_w * 3 / 4, mr_frames_resize_taps(640, dst_w));
        end(mr_frames_resize(P<unsigned char>(1), 3, 640, 480, P<unsigned char>(2), dst_w, dst_w * 3 / 4, P<int>(3), P<int>(4), P<int>(5), P<int>(6), nullptr,
                             g_stream));
    }

    // the entry points of the seven recorded sources that the recorded table never calls
    for (int mode = 0; mode < 2; mode++) {
        begin("unrecorded warp_forward mode%d", mode);
        end(mr_warp_forward(P(1), P(2), P(3), P(4), 2, 3, 60, 44, 1.0f, mode, g_stream));
        for (int which = 0; which < 3; which++) {
            begin("unrecorded warp_backward mode%d which%d", mode, which);
            end(mr_warp_backward(P(1), P(2), P(5), which != 1 ? P(6) : nullptr, which != 2 ? P(7) : nullptr, 2, 3, 60, 44, 1.0f, mode, g_stream));
        }
    }
    for (int scale = 0; scale < 2; scale++) {
        begin("unrecorded occlusion_mask scale%d", scale);
        end(mr_occlusion_mask(P(1), P(2), P(3), P(4), 3LL * 64 * 64, scale ? P(5) : nullptr, scale ? P(6) : nullptr, P(7), P(8), 2, 64, 64, 0.05f, 1.0f,
                              g_stream));
        for (int hit = 0; hit < 2; hit++) {
            begin("unrecorded occlusion_flow scale%d hit%d", scale, hit);
            end(mr_occlusion_flow(P(1), P(2), P(3), P(4), 3LL * 64 * 64, scale ? P(5) : nullptr, scale ? P(6) : nullptr, P(7), P(8), P(9), P(10),
                                  hit ? P<uint8_t>(11) : nullptr, hit ? P<uint8_t>(12) : nullptr, 2, 64, 64, 60, 44, 0.05f, 1.0f, g_stream));
        }
    }
    for (int lut = 0; lut < 2; lut++) {
        begin("unrecorded flow_mask lut%d", lut);
        end(mr_flow_mask(P(1), P<int32_t>(2), lut ? P(3) : nullptr, lut ? 40 : 0, 0.5f, P(4), 2, 64, g_stream));
    }
    begin("unrecorded flow_finalize_forward");
    end(mr_flow_finalize_forward(P(1), P(2), P(3), P(4), P(5), 2, 64, 60, 44, g_stream));
    begin("unrecorded flow_finalize_backward");
    end(mr_flow_finalize_backward(P(5), P(2), P(3), P(4), P(6), 2, 64, 60, 44, g_stream));
    for (int cam = 0; cam < 2; cam++) {
        begin("unrecorded flow_vertices_forward cam%d", cam);
        end(mr_flow_vertices_forward(P(1), P(2), P(3), P(4), P(5), P(6), P(7), cam, 256.0f, P(8), P(9), P(10), P(11), 2, 1778, g_stream));
        begin("unrecorded flow_vertices_parts_forward cam%d", cam);
        end(mr_flow_vertices_parts_forward(P(1), P(12), P(2), P(13), 778, 1000, P(3), P(4), P(5), P(6), P(7), cam, 256.0f, P(8), P(9), P(10), P(11), 2, g_stream));
        for (int clear = 0; clear < 2; clear++) {
            begin("unrecorded flow_pair_prologue_parts cam%d clear%d", cam, clear);
            end(mr_flow_pair_prologue_parts(P(1), P(12), P(2), P(13), 778, 1000, P(3), P(4), P(5), P(6), P(7), cam, 256.0f, P(8), P(9), P(10), P(11),
                                            P<int64_t>(14), cam, P<int64_t>(15), P<int32_t>(16), 1538, 2000, 2, clear ? P<void>(17) : nullptr,
                                            clear ? mr_render_clear_bytes(4, 2 * 3538, 256) : 0, g_stream));
        }
    }
    begin("unrecorded flow_vertices_backward");
    end(mr_flow_vertices_backward(P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), 2, 1778, g_stream));
    begin("unrecorded flow_vertices_parts_backward");
    end(mr_flow_vertices_parts_backward(P(1), P(12), P(2), P(13), 778, 1000, P(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10), 2, g_stream));
    for (int batched = 0; batched < 2; batched++) {
        begin("unrecorded stack_pair_faces batched%d", batched);
        end(mr_stack_pair_faces(P<int64_t>(1), batched, P<int64_t>(2), 778, P<int32_t>(3), 2, 1538, 2000, g_stream));
    }
    // the upstream-compatible raster entry points
    for (int rd = 0; rd < 2; rd++) {
        begin("unrecorded forward_face_index_map depth%d", rd);
        end(mr_forward_face_index_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), 2, 1538, 64, NEAR, FAR, 1, 1, rd, g_stream));
    }
    begin("unrecorded forward_texture_sampling");
    end(mr_forward_texture_sampling(P(1), P(2), P<int32_t>(3), P(4), P(5), P(6), P<int32_t>(7), P(8), 2, 1538, 64, 2, EPS, g_stream));
    begin("unrecorded backward_textures");
    end(mr_backward_textures(P<int32_t>(1), P(2), P<int32_t>(3), P(4), P(5), 2, 1538, 64, 2, g_stream));
    begin("unrecorded backward_depth_map");
    end(mr_backward_depth_map(P(1), P(2), P<int32_t>(3), P(4), P(5), P(6), P(7), 2, 1538, 64, g_stream));
    // kernel D by strips of two lines (rasters 263..525) and of one (526..1421) in the forms the recorded rasters do not
    // reach: alone (no texture, no depth term), with the texture gather only, with the depth gather only; and the
    // upstream-compatible entry point's one-line strips
    for (int is : {480, 1024})
        for (int form = 0; form < 3; form++) {
            Bwd c; c.is = is; c.tex = form == 1; c.rd = form == 2;
            begin("unrecorded render_backward is%d tex%d d%d", is, (int)c.tex, c.rd);
            end(render_backward(c));
        }
    begin("unrecorded backward_pixel_map is1024");
    end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), P(7), 2, 1538, 1024, EPS, 1, 1, g_stream));
    begin("unrecorded face_inv_map");
    end(mr_face_inv_map(P(1), P<int32_t>(2), P(3), 2, 1538, 64, g_stream));
    begin("unrecorded selftest_division");
    end(mr_selftest_division(P(1), P(2), P(3), P(4), 1000, g_stream));
}

// The check checks: an entry point that makes all four kinds of stream-ordered call (launches, memsets, an allocation and its
// release), handed one stream while the recorder expects another.  Every one of its calls must show as off the stream.
void stream_selftest_case() {
    void* const other = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(g_stream) ^ 0x10);
    rec_expect_stream(other);
    begin("selftest: expectation differs from the stream handed over");
    end(mr_backward_pixel_map(P(1), P<int32_t>(2), P(3), P(4), P(5), P(6), P(7), 2, 1538, 256, EPS, 0, 1, g_stream));
    rec_expect_stream(g_stream);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <kernel argument table> [--cus N] [--stack-fill BYTE] [--two-devices] [--stream HEX] [--unrecorded] [--kernel-names]\n", argv[0]);
        return 2;
    }
    rec_load_args(argv[1]);
    int cus = 256;
    bool two_devices = false, unrecorded = false;
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "--cus") && i + 1 < argc) cus = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--stack-fill") && i + 1 < argc) g_stack_fill = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--two-devices")) two_devices = true;
        else if (!std::strcmp(argv[i], "--unrecorded")) unrecorded = true;
        else if (!std::strcmp(argv[i], "--kernel-names")) { rec_print_kernel_names(); return 0; }
        else if (!std::strcmp(argv[i], "--stream") && i + 1 < argc) {
            g_stream = reinterpret_cast<mr_stream_t>(static_cast<uintptr_t>(std::strtoull(argv[++i], nullptr, 16)));
            rec_expect_stream(g_stream);
        }
    }
    rec_set_cus(cus);
    if (two_devices) {
        // the opt-in to more than 48 KB of dynamic LDS is an attribute of a kernel ON a device: the same large launch twice
        // on each of two devices
        for (int round = 0; round < 2; round++)
            for (int dev = 0; dev < 2; dev++) {
                rec_set_device(dev, 2);
                Fwd c; c.B = 2; c.F0 = 7104; c.is = 256;
                begin("two devices: round %d device %d", round, dev);
                end(render_vc_forward(c));
            }
        return 0;
    }
    rec_set_device(0, 1);
    if (unrecorded) {
        // (with the recorded table in front, so that the kernels still unlaunched at the end are unlaunched by ALL cases)
        forward_cases(true); pair_step_cases(true); forward_refusals(); backward_cases(); vc_backward_cases(); scatter_cases();
        pair_forward_cases();
        unrecorded_cases();
        stream_selftest_case();
        std::printf("# never launched\n");
        rec_report_unlaunched();
        return 0;
    }
    forward_cases(cus == 256);
    pair_step_cases(cus == 256);
    if (cus != 256) return 0;  // (only the binning pass looks at the device, for its parts: the cases it decides)
    forward_refusals();
    backward_cases();
    vc_backward_cases();
    scatter_cases();
    pair_forward_cases();
    return 0;
}
