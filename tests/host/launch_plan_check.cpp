// launch_plan_check.cpp -- csrc/launch_plan.hpp on its own, with a host compiler: the invariants the kernels rely on, over an
// exhaustive small grid of shapes, flags and devices plus the benchmark's shapes.  A plan that breaks one of them is an
// out-of-bounds LDS access or a hung barrier on a device; here it is a failing line.  Exit status 0 = every check held;
// tests/test_launch_plan_host.py builds and runs it.
#include "../../handobjectconsist_amd/csrc/launch_plan.hpp"

#include <cstdio>

static long failures = 0, checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        checks++;                                                                     \
        if (!(cond)) {                                                                \
            if (failures < 20) std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what); \
            failures++;                                                               \
        }                                                                             \
    } while (0)

using namespace mr;

static bool power_of_two(int v) { return v > 0 && (v & (v - 1)) == 0; }

static void check_bins(const BinRequest& r) {
    char what[160];
    std::snprintf(what, sizeof what, "vc%d B%d F%d F0%d V%d fb%d is%d fl%x cus%d list%d cleared%d pair%d %d+%d", (int)r.vc, r.B, r.F, r.F0, r.V,
                  (int)r.fill_back, r.is, (unsigned)r.flags, r.cus, (int)r.want_list, (int)r.list_cleared, (int)r.pair, r.Fh, r.Fo);
    const BinPlan p = plan_bins(r);
    CHECK(p.status == MR_OK || !p.launch);
    CHECK(p.grid.nbins() <= MAX_BINS || p.status != MR_OK);
    if (p.status != MR_OK) return;
    // parts: a power of two, within the most the kernels unroll over and the counters the workspace has
    CHECK(power_of_two(p.parts) && p.parts <= MAX_PARTS && p.parts <= bin_layout_parts(r.B, r.F));
    // ... all resident at once: the parts' barrier relies on it (one workgroup per compute unit)
    if (p.parts > 1 && !(r.flags & MR_FLAG_ONE_WORKGROUP_PER_IMAGE)) CHECK((int64_t)r.B * p.parts <= std::min(r.cus, MAX_PART_CUS));
    if (r.flags & MR_FLAG_ONE_WORKGROUP_PER_IMAGE) CHECK(p.parts == 1);
    // the box buffer holds the largest part's boxes, in both orientations under fill-back, hand / object split included
    CHECK(p.box_cap >= (r.F + p.parts - 1) / p.parts);
    if (r.pair)
        for (int k = 0; k < p.parts; k++) {
            int r0, nr;
            pair_part_range(k, p.parts, r.Fh, r.Fo, r0, nr);
            CHECK(p.box_cap >= (r.fill_back ? 2 * nr : nr));
            CHECK(r0 >= 0 && nr >= 0 && r0 + nr <= r.Fh + r.Fo);
        }
    if (!p.launch) return;
    const size_t counters = (size_t)((p.grid.nbins() + 3) & ~3) * 4;
    CHECK((int64_t)p.lds <= LDS_LIMIT && (int64_t)p.lds_fill <= LDS_LIMIT);
    CHECK(p.lds >= counters + (p.lds_boxes ? (size_t)p.box_cap * FACE_BOX_BYTES : 0));
    CHECK(p.lds_fill == counters);
    CHECK(p.lds_opt_in == ((int64_t)p.lds > LDS_DEFAULT_LIMIT));
    CHECK(grid_ok(p.wgs) && p.wgs >= (unsigned)r.B * p.parts && (p.parts == 1 || p.wgs % 8 == 0));
    CHECK(p.images == (unsigned)r.B && p.images <= (unsigned)MAX_BATCH_Y);
    // two launches exactly when the parts are eight or more and the caller did not ask for one
    CHECK(p.two_launches == (p.parts >= 8 && !(r.flags & MR_FLAG_PARTS_IN_ONE_LAUNCH)));
    // the per-face pass inside the binning kernel needs the list, its header cleared, and the boxes in LDS
    if (p.faces == BinPlan::FACES_IN_KERNEL) CHECK(r.vc && p.list && r.list_cleared && p.lds_boxes && r.F0 > 0 && p.form != BinPlan::PLAIN);
    if (p.form != BinPlan::PLAIN) CHECK(p.faces == BinPlan::FACES_IN_KERNEL);
    if (p.faces == BinPlan::FACES_LAUNCH) CHECK(r.F0 > 0 && p.face_blocks * 256u >= (unsigned)r.F0 && p.form == BinPlan::PLAIN);
    if (p.faces == BinPlan::FACES_CLEAR_LIST) CHECK(r.F0 == 0 && p.list);
    // the vertex stage inside needs pairs of images and the vertices behind the boxes
    CHECK((p.prologue != BinPlan::PRO_NONE) == r.pair);
    CHECK((p.form == BinPlan::PROLOGUE) == (p.prologue == BinPlan::PRO_IN_KERNEL));
    if (p.prologue == BinPlan::PRO_IN_KERNEL)
        CHECK((r.B & 1) == 0 && p.lds >= counters + (size_t)p.box_cap * FACE_BOX_BYTES + (size_t)r.V * 12);
    if (p.list) CHECK(p.grid.ysh == 0 && grid_ok((int64_t)r.B * p.grid.nbins()));
}

static void check_tiles(int B, int is, bool listed, bool fused, int64_t bound) {
    char what[96];
    std::snprintf(what, sizeof what, "tiles B%d is%d listed%d fused%d bound%lld", B, is, (int)listed, (int)fused, (long long)bound);
    const TilePlan p = plan_tiles(B, is, listed, fused, bound);
    const int64_t tiles = (int64_t)B * p.tiles_x * p.tiles_y;
    CHECK(p.tiles_x * TILE_W >= is && p.tiles_y * TILE_H >= is);
    if (!p.launch) { CHECK(tiles == 0 || p.status != MR_OK); return; }
    CHECK(p.status == MR_OK && grid_ok(p.wgs) && p.wgs >= 1 && (int64_t)p.wgs <= tiles);
    if (!listed) CHECK((int64_t)p.wgs == tiles);
    else CHECK(fused && (p.wgs % 8 == 0 || (int64_t)p.wgs == tiles));
}

static void check_backward(const BackwardRequest& r) {
    char what[160];
    std::snprintf(what, sizeof what, "bwd B%d F%d is%d ts%d fl%x eps%g gf%d gt%d rgb%d a%d d%d ws%lld", r.B, r.F, r.is, r.ts, (unsigned)r.flags,
                  (double)r.eps, (int)r.grad_faces, (int)r.grad_textures, (int)r.rgb, (int)r.alpha, (int)r.depth, (long long)r.workspace_bytes);
    const BackwardPlan p = plan_render_backward(r);
    // the fused strip-gather only with the list and the strips, and only when a gather has something to do
    if (p.fuse) CHECK(p.use_list && p.strips_d && p.want_d && p.run_gather && p.gather_form != GatherForm::NONE);
    if (p.pixel_map.fused) CHECK(p.fuse && p.pixel_map.strips && p.pixel_map.gather == p.gather_form && p.gather_threads == 0);
    if (p.use_list) CHECK(r.workspace_bytes >= r.list_bytes && !(r.flags & MR_FLAG_REFERENCE_ALGO));
    if (p.strips_d) CHECK(r.workspace_bytes >= r.full_bytes && strip_lines(r.is) > 0 && r.F < (1 << 24));
    CHECK(!(p.list_only && p.want_d));
    CHECK(!(p.tex_atomics && p.gather_tex));
    if (p.gather_tex) CHECK(r.grad_textures && r.ts == 2 && r.eps >= 1e-6f);
    // every requested output has a writer: the face rows by D or the gather, the textures by the gather or the atomics
    if (r.grad_faces) CHECK(p.want_d || p.run_gather);
    if (r.grad_textures) CHECK(p.tex_atomics || (p.gather_tex && p.run_gather));
    if (p.run_gather) CHECK(p.pixel_map.fused != (p.gather_threads > 0) || (int64_t)r.B * r.F == 0);
    if (p.want_d && p.pixel_map.strips) {
        const PixelMapPlan& m = p.pixel_map;
        CHECK((int64_t)m.lds <= 64 * 1024 && m.shape.lines >= 1 && m.shape.lines <= 4);
        CHECK((int64_t)m.shape.strips_axis * m.shape.lines >= r.is);
        CHECK(m.mark.threads >= m.shape.n_weights && m.mark.threads >= m.mark.items);
        CHECK(m.status_grid != MR_OK || (grid_ok(m.wgs) && m.wgs == 8u * (unsigned)m.shape.cap));
        CHECK(m.compact.status != MR_OK || (int64_t)m.compact.chunks * CO_TPB * CO_PER >= r.F);
        if (m.fused) CHECK(grid_ok(m.fused_wgs) && m.fused_wgs == 8u * (m.gather_groups + (unsigned)m.shape.cap) &&
                           (int64_t)m.gather_groups * 8 * PS_T >= (int64_t)r.B * r.F * GGL);
    }
}

int main() {
    const char* what = "";
    // ---- the binning pass: an exhaustive small grid, then the benchmark's shapes ----
    const int batches[] = {0, 1, 2, 3, 8, 16, 32, 64, 128, 192, 65535, 65536};
    const int faces[] = {0, 1, 255, 256, 511, 512, 1538, 3076, 7104, 20000};
    const int rasters[] = {1, 8, 36, 256, 480, 640, 1024, 4096, 9000, 16384};
    const int flag_sets[] = {0, MR_FLAG_FORCE_PARTS, MR_FLAG_PARTS_IN_ONE_LAUNCH, MR_FLAG_ONE_WORKGROUP_PER_IMAGE,
                             MR_FLAG_FORCE_PARTS | MR_FLAG_PARTS_IN_ONE_LAUNCH, MR_FLAG_FORCE_PARTS | MR_FLAG_ONE_WORKGROUP_PER_IMAGE};
    const int devices[] = {0, 1, 64, 104, 256, 304};
    for (int B : batches)
        for (int F0 : faces)
            for (int is : rasters)
                for (int flags : flag_sets)
                    for (int cus : devices)
                        for (int mode = 0; mode < 12; mode++) {
                            BinRequest r{};
                            r.vc = mode >= 2; r.fill_back = r.vc && (mode & 1);
                            r.B = B; r.F0 = F0; r.F = r.fill_back ? 2 * F0 : F0; r.V = 2000; r.is = is; r.flags = flags; r.cus = cus;
                            r.want_list = mode >= 4; r.list_cleared = mode >= 6;
                            r.pair = mode >= 8;
                            if (r.pair) {
                                r.Fh = mode >= 10 ? F0 / 5 : F0; r.Fo = F0 - r.Fh; r.V = mode >= 10 ? 2560 : 778;
                            }
                            check_bins(r);
                        }
    // (the metric mesh 1538 + 2000 faces / 778 + 1000 vertices, fill-back, batches of 8 to 64 pairs at 256, 480 and 640 pixels)
    for (int B : {16, 32, 64, 128})
        for (int is : {256, 480, 640})
            for (int cus : {256, 304, 64}) {
                BinRequest r{};
                r.vc = true; r.fill_back = true; r.B = B; r.F0 = 3538; r.F = 7076; r.V = 1778; r.is = is; r.cus = cus;
                r.want_list = true; r.list_cleared = true; r.pair = true; r.Fh = 1538; r.Fo = 2000;
                check_bins(r);
                const BinPlan p = plan_bins(r);
                CHECK(p.status == MR_OK && p.launch && p.faces == BinPlan::FACES_IN_KERNEL && p.prologue == BinPlan::PRO_IN_KERNEL);
            }
    // the split of a pair step's parts covers every face once
    for (int K : {1, 2, 4, 8, 16})
        for (int Fh : {0, 1, 5, 1538})
            for (int Fo : {0, 1, 7, 2000, 9000}) {
                int next = 0;
                for (int k = 0; k < K; k++) {
                    int r0, nr;
                    pair_part_range(k, K, Fh, Fo, r0, nr);
                    CHECK(r0 == next && nr >= 0);
                    next = r0 + nr;
                }
                CHECK(next == Fh + Fo);
            }

    // ---- the tile launch ----
    for (int B : batches)
        for (int is : rasters)
            for (int listed = 0; listed < 2; listed++)
                for (int fused = 0; fused < 2; fused++)
                    for (long long bound : {-1LL, 0LL, 1LL, 5LL, 8LL, 100LL, 1LL << 20, 1LL << 40}) check_tiles(B, is, listed != 0, fused != 0, bound);
    for (long long cap : {0LL, 8LL, 9LL, 2048LL, 1LL << 30})
        for (long long bound : {-1LL, 0LL, 1LL, 100LL, 1LL << 40}) {
            const unsigned g = listed_grid(bound, cap);
            CHECK(g % 8 == 0 && (int64_t)g <= ((cap + 7) & ~7LL) && (g >= 8 || cap == 0));
        }

    // ---- the generic backward ----
    for (int B : {1, 2, 16, 128})
        for (int F : {1, 255, 1538, 7104, 1 << 24})
            for (int is : {1, 2, 3, 36, 256, 480, 640, 1024, 2048, 8192})
                for (int ts : {2, 4})
                    for (float eps : {1e-7f, 1e-6f, 1e-3f})
                        for (int flags : {0, MR_FLAG_REFERENCE_ALGO, MR_FLAG_COUNT_PIXEL_MAP_TERMS})
                            for (int outs = 0; outs < 32; outs++)
                                for (int ws = 0; ws < 3; ws++) {
                                    BackwardRequest r{};
                                    r.B = B; r.F = F; r.is = is; r.ts = ts; r.eps = eps; r.flags = flags;
                                    r.grad_faces = outs & 1; r.grad_textures = outs & 2; r.rgb = outs & 4; r.alpha = outs & 8; r.depth = outs & 16;
                                    if (r.grad_textures && !r.rgb) continue;  // (refused by the entry point)
                                    // (the layout's sizes: the owner list, and the strips' words behind it)
                                    r.list_bytes = round_up((int64_t)B * F) + 256 + round_up(20LL * B) + round_up((int64_t)B * F * 4) + round_up((int64_t)B * F * 32);
                                    const StripShape sh = strip_shape(B, is);
                                    r.full_bytes = r.list_bytes + (sh.lines ? round_up(sh.n_weights * 4) + round_up(8LL * sh.cap * 4) + 256 : 0);
                                    r.workspace_bytes = ws == 0 ? 0 : ws == 1 ? r.list_bytes : r.full_bytes;
                                    check_backward(r);
                                }
    for (int is = 1; is <= 16384; is += (is < 2100 ? 1 : 97)) {
        const int L = strip_lines(is);
        CHECK(L == 0 || L == 1 || L == 2 || L == 4);
        if (L) CHECK(strip_lds_bytes(is, L) <= 64 * 1024);
    }

    // ---- the vertex-colour backward and the tile scatter ----
    for (int B : {1, 2, 64, 128})
        for (int V : {1, 778, 1778, 2560, 2561, 3840, 3841, 5000})
            for (int is : {4, 36, 256, 480, 640, 1024, 1028, 8192, 8193})
                for (int variant = 0; variant < 4; variant++) {
                    char what[96];
                    std::snprintf(what, sizeof what, "scatter B%d V%d is%d variant%d", B, V, is, variant);
                    const ScatterVCPlan v = plan_scatter_vc(B, V, 1538, is, (variant & 1) ? MR_FLAG_FORCE_GATHER : 0);
                    if (v.status == MR_OK && v.scatter) {
                        CHECK((int64_t)v.lds <= SV_MAX_TABLE_BYTES && (int64_t)v.lds >= (int64_t)V * 3 * 8 && !(variant & 1));
                        CHECK(v.rx_n * SV_W >= is && v.ry_n * SV_H >= is && v.wgs == (unsigned)(B * v.rx_n * v.ry_n));
                    }
                    if (v.status == MR_OK && !v.scatter) CHECK(is <= MAX_GATHER_VC_RASTER && v.gather_threads == (int64_t)B * 1538 * GLPF);
                    const ScatterPlan t = plan_scatter_tiles(B, V, is, (variant & 1) != 0, (variant & 2) != 0);
                    if (t.status != MR_OK) continue;
                    // the table within its limit, the tiles within the covered-tile list, 8 / 16 / 32 workgroups per image
                    CHECK((int64_t)t.lds <= SV_MAX_TABLE_BYTES && (int64_t)t.lds >= (int64_t)V * ((variant & 1) ? 3 : 2) * 8);
                    CHECK(is % 4 == 0 && t.tiles_x * t.tiles_y <= ST_MAX_TILES && t.tiles_x * ST_TW >= is && t.tiles_y * ST_TH >= is);
                    CHECK(t.groups == 8 || t.groups == 16 || t.groups == 32);
                    CHECK((variant & 2) || t.groups == ST_G);
                    CHECK(t.wgs == (unsigned)(B * t.groups));
                }
    {
        const char* what = "workgroups per image of the pair scatter at the benchmark's rasters";
        CHECK(plan_scatter_tiles(16, 1778, 256, false, true).groups == 8);
        CHECK(plan_scatter_tiles(16, 1778, 480, false, true).groups == 32);
        CHECK(plan_scatter_tiles(16, 1778, 640, false, true).groups == 32);
    }

    if (failures == 0) std::printf("launch_plan_check: ok (%ld checks)\n", checks);
    else std::printf("launch_plan_check: %ld of %ld checks failed\n", failures, checks);
    return failures == 0 ? 0 : 1;
}
