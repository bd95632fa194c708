// launch_plan.hpp -- what the raster and warp launchers decide before they launch, as plain structs returned by pure functions
// of the shapes, the flags and the device's compute-unit count.  Plain C++17, no HIP include, no pointer and no runtime call
// (tests/host/launch_plan_check.cpp builds it with the host compiler alone and checks the invariants the kernels rely on).
//
// A launcher reads: check the arguments, plan, fill the parameter block from the plan, launch by switching on the plan.  The
// constants a decision needs live here; the .hip file that owns the kernel ties each to the struct or kernel it mirrors with a
// static_assert.  The measurements that justify a decision stay with it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/meshraster_hip.h"
#include "host_layout.hpp"

#if defined(__HIP__)
#define MR_PLAN_HD __attribute__((host)) __attribute__((device))
#else
#define MR_PLAN_HD
#endif

namespace mr {

// ---- constants shared by the kernels and the plans ---------------------------------------------------------------------
constexpr int TILE_W = 32, TILE_H = 8;  // tile size in pixels (one pixel per thread)
constexpr int TPB = 256;              // threads per workgroup (4 waves)
constexpr int BIN_TPB = 1024;         // bin_boxes_kernel: one workgroup per image
constexpr int MAX_BINS = 8192;        // LDS counters (32 KB)
constexpr int MAX_PARTS = 16;         // most workgroups per image of the binning pass
constexpr int MAX_PART_CUS = 256;     // the most compute units the parts are sized for (the workspace layout assumes these)
constexpr int64_t LDS_DEFAULT_LIMIT = 48 * 1024;  // dynamic LDS a kernel may ask for without the opt-in
constexpr int64_t LDS_LIMIT = 152 * 1024;         // ... with it: what a plan may spend
constexpr int MAX_BATCH_Y = 65535;    // an image per grid row (face_records_kernel)
constexpr int FACE_BOX_BYTES = 8;     // sizeof(FaceBox)
constexpr int WAVE = 64;

constexpr int SV_WAVES = 16;                                    // scatter_vc_kernel: waves per block
constexpr int SV_RPW = 2, SV_W = 64, SV_H = SV_WAVES * SV_RPW;  // rows per wave, region
constexpr int SV_MAX_TABLE_BYTES = 60 * 1024;                   // the per-image colour table in LDS
constexpr int GLPF = 4;               // lanes per face of the vertex-colour gather
constexpr int GGL = 8;                // lanes per face of the generic gather (E: 74 -> 64 us, E + F: 105 -> 93 us against 4; 16: 70 / 101)
constexpr int MAX_GATHER_VC_RASTER = 8192;  // gather fragment encoding: 13 bits per bbox offset

constexpr int ST_G = 8;       // tile scatter: workgroups per image (sp.groups), at least
constexpr int ST_G_MAX = 32;
constexpr int ST_WAVES = 8;   // waves per workgroup
constexpr int ST_TW = 32, ST_TH = 8;  // the forward's tile
constexpr int ST_MAX_TILES = 4096;    // tiles per image the covered-tile list in LDS can hold (1024 x 1024 pixels)
// fixed point of the per-workgroup sums: terms below 2^ST_FIX_BITS in magnitude (2^-37 of the workgroup's largest gradient
// per term: 13 bits below the last bit of an fp32 value of that size), sums below 2^ST_SUM_BITS (st_headroom)
constexpr int ST_FIX_BITS = 37, ST_SUM_BITS = 50;

constexpr int PS_T = 256;      // kernel D by strips: threads per workgroup
constexpr int PS_QCAP = 1024;  // queued entries; a round of PS_T faces adds at most 3 * PS_T
constexpr int PS_TASKS = 1024; // chunk tasks of a wave's batch: 64 items, at most 16 chunks each
constexpr int CO_TPB = 1024, CO_PER = 1;  // compact_owners_kernel
constexpr int SL_T = 1024;                // strip_list_kernel

constexpr int64_t blocks_of(int64_t n, int64_t per) { return (n + per - 1) / per; }

// ---- the binning pass (raster_fwd.hip: launch_bins) ----------------------------------------------------------------------

// PROLOGUE (pair steps): the parts of an image split its faces AT the hand / object boundary -- Kh parts share the Fh hand faces,
// K - Kh the Fo object faces, in proportion -- so that a part needs only the vertices of ITS side in LDS (hand faces index the
// hand's vertices, object faces the object's: warpbranch.py:49-55, the contract of the stacked mesh): one trip of the vertex
// stage per part instead of two at the metric workload.  Returns the part's real faces [r0, r0 + nr) and its side (0 hand, 1 object,
// -1: no split -- one part, or a mesh with one side only).
MR_PLAN_HD inline int pair_part_range(int part, int K, int Fh, int Fo, int& r0, int& nr) {
    const int F0 = Fh + Fo;
    if (K < 2 || Fh <= 0 || Fo <= 0) {
        r0 = (int)((int64_t)F0 * part / K); nr = (int)((int64_t)F0 * (part + 1) / K) - r0;
        return -1;
    }
    int Kh = (int)(((int64_t)K * Fh + F0 / 2) / F0);
    Kh = Kh < 1 ? 1 : (Kh > K - 1 ? K - 1 : Kh);
    if (part < Kh) {
        r0 = (int)((int64_t)Fh * part / Kh); nr = (int)((int64_t)Fh * (part + 1) / Kh) - r0;
        return 0;
    }
    const int q = part - Kh, Ko = K - Kh;
    r0 = (int)((int64_t)Fo * q / Ko); nr = (int)((int64_t)Fo * (q + 1) / Ko) - r0;
    r0 += Fh;
    return 1;
}

// the raster's bins: a bin is TILE_W x (TILE_H << ysh) pixels, as few rows of tiles per bin as keep the bins within MAX_BINS
struct BinGrid {
    int tiles_x, tiles_y, nbx, nby, ysh;
    int nbins() const { return nbx * nby; }
};
inline BinGrid bin_grid(int is) {
    BinGrid g;
    g.tiles_x = (int)blocks_of(is, TILE_W); g.tiles_y = (int)blocks_of(is, TILE_H);
    g.nbx = g.tiles_x;
    g.ysh = 0;
    while ((int64_t)g.tiles_x * ((g.tiles_y + (1 << g.ysh) - 1) >> g.ysh) > MAX_BINS) g.ysh++;
    g.nby = (g.tiles_y + (1 << g.ysh) - 1) >> g.ysh;
    return g;
}
// a tile list can be built when a bin is a tile and the global tile ids fit 31 bits
inline bool tile_list_ok(int B, const BinGrid& g) { return g.ysh == 0 && grid_ok((int64_t)B * g.nbx * g.nby); }

// Workgroups per image of the binning pass: the largest power of two (<= 16) that keeps B x parts within the device's
// compute units -- every workgroup of the launch resident at once, which the parts' barrier relies on -- and leaves a part
// at least 256 faces.  Phase stamps (profiles/r05_binning_parts.txt): the exchange costs a part
// ~2.5 us (publish 0.4, barrier 0.8, the other parts' counters 1.4) once it stays inside the XCD's L2; 16 renders of 480 x 480
// (config 3, the reference's default batch size) 19.5 -> 13.9 us per workgroup, 64 renders 19.6 -> 16.6, 128 renders 21.7 -> ~19.
inline int bin_parts(int B, int F, int cus, int per_cu = 2) {
    int k = 1;
    while (k < MAX_PARTS && (int64_t)B * k * 2 <= (int64_t)per_cu * cus && F / (k * 2) >= 256) k *= 2;
    return k;
}
// (the workspace is sized for a 256-CU device, the most plan_bins assumes: the layout must not depend on the device at hand)
inline int bin_layout_parts(int B, int F) { return bin_parts(B, F, MAX_PART_CUS); }
// words of one part's counters in the workspace: its raw bin counters + {its large faces, its "everywhere" flag}, padded
inline int part_counter_words(const BinGrid& g) { return (g.nbins() + 4 + 31) & ~31; }

struct BinRequest {
    bool vc;            // vertex-colour mode (faces from vertices + indices)
    int B, F, F0, V;    // images, virtual faces (2 F0 with fill-back), real faces, vertices
    bool fill_back;
    int is, flags, cus; // raster, MR_FLAG_*, compute units of the current device
    bool want_list;     // the caller asks for the tile list (sparse tiles with a bound, or a dense listed launch)
    bool list_cleared;  // the caller cleared the tile list's header on this stream -- what the per-face pass's first thread does
    bool pair;          // a pair step's render: the vertex stage has not run yet
    int Fh, Fo;         // ... its hand / object faces
};

struct BinPlan {
    int status;         // MR_OK, or why nothing is launched
    BinGrid grid;
    bool list;          // the tile list is built
    int64_t tile_cap;   // ... with room for this many entries in each of its two parts
    bool launch;        // false: refused, or an empty batch
    int parts, box_cap, lds_boxes;
    enum Prologue { PRO_NONE, PRO_IN_KERNEL, PRO_SEPARATE } prologue;
    enum FacePass { FACES_IN_KERNEL, FACES_LAUNCH, FACES_CLEAR_LIST, FACES_NONE } faces;
    enum Form { PLAIN, RECORDS, PROLOGUE } form;  // which bin_boxes / bin_count kernel
    bool two_launches;  // count launch + fill launch instead of the last-arriver form
    size_t lds, lds_fill;   // dynamic LDS of the (first) launch / of the fill launch
    unsigned wgs;           // workgroups of the binning launches
    unsigned face_blocks, images;  // per-face pass: blocks per image x images
    bool lds_opt_in;        // the launch needs more than the default dynamic LDS limit
};

inline BinPlan plan_bins(const BinRequest& r) {
    BinPlan p{};
    p.grid = bin_grid(r.is);
    if (p.grid.nbx > MAX_BINS) { p.status = MR_ERR_BADARG; return p; }  // (image_size <= 16384 keeps a row of bins within the counters)
    p.list = r.want_list && tile_list_ok(r.B, p.grid);
    const int nbins = p.grid.nbins();
    p.tile_cap = p.list ? (int64_t)r.B * nbins : 0;
    // parts per image (bin_boxes_kernel, PARTS): B x parts workgroups, all resident at once; MR_FLAG_ONE_WORKGROUP_PER_IMAGE: one
    // (at most one workgroup per compute unit: two per compute unit were measured at 2B = 128: 37.7 us against 28.9 with two
    // parts and 28.5 with one; config 3's 16 renders: 16 parts 23.1 us, one part 26.0)
    int parts = (r.flags & MR_FLAG_ONE_WORKGROUP_PER_IMAGE) ? 1 : bin_parts(r.B, r.F, std::min(r.cus, MAX_PART_CUS), 1);
    parts = std::min(parts, bin_layout_parts(r.B, r.F));
    const bool fused_records = r.vc && r.list_cleared && p.list && r.F0 > 0;
    // The parts pay where they split the PER-FACE pass (fused_records: 64 renders of 256 x 256 22.1 us with 4 parts against 24.3
    // with one, 16 renders of 480 x 480 21.9 / 24.5, 64 of 640 x 640 31.1 / 35.5; 128 renders: 28.3 / 28.5).  With the boxes
    // already in memory a part only saves counting, and the exchange costs more than that unless the bins are many: 128 renders
    // of 256 x 256 19.6 us with two parts, 17.8 with one; 64 renders 16.9 / 15.6; 16 of 480 x 480 18.3 / 17.5; 64 of 640 x 640
    // (1600 bins) 26.2 / 27.9 (round 6, rocprofv3 over `bench.py --kernels-only` / scripts/hot_only.py).
    if (!fused_records && nbins <= 1024 && !(r.flags & MR_FLAG_FORCE_PARTS)) parts = 1;
    p.parts = parts;
    const size_t lds_counters = (size_t)((nbins + 3) & ~3) * sizeof(int);
    size_t lds = lds_counters;
    // (boxes of the largest part: its share of the real faces in both orientations, or of the virtual faces)
    int box_cap = (r.F + parts - 1) / parts + 2;
    if (r.pair) {  // (the parts of a pair step split at the hand / object boundary: pair_part_range)
        int most = 0;
        for (int k = 0; k < parts; k++) {
            int r0, nr;
            pair_part_range(k, parts, r.Fh, r.Fo, r0, nr);
            most = std::max(most, nr);
        }
        box_cap = std::max(box_cap, (r.fill_back ? 2 * most : most) + 2);
    }
    p.box_cap = box_cap;
    const size_t box_lds = (size_t)box_cap * FACE_BOX_BYTES;
    p.lds_boxes = (lds + box_lds <= (size_t)LDS_LIMIT) ? 1 : 0;
    if (p.lds_boxes) lds += box_lds;
    if (r.B == 0) return p;  // (an empty batch: only the parameter blocks are filled)
    if (r.B > MAX_BATCH_Y) { p.status = MR_ERR_BADARG; return p; }
    p.launch = true;
    // the per-face pass runs inside the binning kernel when the caller cleared the list header and the boxes stay in LDS
    const bool records_in_kernel = fused_records && p.lds_boxes;
    // ... and the pair's vertex stage too where the vertices fit behind the boxes -- else as a launch of its own, in front
    p.prologue = BinPlan::PRO_NONE;
    if (r.pair) {
        const size_t v_lds = (size_t)r.V * 3 * sizeof(float);
        if (r.vc && records_in_kernel && (r.B & 1) == 0 && lds + v_lds <= (size_t)LDS_LIMIT) {
            p.prologue = BinPlan::PRO_IN_KERNEL;
            lds += v_lds;
        } else {
            p.prologue = BinPlan::PRO_SEPARATE;
        }
    }
    // no face, no per-face pass: the list counters that pass clears (thread 0 of image 0) are cleared by a memset, before
    // the binning pass adds to them -- an empty mesh gives an empty list, not whatever the workspace held
    p.faces = records_in_kernel ? BinPlan::FACES_IN_KERNEL : r.F0 > 0 ? BinPlan::FACES_LAUNCH : p.list ? BinPlan::FACES_CLEAR_LIST : BinPlan::FACES_NONE;
    p.face_blocks = (unsigned)blocks_of(r.F0, 256); p.images = (unsigned)r.B;
    p.form = p.prologue == BinPlan::PRO_IN_KERNEL ? BinPlan::PROLOGUE : records_in_kernel ? BinPlan::RECORDS : BinPlan::PLAIN;
    p.lds = lds;
    p.lds_fill = lds_counters;  // (counters only: the fill launch keeps no boxes in LDS)
    p.lds_opt_in = (int64_t)lds > LDS_DEFAULT_LIMIT;
    // (parts > 1: workgroup i = part (i / 8) % parts of image (i / 8 / parts) * 8 + i % 8 -- an image's parts on one XCD)
    p.wgs = parts > 1 ? (unsigned)((r.B + 7) / 8) * 8u * (unsigned)parts : (unsigned)r.B;
    // (eight parts or more: the parts' exchange across a kernel boundary -- count launch, fill launch.  Measured on one box, pair
    // steps, device time per hot-path pass: 16 renders of 480 x 480 in 16 parts 27.7 us as one launch, 13.0 + 8.7 as two (0.097 ->
    // 0.092 ms); 32 renders in 8 parts and 64 in 4: no difference (0.0811 / 0.0818, 0.1109 / 0.1112); 128 renders of 256 x 256 in
    // 2 parts 33.4 against 22.4 + 13.1 -- with few parts the last arriver's serial share is small and the second launch's floor
    // is not.  MR_FLAG_PARTS_IN_ONE_LAUNCH: the last-arriver form whatever the parts)
    p.two_launches = parts >= 8 && !(r.flags & MR_FLAG_PARTS_IN_ONE_LAUNCH);
    return p;
}

// Can a dense launch (every requested plane written for every pixel) go over the tile list?  Full tiles with 16-byte rows,
// no per-pixel inverse map (the background stream does not write one), a raster whose bins are tiles.
inline bool dense_list_ok(int B, int is, bool inverse_map, int flags) {
    if ((flags & (MR_FLAG_REFERENCE_ALGO | MR_FLAG_TILE_PER_WORKGROUP)) || inverse_map) return false;
    if ((is % TILE_W) != 0 || (is % TILE_H) != 0) return false;
    return tile_list_ok(B, bin_grid(is));
}

// ---- the tile launch (raster_fwd.hip: launch_tiles) ----------------------------------------------------------------------
// `tile_bound` (listed launches): the caller's guess of the tile-list length = workgroups to dispatch; a longer list
// is walked with a grid stride, surplus workgroups leave after one scalar load.  Zero or less: a quarter of the screen.
struct TilePlan {
    int status;
    bool launch;
    int tiles_x, tiles_y;
    unsigned wgs;
};
inline TilePlan plan_tiles(int B, int is, bool listed, bool fused, int64_t tile_bound) {
    TilePlan p{};
    p.tiles_x = (int)blocks_of(is, TILE_W);
    p.tiles_y = (int)blocks_of(is, TILE_H);
    const int64_t nblocks = (int64_t)B * p.tiles_x * p.tiles_y;
    if (nblocks == 0) return p;
    if (!grid_ok(nblocks)) { p.status = MR_ERR_BADARG; return p; }
    if (listed) {
        // Listed launch: `bound` workgroups take one list entry each; whatever the list holds beyond the caller's guess
        // is walked afterwards by the same workgroups (raster_overflow_tiles).
        if (!fused) { p.status = MR_ERR_NOTIMPL; return p; }  // (no lists for the five-entry-point compatible path)
        if (tile_bound <= 0) tile_bound = (nblocks + 3) / 4;
        p.wgs = (unsigned)std::min<int64_t>(nblocks, std::max<int64_t>((tile_bound + 7) & ~(int64_t)7, 8));
    } else {
        p.wgs = (unsigned)nblocks;
    }
    p.launch = true;
    return p;
}

// listed launches of the warp half: the same guess over a list of `cap` entries
inline unsigned listed_grid(int64_t tile_bound, int64_t cap) {
    if (tile_bound <= 0) tile_bound = (cap + 3) / 4;
    return (unsigned)std::min<int64_t>((cap + 7) & ~(int64_t)7, std::max<int64_t>((tile_bound + 7) & ~(int64_t)7, 8));
}

// ---- the generic backward (raster_bwd.hip: mr_render_backward, launch_pixel_map) -------------------------------------------

// lines per strip: the most whose records leave room for three workgroups per compute unit; 0 = raster too wide
inline int strip_lines(int is) {
    for (int L = 4; L >= 1; L >>= 1)
        if (L * (is + 1) * 36LL <= 37 * 1024) return L;
    return ((is + 1) * 36LL <= 50 * 1024) ? 1 : 0;  // (one workgroup of 64 KB)
}
inline int64_t strip_lds_bytes(int is, int L) {
    return 2LL * L * (is + 1) * 16 + (((int64_t)L * (is + 1) * 4 + 15) & ~15LL) + PS_QCAP * 4LL + (PS_T / WAVE) * (PS_TASKS * 2LL + WAVE * 8LL);
}
// kernel D's strip bookkeeping: strips per axis, capacity of a per-XCD list, weight words [B][2 strips_axis]
struct StripShape {
    int lines, strips_axis, strips, cap;  // lines per strip; strips per axis, per image (both axes), per XCD list
    int64_t n_weights;
};
inline StripShape strip_shape(int B, int is) {
    StripShape s{};
    s.lines = strip_lines(is);
    if (s.lines == 0) return s;  // (a raster whose lines do not fit LDS: no strips, no bytes)
    s.strips_axis = (is + s.lines - 1) / s.lines;
    s.strips = 2 * s.strips_axis;
    const int64_t S = s.strips;
    s.cap = (int)(((B + 7) / 8) * S);
    s.n_weights = (int64_t)B * S;
    return s;
}
// kernel D by strips needs the workspace, a raster whose lines fit LDS and 24-bit owner numbers
inline bool strips_apply(int B, int F, int is, int64_t workspace_bytes, int64_t full_bytes, int flags) {
    return workspace_bytes >= full_bytes && !(flags & MR_FLAG_REFERENCE_ALGO) && strip_lines(is) != 0 && (int64_t)B * F < 0x7fffffffLL &&
           F < (1 << 24);
}

// (a plan gives a 1-D launch as its thread count; launch1d is the one place that skips an empty one and refuses a grid past
// the limit)

// the marking pass over the face index map, four pixels per thread where the raster allows; it clears `n_weights` strip
// weights on the way, one word per thread (2 B is / L words -- more than B is^2 / 4 pixel quads for rasters of one or two
// pixels, found by tests/fuzz_parity.py: the launch then covers the weights, the kernels guard)
struct MarkPlan {
    bool quads;
    int64_t items, ppi;  // pixel quads or pixels; pixels per image
    int64_t threads;     // one per item, and enough for the weights
};
inline MarkPlan plan_mark(int B, int is, int64_t n_weights) {
    MarkPlan m{};
    m.ppi = (int64_t)is * is;
    m.quads = m.ppi % 4 == 0;
    m.items = m.quads ? m.ppi * B / 4 : m.ppi * B;
    m.threads = std::max(m.items, n_weights);
    return m;
}
// flags -> lists (+ zero rows)
struct CompactPlan {
    int status;
    bool launch;
    int chunks;
    unsigned wgs;
};
inline CompactPlan plan_compact(int B, int F) {
    CompactPlan c{};
    c.chunks = (int)blocks_of(F, CO_TPB * CO_PER);
    const int64_t blocks = (int64_t)B * c.chunks;
    if (!grid_ok(blocks)) { c.status = MR_ERR_BADARG; return c; }
    c.launch = blocks != 0;
    c.wgs = (unsigned)blocks;
    return c;
}

// kernel D: by strips when a workspace of the full size is available (leaves the owner list for the gather behind), else
// the plane-reading per-face walk (same results up to the order of the fp32 additions).  `gather_tex` / `gather_depth`: the
// E / F gather of the same call asks to go out INSIDE the strip kernel's launch (strip_gather_kernel); `fused` says whether it does.
// which planes the E / F gather walks: the depth term, the texture gradients, both
enum class GatherForm { NONE, DEPTH, TEX, TEX_DEPTH };
inline GatherForm gather_form(bool tex, bool depth) {
    return tex ? (depth ? GatherForm::TEX_DEPTH : GatherForm::TEX) : (depth ? GatherForm::DEPTH : GatherForm::NONE);
}

struct PixelMapPlan {
    bool strips;
    int64_t walk_threads;  // !strips: one wave per face
    StripShape shape;
    MarkPlan mark;
    bool after_mark;     // false: no face, the call ends behind the marking pass
    CompactPlan compact;
    int status_grid;     // the strip launch's own grid check
    unsigned wgs;        // strip kernel alone
    size_t lds;
    bool fused;          // the gather rides in the strip kernel's launch
    GatherForm gather;   // ... in this form
    unsigned fused_wgs, gather_groups;
};
inline PixelMapPlan plan_pixel_map(int B, int F, int is, bool strips, GatherForm gather = GatherForm::NONE, int64_t gather_threads = 0) {
    PixelMapPlan p{};
    const int64_t nfaces = (int64_t)B * F;
    p.strips = strips;  // (strips_apply: the caller asks once)
    if (!p.strips) { p.walk_threads = nfaces * WAVE; return p; }
    p.shape = strip_shape(B, is);
    p.mark = plan_mark(B, is, p.shape.n_weights);
    p.after_mark = nfaces != 0;
    p.compact = plan_compact(B, F);
    const int64_t grid = 8LL * p.shape.cap;
    p.status_grid = grid_ok(grid) ? MR_OK : MR_ERR_BADARG;
    p.wgs = (unsigned)grid;
    p.lds = (size_t)strip_lds_bytes(is, p.shape.lines);
    p.gather = gather;
    if (gather != GatherForm::NONE) {
        const int64_t gblocks = blocks_of(gather_threads, PS_T);
        const int64_t ggroups = (gblocks + 7) / 8, total = (ggroups + p.shape.cap) * 8;
        if (grid_ok(total) && ggroups <= 0x0fffffffLL) {
            p.fused = true;
            p.fused_wgs = (unsigned)total;
            p.gather_groups = (unsigned)ggroups;
        }
    }
    return p;
}

struct BackwardRequest {
    int B, F, is, ts, flags;
    float eps;
    bool grad_faces, grad_textures;  // which outputs the caller wants
    bool rgb, alpha, depth;          // which incoming gradients take part (flag set and every map of it present)
    int64_t workspace_bytes;         // 0 without a workspace
    int64_t list_bytes, full_bytes;  // what the owner list alone / the strips too need
};
struct BackwardPlan {
    bool want_d;      // D: pixel-map term (writes all 9 slots of every face row)
    bool want_f;      // F: the depth term
    bool gather_tex;  // E: texture gradients by the gather (2 x 2 x 2 textures, eps >= 1e-6), else by atomics over the pixels
    bool run_gather;  // the E / F gather runs at all
    bool strips_d;    // D by strips
    bool use_list;    // the gather walks the list of the faces that own a pixel
    bool fuse;        // D's walk and the gather ask for ONE launch (strip_gather_kernel); pixel_map.fused: they get it
    bool list_only;   // no D: the list is built for the gather alone (clear, mark, compact)
    bool tex_atomics; // grad_textures by memset + atomics over the pixels
    bool accumulate_faces, count_terms, zero_textures_in_d, zero_textures_in_list;
    PixelMapPlan pixel_map;   // want_d
    MarkPlan mark;            // list_only
    CompactPlan compact;      // list_only
    size_t tex_bytes;         // tex_atomics
    int64_t tex_threads;      // tex_atomics: one thread per pixel
    int64_t gather_threads;   // the gather as a launch of its own (run_gather and not fused), GGL lanes per face; else 0
    GatherForm gather_form;
};
inline BackwardPlan plan_render_backward(const BackwardRequest& r) {
    BackwardPlan p{};
    const int64_t nfaces = (int64_t)r.B * r.F, npx = (int64_t)r.B * r.is * r.is;
    p.want_d = r.grad_faces && (r.rgb || r.alpha);
    p.want_f = r.grad_faces && r.depth;
    p.gather_tex = r.grad_textures && r.ts == 2 && r.eps >= 1e-6f && !(r.flags & MR_FLAG_REFERENCE_ALGO);
    p.run_gather = (p.gather_tex || r.grad_faces) && (p.gather_tex || p.want_f || !p.want_d);
    // with a workspace the faces that own a pixel are listed once (kernel D needs the list anyway) and the gather
    // walks only those: the others -- four fifths of a hand + object mesh -- get their zero rows when the list is built
    p.strips_d = strips_apply(r.B, r.F, r.is, r.workspace_bytes, r.full_bytes, r.flags);
    p.use_list = p.want_d ? p.strips_d
                          : (r.workspace_bytes > 0 && r.workspace_bytes >= r.list_bytes && !(r.flags & MR_FLAG_REFERENCE_ALGO) && nfaces <= 0xffffffffLL);
    p.accumulate_faces = p.want_d;
    p.count_terms = (r.flags & MR_FLAG_COUNT_PIXEL_MAP_TERMS) != 0;
    const int64_t gather_threads = nfaces * GGL;
    p.gather_form = gather_form(p.gather_tex, p.want_f);
    bool gathered = false;
    if (p.want_d) {
        p.zero_textures_in_d = p.use_list && p.run_gather && p.gather_tex;
        // Round 5: kernel D's walk and the E / F gather go out as ONE launch when both run over the owner lists
        // (strip_gather_kernel)
        p.fuse = p.use_list && p.strips_d && p.run_gather && (p.gather_tex || p.want_f);
        p.pixel_map = plan_pixel_map(r.B, r.F, r.is, p.strips_d, p.fuse ? p.gather_form : GatherForm::NONE, gather_threads);
        gathered = p.pixel_map.fused;
    } else if (p.use_list && p.run_gather) {
        p.list_only = true;
        p.mark = plan_mark(r.B, r.is, 0);
        p.compact = plan_compact(r.B, r.F);
        p.zero_textures_in_list = p.gather_tex;
    }
    p.tex_atomics = r.grad_textures && !p.gather_tex;
    if (p.tex_atomics) {
        p.tex_bytes = (size_t)nfaces * r.ts * r.ts * r.ts * 3 * sizeof(float);
        p.tex_threads = npx;
    }
    if (p.run_gather && !gathered) p.gather_threads = gather_threads;
    return p;
}

// ---- the vertex-colour backward and the tile scatter (raster_bwd_vc.hip) --------------------------------------------------
struct ScatterVCPlan {
    int status;
    bool scatter;       // pixel-parallel scatter when the per-image colour table fits LDS (MR_FLAG_FORCE_GATHER: the gather)
    int rx_n, ry_n;     // regions per row / column
    unsigned wgs;
    size_t lds;         // the table
    int64_t gather_threads;  // !scatter: GLPF lanes per face
};
inline ScatterVCPlan plan_scatter_vc(int B, int V, int F0, int is, int flags) {
    ScatterVCPlan p{};
    const int64_t table_bytes = (((int64_t)V * 3 + 1) / 2) * 16;
    if (table_bytes <= SV_MAX_TABLE_BYTES && !(flags & MR_FLAG_FORCE_GATHER)) {
        p.scatter = true;
        p.rx_n = (int)blocks_of(is, SV_W); p.ry_n = (int)blocks_of(is, SV_H);
        const int64_t blocks = (int64_t)B * p.rx_n * p.ry_n;
        if (!grid_ok(blocks)) p.status = MR_ERR_BADARG;
        p.wgs = (unsigned)blocks;
        p.lds = (size_t)table_bytes;
        return p;
    }
    if (is > MAX_GATHER_VC_RASTER) { p.status = MR_ERR_BADARG; return p; }
    p.gather_threads = (int64_t)B * F0 * GLPF;
    return p;
}

// the tile walk reads 4-pixel groups with 16-byte loads and keeps the colour table in LDS: three sums per vertex for a
// colour-space gradient, two for a flow-space one
struct ScatterPlan {
    int status;
    int tiles_x, tiles_y, groups;
    unsigned wgs;
    size_t lds;
};
inline ScatterPlan plan_scatter_tiles(int B, int V, int is, bool colour_space, bool pairs) {
    ScatterPlan p{};
    const int64_t table_bytes = (((int64_t)V * (colour_space ? 3 : 2) + 1) / 2) * 16;
    p.tiles_x = (int)blocks_of(is, ST_TW); p.tiles_y = (int)blocks_of(is, ST_TH);
    if (is % 4 != 0 || table_bytes > SV_MAX_TABLE_BYTES || (int64_t)p.tiles_x * p.tiles_y > ST_MAX_TILES) { p.status = MR_ERR_NOTIMPL; return p; }
    // workgroups per image.  mr_render_flow_backward: ST_G.  The pair launches walk a workgroup's covered tiles a wave (the
    // pair loss's backward, pass 1: two tiles, one behind the other) at a time, and larger rasters have more of them per image
    // (a sixth of 256 / 900 / 1600 tiles), so they get more workgroups, ~8 tiles each: 8 / 32 / 32.  A 480 x 480 pair at
    // B = 8: 73 -> 46 us (mr_flow_pair_backward_tiles), 30 -> 19 us (_unit_tiles) with 32 instead of 8; 640 x 640 at B = 32:
    // 86 -> 74 us cold (_unit_tiles)
    p.groups = ST_G;
    while (pairs && p.groups < ST_G_MAX && p.tiles_x * p.tiles_y > 48 * p.groups) p.groups *= 2;
    const int64_t blocks = (int64_t)B * p.groups;
    if (!grid_ok(blocks)) { p.status = MR_ERR_BADARG; return p; }
    p.wgs = (unsigned)blocks;
    p.lds = (size_t)table_bytes;
    return p;
}

// The scalar arithmetic of the scatter's kernels (scatter_tiles_body): what a workgroup derives from the images' counts of
// covered tiles, its index and the launch's grid.  The kernel does the sums over the images with wave scans and calls these per
// element; tests/host/launch_plan_cases.cpp calls them in plain loops.
//
// The split (WORK): q = tiles per workgroup, at least one per wave, such that sum st_parts(n_b, q) fits the grid.  First try
// q = ST_WAVES; where that needs more workgroups than the launch has, st_second_q and a second sum, clamped by st_used.
MR_PLAN_HD inline int st_parts(int n, int q) { return (n + q - 1) / q; }  // workgroups of an image with n covered tiles
MR_PLAN_HD inline int st_second_q(int N, int grid, int B2) {  // N = the launch's covered tiles
    const int room = grid - B2 > 1 ? grid - B2 : 1;           // (sum ceil(n_b / q) <= N / q + B2)
    const int q = (N + room - 1) / room;
    return q > ST_WAVES ? q : ST_WAVES;
}
// (grid <= images: cannot be; the surplus images would go without a gradient)
MR_PLAN_HD inline int st_used(int used, int grid) { return used > grid ? grid : used; }
// Logical index -> slot of the `used` workgroups with work, where the grid is a multiple of 8 (else the index is the slot).
// xcd_remap gave XCD x the logical indices [x grid / 8, (x + 1) grid / 8): it takes the slots [x used / 8, (x + 1) used / 8) with
// the first of them -- every XCD the same share of the work, images in list order (as the forward's tile list hands them to the
// XCDs), divisions by 8 only.  Index lidx is the j-th of its XCD, which has n slots from k0 on: slot k0 + j, none when j >= n.
struct StSlot {
    int k0, j, n;
};
MR_PLAN_HD inline StSlot st_slot(int lidx, int grid, int used) {
    const int per = grid >> 3, x = lidx / per;
    const int k0 = (int)(((long long)x * used) >> 3), k1 = (int)(((long long)(x + 1) * used) >> 3);
    return StSlot{k0, lidx - x * per, k1 - k0};
}
// workgroup `part` of the pb that share an image's list of nb tiles takes the tiles [first, first + n)
struct StShare {
    int first, n;
};
MR_PLAN_HD inline StShare st_share(int nb, int pb, int part) {
    const int each = nb / pb, rem = nb % pb;
    return StShare{part * each + (part < rem ? part : rem), each + (part < rem ? 1 : 0)};
}
// The fixed point.  A table cell receives at most 3 terms per pixel (a face may name one vertex three times) of every tile the
// workgroup walks -- workgroup `part` of G, a wave per tile, over a list of n_hits --, each below 2^ST_FIX_BITS in magnitude:
// 2^13 of them fit the 51-bit field of the sums.  A workgroup with more (beyond ten covered tiles: large rasters, screen-filling
// meshes) gives up one bit of the 37 per doubling -- at 256 tiles per workgroup that is still 2^-32 of the largest gradient per
// term.
MR_PLAN_HD inline int st_tiles_walked(int n_hits, int part, int G) {
    const int rem = n_hits - part * ST_WAVES;
    const int rounds = rem / (G * ST_WAVES), tail = rem % (G * ST_WAVES);  // full rounds of the G workgroups' waves, and the last
    return rounds * ST_WAVES + (tail < ST_WAVES ? tail : ST_WAVES);
}
MR_PLAN_HD inline long long st_terms(int n_hits, int part, int G) { return 3LL * ST_TW * ST_TH * st_tiles_walked(n_hits, part, G); }
MR_PLAN_HD inline int st_headroom(long long terms) {
    int headroom = 0;
    while ((terms >> headroom) >= (1LL << (ST_SUM_BITS - ST_FIX_BITS))) headroom++;
    return headroom;
}
// ... and the binary point of the terms: bm = the float bits of the workgroup's largest |gradient|
MR_PLAN_HD inline int st_shift(int headroom, unsigned bm) { return ST_FIX_BITS - headroom - ((int)(bm >> 23) - 126); }

// ---- the listed pair-loss forward (warp_tiles.hip: launch_flow_pair_forward) -----------------------------------------------
// the form -- records / unit gradient / loss only --, the criterion and the batch's element types are chosen once per launch
struct PairFwdPlan {
    enum Form { LOSS_ONLY, UNIT_GRAD, RECORDS } form;
    enum Types { F32_F32, BF16_U8, BF16_F32 } types;
    bool l2;
    int tiles_x, tiles_y;
    unsigned wgs, finalize_wgs;
};
inline PairFwdPlan plan_pair_forward(int B, int is, bool records, bool grad, int criterion, int image_dtype, int mask_dtype, int64_t tile_bound,
                                     int64_t list_capacity) {
    PairFwdPlan p{};
    p.form = records ? PairFwdPlan::RECORDS : grad ? PairFwdPlan::UNIT_GRAD : PairFwdPlan::LOSS_ONLY;
    p.types = image_dtype == MR_DTYPE_F32 ? PairFwdPlan::F32_F32 : mask_dtype == MR_DTYPE_U8 ? PairFwdPlan::BF16_U8 : PairFwdPlan::BF16_F32;
    p.l2 = criterion == MR_CRITERION_L2;
    p.tiles_x = (int)blocks_of(is, 32); p.tiles_y = (int)blocks_of(is, 8);
    p.wgs = listed_grid(tile_bound, list_capacity);
    p.finalize_wgs = (unsigned)B;
    return p;
}

}  // namespace mr
