// launch_plan_cases.cpp -- what csrc/launch_plan.hpp decides for a pair step's render and scatter at given mesh sizes, one line
// per row of standard input, on a device of 256 compute units.  tests/test_pair_mesh_cases_host.py builds it with the host
// compiler, feeds it the shapes of tests/pair_mesh_cases.py and asserts that every mesh-dependent decision is reached by a case.
//
// input rows:  B2 V Fh Fo fill_back is      (B2 = both frames of every pair: the render's batch)
// output rows: key=value pairs, `sides` = the side of every part (pair_part_range), comma-separated
#include "../../handobjectconsist_amd/csrc/launch_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mr;

// `launch_plan_cases scatter`: the pair step's backward scatter (unit_scatter_tiles_kernel, raster_bwd_vc.hip) at given counts of
// covered 32 x 8 tiles per image, on a device of 256 compute units: how many workgroups every image gets and, for every
// workgroup, the `terms` and `headroom` the kernel computes.  tests/test_pair_upstream_cases_host.py feeds it the oracle's
// coverage.
// input rows:  B2 V is n_0 ... n_(B2-1)
// output rows: groups=<plan's workgroups per image> grid= q= used= per_image=<workgroups of image 0,1,..> wgs=<image.tiles.terms.headroom;...> max_headroom=
//
// Every figure comes from the functions the kernel itself calls (launch_plan.hpp: st_parts, st_second_q, st_used, st_share,
// st_terms, st_headroom); what is written out here is only the kernel's sums over the images, which it does with wave scans, and
// the walk over the workgroups: image b takes slots [base, base + parts) of the `used` slots, every slot below `used` is taken by
// one workgroup (the XCD shares [x used / 8, (x + 1) used / 8) tile [0, used): st_slot, checked for every row), and a workgroup
// walks its share as part 0 of 1.
static int scatter_cases() {
    int B2, V, is;
    while (std::scanf("%d %d %d", &B2, &V, &is) == 3) {
        if (B2 <= 0 || B2 > 4096) return 1;
        std::vector<int> ncov(B2);
        for (int b = 0; b < B2; b++)
            if (std::scanf("%d", &ncov[b]) != 1 || ncov[b] < 0) return 1;
        const ScatterPlan s = plan_scatter_tiles(B2, V, is, false, true);
        if (s.status != 0) { std::printf("status=%d\n", s.status); continue; }
        const int grid = (int)s.wgs, T = s.tiles_x * s.tiles_y;
        int q = ST_WAVES, used = 0, N = 0;
        for (int n : ncov) {
            if (n > T) return 1;
            N += n; used += st_parts(n, ST_WAVES);
        }
        if (used > grid) {
            q = st_second_q(N, grid, B2);
            used = 0;
            for (int n : ncov) used += st_parts(n, q);
            used = st_used(used, grid);
        }
        // (the walk below relies on it: the logical indices of the grid take every slot below `used` exactly once -- a grid that
        // is a multiple of 8 through st_slot, as the kernel does)
        std::vector<int> taken(used, 0);
        for (int l = 0; l < grid; l++) {
            const StSlot sl = (grid & 7) == 0 ? st_slot(l, grid, used) : StSlot{0, l, used};
            if (sl.j < sl.n && (sl.k0 + sl.j < 0 || sl.k0 + sl.j >= used || taken[sl.k0 + sl.j]++ != 0)) return 1;
        }
        if (std::count(taken.begin(), taken.end(), 1) != used) return 1;
        std::printf("status=0 groups=%d grid=%d q=%d used=%d per_image=", s.groups, grid, q, used);
        for (int b = 0; b < B2; b++) std::printf("%s%d", b ? "," : "", st_parts(ncov[b], q));
        std::printf(" wgs=");
        int base = 0, max_headroom = 0;
        bool first = true;
        for (int b = 0; b < B2; b++) {
            const int nb = ncov[b], pb = st_parts(nb, q);
            for (int part = 0; part < pb && base + part < used; part++) {
                const int n_hits = st_share(nb, pb, part).n;
                const long long terms = st_terms(n_hits, 0, 1);
                const int headroom = st_headroom(terms);
                std::printf("%s%d.%d.%lld.%d", first ? "" : ";", b, n_hits, terms, headroom);
                first = false;
                max_headroom = std::max(max_headroom, headroom);
            }
            base += pb;
        }
        std::printf(" max_headroom=%d\n", max_headroom);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "scatter") == 0) return scatter_cases();
    int B2, V, Fh, Fo, fill_back, is;
    while (std::scanf("%d %d %d %d %d %d", &B2, &V, &Fh, &Fo, &fill_back, &is) == 6) {
        // the request of mr_pair_step_forward's render (raster_fwd.hip: launch_bins under launch_flow_render)
        BinRequest r{};
        r.vc = true; r.B = B2; r.F0 = Fh + Fo; r.F = fill_back ? 2 * r.F0 : r.F0; r.V = V; r.fill_back = fill_back != 0; r.is = is;
        r.flags = 0; r.cus = 256; r.want_list = true; r.list_cleared = true; r.pair = true; r.Fh = Fh; r.Fo = Fo;
        const BinPlan p = plan_bins(r);
        const int K = p.parts, F0 = Fh + Fo;
        // Kh as pair_part_range rounds it, before and after its clamp (-1: no split)
        int kh_raw = -1, kh = -1;
        if (K >= 2 && Fh > 0 && Fo > 0) {
            kh_raw = (int)(((int64_t)K * Fh + F0 / 2) / F0);
            kh = kh_raw < 1 ? 1 : (kh_raw > K - 1 ? K - 1 : kh_raw);
        }
        std::printf("status=%d parts=%d two_launches=%d lds_boxes=%d prologue=%d faces=%d form=%d lds=%zu lds_opt_in=%d kh_raw=%d kh=%d", p.status,
                    p.parts, (int)p.two_launches, p.lds_boxes, (int)p.prologue, (int)p.faces, (int)p.form, p.lds, (int)p.lds_opt_in, kh_raw, kh);
        std::printf(" sides=");
        int hand_parts = 0, least_obj = -1;
        for (int k = 0; k < K; k++) {
            int r0, nr;
            const int side = pair_part_range(k, K, Fh, Fo, r0, nr);
            std::printf("%s%d", k ? "," : "", side);
            hand_parts += side == 0;
            if (side == 1 && (least_obj < 0 || nr < least_obj)) least_obj = nr;
        }
        // (the clamp as the parts show it: hand parts counted from the sides must equal kh)
        const ScatterPlan s = plan_scatter_tiles(B2, V, is, false, true);
        const ScatterPlan c = plan_scatter_tiles(B2, V, is, true, true);
        std::printf(" hand_parts=%d least_obj_faces=%d groups=%d scatter_status=%d colour_table=%zu colour_status=%d\n", hand_parts, least_obj, s.groups,
                    s.status, c.lds, c.status);
    }
    return 0;
}
