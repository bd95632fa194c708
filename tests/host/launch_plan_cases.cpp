// launch_plan_cases.cpp -- what csrc/launch_plan.hpp decides for a pair step's render and scatter at given mesh sizes, one line
// per row of standard input, on a device of 256 compute units.  tests/test_pair_mesh_cases_host.py builds it with the host
// compiler, feeds it the shapes of tests/pair_mesh_cases.py and asserts that every mesh-dependent decision is reached by a case.
//
// input rows:  B2 V Fh Fo fill_back is      (B2 = both frames of every pair: the render's batch)
// output rows: key=value pairs, `sides` = the side of every part (pair_part_range), comma-separated
#include "../../handobjectconsist_amd/csrc/launch_plan.hpp"

#include <cstdio>

using namespace mr;

int main() {
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
