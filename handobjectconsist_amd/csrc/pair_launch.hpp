// pair_launch.hpp -- host side of the frame-pair path: the argument blocks and launchers that more than one .hip file uses.
// The public entry points (include/meshraster_hip.h) and mr_pair_step_forward / _backward (pair_step.hip) fill one of these
// plain structs BY FIELD NAME and hand it to the launcher, which validates it and forms the kernel's own parameter struct.
// A zero-initialised block asks for nothing optional: what is not assigned is NULL / 0 / MR_CRITERION_L1.
#pragma once
#include "mr_common.hpp"
#include "launch_plan.hpp"
#include "vertex_stage_device.hpp"

namespace mr {

// mr_render_flow_forward's arguments (raster_fwd.hip), plus what only the pair step passes:
//   pro      the vertex stage of the frame pair has NOT run yet and rides in the binning pass: `verts` (unused then),
//            `faces_idx` and `vcolors` are the buffers that stage fills -- pro->v.ndc1 / cols12 and pro->f.out point into them
//   records  [B,is,is] 16-byte records {colour 0, colour 1, alpha, mask} in place of the rgb / alpha / mask planes (listed
//            sparse launches only: the dense background stream writes planes)
struct FlowRenderArgs {
    const float* verts; const int32_t* faces_idx; const float *vcolors, *background; int bg_stride;
    const float* keep_lut; int n_lut; float alpha_thresh;
    float *rgb_img, *alpha_img, *mask_img, *depth_img, *weight_map; int32_t* face_index_map; uint8_t* tile_hit;
    void* workspace; int64_t workspace_bytes;
    int batch_size, num_verts, num_faces, fill_back, image_size; float near_, far_, eps; int flags;
    int32_t* vertex_id_map; int tile_bound; uint32_t* tile_count_out; float* zero_fill; int64_t zero_fill_count; int texel_layout;
    const PairPrologue* pro; void* records;
};
int launch_flow_render(const FlowRenderArgs& a, hipStream_t s);

// mr_flow_pair_forward_grad_tiles' arguments (warp_tiles.hip: occlusion + flow epilogue + pair loss over the render's tile list, then
// the finalize launch).  The optional group:
//   unit_grad, unit_grad_max, loss_sum, scatter_work   without unit_grad: the loss-only form, mr_flow_pair_forward_tiles
//   mean_out, mean_of   the mean over the batch: mean_out[0] = the mean of loss_bwd + loss_fwd (mean_of = 0) or of loss_fwd
//                       (1); mean_out[1 .. B] scratch.  The list header's spare words must have been cleared with the header
//                       (MR_FLAG_TILE_LIST_CLEARED's region: the pair prologue does it)
//   reset_list          the finalize launch leaves the list header's counters zero for the next step
//   records             the render's 16-byte pixel records [2B,is,is] in place of the mask / flow / scale planes, which are
//                       not looked at then (needs unit_grad); occl1 / occl2 may be NULL -- the occlusion maps are not kept
//   image_dtype, mask_dtype   MR_DTYPE_* of image_ref / image and of jitter_ref / jitter (zero: fp32); (F32, F32), (BF16, U8)
//                       and (BF16, F32) have kernels
struct FlowPairFwdArgs {
    const float *mask_flow1, *mask_flow2, *flow12, *flow21; int64_t flow_bstride; const float *flow12_scale, *flow21_scale;
    float *occl1, *occl2, *flow_out12, *flow_out21; const uint8_t *tile_hit1, *tile_hit2;
    const void *image_ref, *image, *jitter_ref, *jitter; int jitter_channels;
    void* workspace; int64_t workspace_bytes; float *sums, *loss_fwd, *loss_bwd;
    int batch_size, image_size, height, width; float distance_thresh, warp_thresh, pair_thresh;
    const void *list_header, *list_entries; int64_t list_capacity, tile_bound;
    float *unit_grad, *unit_grad_max, *loss_sum; void* scatter_work; float* mean_out; int mean_of, reset_list;
    const void* records; int criterion, image_dtype, mask_dtype;
};
int launch_flow_pair_forward(const FlowPairFwdArgs& a, hipStream_t s);

// mr_flow_pair_backward_unit_tiles' arguments (raster_bwd_vc.hip), plus the two extra incoming gradients of mr_pair_step_backward:
// of loss_bwd + loss_fwd and of the batch mean (ScatterTilesParams::gl_sum / gl_mean; mean_of as in the forward)
struct UnitScatterArgs {
    const int32_t* face_index_map; const uint32_t* tile_hit; const float* weight_map; const int32_t* vertex_id_map;
    const float *unit_grad, *unit_grad_max, *sums, *grad_loss_fwd, *grad_loss_bwd, *grad_loss_sum, *grad_mean; int mean_of;
    int height, width; float* grad_vcolors; int batch_size, num_verts, num_faces, fill_back, image_size; float eps;
    int flags, texel_layout; const void* scatter_work;
};
int launch_unit_scatter_tiles(const UnitScatterArgs& a, hipStream_t s);

}  // namespace mr
