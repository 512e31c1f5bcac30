// The rasterizer forward's workspace as the backward (rasterizer_backward.hip) reads it.  The layout itself stays private
// to rasterizer.hip (carve()); this is the read-only view of what one forward left there.
#pragma once

#include <cstddef>

#include <hip/hip_runtime.h>

namespace amav {
namespace raster {

struct WorkspaceView {
    const float4 *geom;              // [F*N][3]: {x, y, qa, qb} {qc, log2(opacity), r, g} {b, 1/depth, bx, by}
    const uint4 *rectd;              // [F*N]: {cx0 | cy0 << 16, cx1 | cy1 << 16, depth bits, radius} (binned rectangle)
    const int *tile_off;             // [F*(T+1)] exclusive scan within the frame; [T] = the frame's instance count
    const unsigned long long *keys;  // [F * cap_per_frame] (depth bits << 32 | index), unsorted for lists <= sort_cap
    const unsigned *sorted;          // [F * cap_per_frame] blend order of the lists longer than sort_cap
    const int *overflow;             // device flag: some frame exceeded its region (nothing else is valid then)
    long long cap_per_frame;
    int sort_cap;                    // lists longer than this were ordered by sort_big (into `sorted`)
    size_t bytes;                    // workspace bytes the forward needs at these sizes
};

// sizes exactly as the forward call gave them (instance_capacity is the total, as in amav_raster_args)
WorkspaceView workspace_view(void *workspace, int F, int N, int H, int W, long long instance_capacity);

}  // namespace raster
}  // namespace amav
