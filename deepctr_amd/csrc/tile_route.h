// Where a fused op's per-workgroup tile lives (host side): in the LDS when it fits, otherwise in a per-workgroup slice of the
// caller's workspace (the general route: persistent workgroups, one slice each — nothing is refused for its size).  One definition of
// the limits and of the slice arithmetic for every op that follows the workspace protocol.
#pragma once
#include <stddef.h>

#include "dctr_common.h"

constexpr size_t DCTR_LDS_MAX = 160 * 1024;             // one workgroup's LDS on gfx950
constexpr int DCTR_GLOBAL_WGS = 256;                    // general route: at most this many workgroups (workspace slices)
constexpr size_t DCTR_GLOBAL_MAX = (size_t)256 << 20;   // general route: at most this much workspace (but always one slice)

struct dctr_tile_route {
    bool global;            // the general route (the tile in the workspace)
    int grid_max;           // general route: workgroups the workspace has slices for
    size_t route_bytes;     // workspace of the general route (0 on the LDS route)
};

// the general route's slices for a tile of tile_bytes, whatever its size (ops that may be forced onto the workspace route)
static inline dctr_tile_route dctr_workspace_slices(size_t tile_bytes) {
    const size_t gmax = DCTR_GLOBAL_MAX / tile_bytes;
    const int grid_max = (int)(gmax < 1 ? 1 : gmax > DCTR_GLOBAL_WGS ? DCTR_GLOBAL_WGS : gmax);
    return {true, grid_max, tile_bytes * grid_max};
}

static inline dctr_tile_route dctr_plan_tile_route(size_t tile_bytes) {
    if (tile_bytes <= DCTR_LDS_MAX) return {false, 0, 0};
    return dctr_workspace_slices(tile_bytes);
}

// The launch's demand for the workspace that `entry` (the op's *_workspace_bytes function) reported: `need` bytes behind a 16-B
// aligned pointer.  op and entry are string literals: every op keeps its own message.
#define DCTR_REQUIRE_WORKSPACE(op, entry, ptr, bytes, need)                                                            \
    do {                                                                                                               \
        DCTR_REQUIRE((ptr) && (bytes) >= (need), DCTR_E_NULL, op ": this shape needs a workspace of %zu bytes (" entry ")", \
                     (size_t)(need));                                                                                  \
        DCTR_REQUIRE(dctr_aligned16(ptr), DCTR_E_ALIGN, op ": workspace not 16-B aligned");                            \
    } while (0)
