// The block -> tile mapping of the eye pass and its workgroup shapes (GridParams and the tile constants: cgrt_frame.h).  Part of libcgrt.so (cgrt_hip.hip).
#ifndef CGRT_GRID_HPP
#define CGRT_GRID_HPP
#include "cgrt_device_math.hpp"
#include "cgrt_frame.h"  // GridParams, the workgroup / tile constants
#include "cgrt_sphere_mask.h"  // global_row

static constexpr uint32_t kNoWaveTile = 0xffffffffu;
// Workgroup shapes.  NT = 256: four waves on a 32x8-pixel tile (2x2 sub-tiles of 16x4).  NT = 64: ONE wave on a 16x4 tile --
// a workgroup's wave slots and LDS are only handed on when its LAST wave retires, so with four very unequal waves (a
// Bezier vase covering part of a tile: a wave over it works ~100x longer than its neighbours) slots idle; with one wave
// per workgroup every slot is reused the moment its wave ends.
template <int NT>
struct TileGeom {
    static_assert(NT == 256 || NT == 64, "workgroup = 4 waves or 1 wave");
    static constexpr int W = NT == 256 ? 32 : 16, H = NT == 256 ? 8 : 4;
};

// blockIdx -> tile, XCD-aware.  Workgroups are dealt round-robin to the 8 XCDs, each with a private 4 MiB L2, so the
// blocks b, b+8, b+16, ... share an L2.  Tiles are grouped in super-tiles of kSuperW x kSuperH tiles (128 x 32 pixels);
// the blocks of one XCD group walk one super-tile after another, so the tiles an L2 serves at any moment are neighbours in
// the image and want the same tree nodes, triangles and texels -- while successive super-tiles alternate between the XCD
// groups, which keeps the expensive part of a frame (a mesh in one corner) spread over all of them.  Only placement
// changes: every tile is still rendered exactly once by exactly one workgroup.
// Measured (MI355X): C3 (glass bunny) 50.3 -> 46.6 ms, C4 (dragon) 205.5 -> 197.2 ms; but C2 4.05 -> 4.47 ms and the
// Bezier vase 8.1 -> 9.0 ms -- scenes with no tree to share, whose expensive tiles (glass sphere, vase) then sit on
// one or two XCDs.  So the launch picks it for scenes with meshes and no Bezier object, row-major otherwise.
// false: this block has no tile (edge of the super-tile grid)
__device__ __forceinline__ bool tile_of_block(const GridParams &g, int b, int &tile_x, int &tile_y, int tile_w = kTileW,
                                              int tile_h = kTileH) {
    const int tiles_x = (g.W + tile_w - 1) / tile_w, tiles_y = (g.rows + tile_h - 1) / tile_h;
    if (!g.xcd_tiles) {
        tile_x = b % tiles_x;
        tile_y = b / tiles_x;
        return true;
    }
    const int sx = (tiles_x + kSuperW - 1) / kSuperW;
    const int group = b % kXcds, q = b / kXcds;
    const int super = (q / kSuperTiles) * kXcds + group, t = q % kSuperTiles;
    tile_x = (super % sx) * kSuperW + t % kSuperW;
    tile_y = (super / sx) * kSuperH + t / kSuperW;
    return tile_x < tiles_x && tile_y < tiles_y;
}

#endif
