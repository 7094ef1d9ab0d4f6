// gallery_nearest_plan.h -- what rfd_gallery_nearest (include/rfd.h, "nearest") decides on the host before anything is enqueued:
// which form of the scan runs, how rows [row0, row0 + n) are cut into A tiles, how the gallery's row blocks are cut into B
// splits, the grid and the workspace.  Plain host code: nothing of HIP is included, so tests/cpp/gallery_nearest_plan_check.cpp
// builds it with the host compiler alone.  gallery_host.hip does what is planned here; kernels_gallery_nearest.hip launches it.
//
// The decomposition.  A workgroup (four waves) owns one A tile of `tile_rows` rows and one B split.  The row blocks of 16 are
// dealt to the splits in groups of four consecutive blocks, round-robin: group b / 4 belongs to split (b / 4) % splits, and wave
// w of the workgroup takes block 4 * group + w.  So the workgroups of one tile, which run side by side, sweep the gallery
// together as the search's workgroups do, instead of each streaming a region of its own.  The grid is tiles x splits
// with the tile as the fast index, so workgroups that run side by side for different tiles walk the SAME split and share its
// bytes in L2.
//   Many A rows: tiles >= the target of workgroups, splits = 1, and HBM/L2 traffic is tiles x the gallery's bytes.
//   Few A rows: the gallery is split until tiles x splits reaches the target, as long as a split keeps a group of blocks; the
//   merge kernel reduces the splits' keys, so 32 new rows against a million still occupy every CU.
// The target is four workgroups per CU: the register-stationary form runs one workgroup per CU at a time, and with four times
// as many, smaller, workgroups than CUs the last round is at most a quarter empty.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rfd {

constexpr int kNearestFormLds = 0;       // A fragments in LDS, any dim the gallery accepts: 32 rows per tile
constexpr int kNearestFormRegisters = 1; // A fragments in registers, K loop unrolled at compile time, dim 512: 64 rows per tile
constexpr int kNearestWaves = 4;         // waves of a workgroup; each takes every fourth block of the split
constexpr int kNearestTargetPerCu = 4;   // workgroups per CU a call is split into while the gallery allows it

struct GalleryNearestPlan {
    int form;             // kNearestForm*
    int tile_rows;        // A rows of a workgroup, a multiple of 16
    int tiles;            // ceil(n / tile_rows); tile t owns rows [row0 + t * tile_rows, ...) of the call
    int splits;           // B splits; split s owns the row blocks b < blocks with (b / kNearestWaves) % splits == s
    int blocks;           // ceil(rows / 16)
    int blocks_per_split; // the most blocks a split owns; every split owns at least one
    int64_t grid;         // tiles * splits workgroups (grid.x, tile fast); 0: nothing to launch
    int64_t ws_bytes;     // splits * n keys of 8 bytes
};

constexpr int kNearestRegisterMinRows = 33; // A rows of a call from which dim 512 takes the register form (see below)
constexpr int kNearestMaxTileRows = 64;

// The form and the tile of a call: the one place where they are chosen.  The register form keeps 64 A rows per workgroup, pays
// for them with one wave per SIMD, and its MFMAs do not wait for LDS; the LDS form keeps 32 rows and runs several workgroups
// per CU.  Measured at dim 512 on 1 M rows (profiles/gallery_nearest.txt): the register form is 1.4 to 2 times faster from 64
// A rows up, the LDS form 8 % faster at 32, where one of its tiles holds the whole call and the register form's second half
// would be padding.  So a call of at most 32 rows takes the LDS form.
inline int gallery_nearest_form(int dim, int n) { return dim == 512 && n >= kNearestRegisterMinRows ? kNearestFormRegisters : kNearestFormLds; }
inline int gallery_nearest_tile_rows(int dim, int n) { return gallery_nearest_form(dim, n) == kNearestFormRegisters ? 64 : 32; }

// The cap of the grid: tiles alone when they reach the target, else fewer than target + tiles workgroups.
inline int64_t gallery_nearest_grid_cap(int n, int dim, int cus)
{
    const int tr = gallery_nearest_tile_rows(dim, n);
    return ((int64_t)n + tr - 1) / tr + (int64_t)kNearestTargetPerCu * cus;
}

// Bytes a gallery's workspace must hold for any call on at most `capacity` rows: splits * n <= target * tile_rows + n keys.
inline int64_t gallery_nearest_ws_bound(int capacity, int /*dim*/, int cus)
{
    return ((int64_t)kNearestTargetPerCu * cus * kNearestMaxTileRows + capacity) * 8;
}

// rows: the rows handed out (B side); [row0, row0 + n): the A rows, within them; dim: a multiple of 32 in 32..1024; cus >= 1.
// Arguments outside that give grid = 0.
inline GalleryNearestPlan gallery_nearest_plan(int rows, int row0, int n, int dim, int cus)
{
    GalleryNearestPlan p = {};
    p.form = gallery_nearest_form(dim, n);
    p.tile_rows = gallery_nearest_tile_rows(dim, n);
    if (rows < 1 || row0 < 0 || n < 1 || n > rows - row0 || dim < 32 || dim > 1024 || dim % 32 != 0 || cus < 1) return p;
    p.tiles = (int)(((int64_t)n + p.tile_rows - 1) / p.tile_rows);
    p.blocks = (int)(((int64_t)rows + 15) / 16);
    const int64_t target = (int64_t)kNearestTargetPerCu * cus;
    int64_t want = p.tiles >= target ? 1 : (target + p.tiles - 1) / p.tiles;         // splits that reach the target
    const int64_t groups = ((int64_t)p.blocks + kNearestWaves - 1) / kNearestWaves;  // of four consecutive blocks; the last may be partial
    if (want > groups) want = groups;                                                // no split is empty
    p.splits = (int)want;
    const int64_t most = ((groups + want - 1) / want) * kNearestWaves;
    p.blocks_per_split = (int)(most < p.blocks ? most : p.blocks);
    p.grid = (int64_t)p.tiles * p.splits;
    p.ws_bytes = (int64_t)p.splits * n * 8;
    return p;
}

} // namespace rfd
