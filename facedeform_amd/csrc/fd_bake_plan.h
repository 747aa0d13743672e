// fd_bake_plan.h -- the layout fd_bake.hip's pack kernel writes and its launch reads: one place for the
// constants, so that the two cannot disagree (fd_shared_plan.h is the precedent).  Host and device.
//
// The product is B = f . Psi S': N x (C + 4) by (C + 4) x M on v_mfma_f64_16x16x4_f64.  The vertices are the FIRST operand's
// rows (lane l: vertex l & 15, depth l >> 4), S' the second's columns (lane l: column l & 15, depth l >> 4), so accumulator
// register r of lane l is entry (vertex (l >> 4) + 4 r, column l & 15): sixteen consecutive lanes hold sixteen consecutive
// columns of one row of B, a 128-byte run.
//
// Depth.  A step is 4 rows of S' in the records' order: ceil(C / 4) steps of records (rows past C are 0.0 against a centre
// record of zeros), then ONE step for the polynomial rows 1, x, y, z.
// Columns.  M is cut into 16-column tiles, the tiles into `panels` panels of `ntp` tiles each (ntp <= kPanelTiles: 256 columns,
// 128 accumulator registers); columns past M are 0.0.  The panels are made equal, so a rig just above 256 points runs two
// panels of half the width, not a full one and a sliver.
// The gradient launch (fd_deform_bake_grad*) is the same product with three first operands per depth step and
// so three accumulators per tile: its panels are capped at kGradPanelTiles tiles.  plan() takes the cap; the layout below is the
// same text for both, and the pack kernel writes either.
// Scratch, in doubles:
//   [0, 16 steps)                      the centre records {cx, cy, cz, s}, four per step; the polynomial step's are zeros
//   [16 steps, + panels steps ntp 64)  S' in operand-tile order: ((panel steps + step) ntp + tile) 64 + lane
#pragma once
#include <stddef.h>

namespace fd {
namespace bake {

constexpr int kWaves = 8;                    // waves of a workgroup
constexpr int kBlock = 64 * kWaves;
constexpr int kTile = 16;                    // vertices of a wave, columns of a tile
constexpr int kGroup = kTile * kWaves;       // vertices of a workgroup
constexpr int kPanelTiles = 16;              // tiles of a panel at most
constexpr int kGradComps = 3;                // the gradient launch: accumulators per tile, one per component of x
constexpr int kGradPanelTiles = 4;           // tiles of a panel of the gradient launch at most
constexpr int kPackThreads = 256;

struct Plan {
    int C, M;            // records, columns
    int steps;           // depth steps, the polynomial step included
    int tiles;           // 16-column tiles of M
    int panels, ntp;     // panels, tiles per panel
    __host__ __device__ size_t cen_doubles() const { return (size_t)16 * steps; }
    __host__ __device__ size_t tile_at(int panel, int step, int tile) const
    {
        return cen_doubles() + (((size_t)panel * steps + step) * ntp + tile) * 64;
    }
    __host__ __device__ size_t doubles() const { return tile_at(panels, 0, 0); }
    // LDS doubles of one staged step: its four centre records and its ntp operand tiles
    __host__ __device__ int step_doubles() const { return 16 + 64 * ntp; }
};

// cap: tiles of a panel at most (kPanelTiles, or kGradPanelTiles for the gradient launch)
__host__ __device__ inline Plan plan(int C, int M, int cap = kPanelTiles)
{
    Plan p;
    p.C = C; p.M = M;
    p.steps = (C + 3) / 4 + 1;
    p.tiles = (M + kTile - 1) / kTile;
    p.panels = (p.tiles + cap - 1) / cap;
    p.ntp = p.panels ? (p.tiles + p.panels - 1) / p.panels : 0;
    return p;
}

// LDS of the launch with NT accumulator tiles, in doubles: what one workgroup stages of S' and the centres at a time.  Static
// LDS (at most 64 KiB); the narrow launch keeps half, so that two of its workgroups share a compute unit.
template <int NT> constexpr int lds_doubles() { return NT > 4 ? 7280 : 3584; }

static_assert(kBlock == 512 && kGroup == 128, "eight waves of sixteen vertices");
static_assert(kPanelTiles * 4 * 2 == 128, "a panel's accumulators: 16 tiles x 4 doubles = 128 registers, the Gram kernel's budget");
static_assert(kGradPanelTiles * kGradComps * 4 * 2 == 96, "a gradient panel's accumulators: 4 tiles x 3 components x 4 doubles = 96 registers");
static_assert(kGradPanelTiles <= kPanelTiles && lds_doubles<kGradPanelTiles>() >= 16 + 64 * kGradPanelTiles, "the gradient launch stages at least one step");
static_assert(lds_doubles<16>() * 8 <= 65536 && lds_doubles<4>() * 8 <= 32768, "static LDS");
static_assert(lds_doubles<16>() >= 16 + 64 * 16 && lds_doubles<4>() >= 16 + 64 * 4, "at least one step fits");

}  // namespace bake
}  // namespace fd
