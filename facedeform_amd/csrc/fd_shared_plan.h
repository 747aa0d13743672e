// fd_shared_plan.h -- the ONE copy of what the host decides for a shared-rig fp32 launch (fd_batch_deform_shared_dev,
// fd_eval_shared.hip): which of the four kernel forms runs, where the pack kernel leaves things in the scratch, and how much
// scratch and LDS that takes.  launch_deform_shared, its two pack kernels, the vector launch that reads the same scratch
// (fd_vectors_shared.hip) and the C ABI (fd_capi.hip: scratch sizes, fd_shared_kernel_name) all take their numbers from
// shared_plan(); DESIGN.md 4.1c has the table.  Host arithmetic only: no HIP type enters, so a stand-alone program can include
// it (tests/tools/shared_plan_check.cpp), as with fd_fit_host.h.
#pragma once
#include <cstddef>

namespace fd {

constexpr size_t kSharedLdsBudget = 158 * 1024;   // of 160 KiB (one workgroup per CU)
constexpr int kGaussShift = 10;      // Gaussian kinds: phi (<= 1) enters the matrix pipe as 2^10 phi, clear of the fp16 subnormals;
                                     // the frame records' inv_scale carries 2^-10 with it
// sizeof(MfmaTileH) and sizeof(SharedFrame): fd_eval_shared.hip holds the static_assert against the structs
constexpr size_t kMfmaTileHBytes = 768;
constexpr size_t kSharedFrameBytes = 32;

// ---- up to 16 frames: 16-row output tiles (k_deform32_tps_shared), 8 waves of 64 vertices ----
// Two row layouts of the output tiles (16 rows x 16 vertices each):
//   padded (up to 12 frames): tile T holds frames 4 T .. 4 T + 3, row = 4 (frame - 4 T) + component, one row in
//     four unused -- ceil(F / 4) tiles;
//   dense (13 frames and more): frames come in blocks of 16 and a block is three tiles, one per component:
//     tile 3 B + c holds component c of frames 16 B .. 16 B + 15, row = frame - 16 B -- 3 ceil(F / 16) tiles, no
//     unused rows at F = 16.
// Either way the 4 x 4 transpose across lane groups in the epilogue leaves every lane with all rows of
// every tile for ONE vertex.
constexpr int kSharedThreads = 512;
constexpr bool shared_dense(int nF) { return nF > 12; }
constexpr int shared_tiles(int nF) { return shared_dense(nF) ? 3 * ((nF + 15) / 16) : (nF + 3) / 4; }
constexpr int shared_slots(int nT, bool dense) { return dense ? nT / 3 * 16 : nT * 4; }     // frame records

// ---- 17 to 32 frames, thin-plate and the Gaussian kinds alike: 32-row tiles ----
// (the 16-row kernel at six tiles was measured against them: 201 against 175 us at 256 centres x 32 frames)
constexpr bool shared_wide(int nF) { return nF > 16; }
constexpr int kWideSlots = 32;       // frame records the 32-row kernels load, whatever the frame count
constexpr int kWideWaves = 8;        // waves per workgroup of the two-tile kernel (k_deform32_tps_shared_wide): two per SIMD, 64 vertices each
constexpr int kW1Waves = 12;         // of the one-tile kernel (k_deform32_shared_w1): three per SIMD
constexpr int kW1Unit = 32;          // its vertices per wave and unit
// Rows of the output tiles are packed densely: row 3 f + c of the stack of 32-row tiles is component c of frame slot f, so
// 17..20 frames are TWO tiles (60 rows of 64) where one tile per component would be three -- a third fewer matrix
// instructions for a 20-frame launch.  After the epilogue's lane-half swap a lane holds every row of every tile for its own
// vertex, so any row <-> (frame, component) map costs nothing there.
// Frame slots come in fours (the fall-off rows leave four frames per store): a launch of nF frames runs
// NSLOT = 4 ceil(nF / 4) slots, and slots nF .. NSLOT - 1 are DUPLICATES of frame nF - 1 (same weights, scale and output
// pointers: the same bits stored twice to the same address) -- so every frame count takes the straight-line epilogue.
constexpr int wide_slots(int nF) { return (nF + 3) / 4 * 4; }
constexpr int wide_tiles(int nslot) { return (3 * nslot + 31) / 32; }               // 2 up to 20 slots (21 frames would fit, 24 slots do not), else 3
constexpr int wide_w16(int nt) { return nt * 2 * 2 * 64; }                          // 16-byte words of weight tiles per K block: [tile][K step][hi, lo][lane]
// LDS of the one-tile kernel beside its K blocks (the kernel lists the pieces)
constexpr size_t w1_fixed_lds(int nt) { return kSharedFrameBytes * (size_t)kWideSlots + 32 * 16 + (size_t)nt * 64 * 16 + 256 * sizeof(unsigned long long) + 16; }

struct SharedPlan {
    int variant;            // 0 padded 16-row, 1 dense 16-row, 2 32-row two-tile, 3 32-row one-tile (w1)
    int ntiles, nslot;      // row tiles and frame slots of that variant
    int nkb, kchunk;        // K blocks of 32 centres; how many of them LDS holds at a time (0: not even one fits)
    size_t poly_at, copy_at, norm_at;   // 16-byte words into the scratch: polynomial tiles, the rest rig's centre copy, its normalisation
    size_t wtile_bytes, frame_bytes;    // what the scratch must hold
    size_t lds_fixed, lds_per_kb;       // LDS = lds_fixed + lds_per_kb * kchunk
    int threads, group_vertices;        // block size, vertices per workgroup and group
    const char *kernel;
};

// Mpad: centres padded to a multiple of 16; nF: 1 .. 32 frames.  `kind` decides nothing today (thin-plate and the Gaussian
// kinds share the shapes; the kernels differ in a template argument only): it is what a caller asks with, and stays in the
// signature for the day a kind's centre records take another size.
inline SharedPlan shared_plan(int Mpad, int nF, int kind)
{
    (void)kind;
    SharedPlan q{};
    q.nkb = (Mpad / 16 + 1) / 2;
    if (!shared_wide(nF)) {
        const bool dense = shared_dense(nF);
        q.variant = dense ? 1 : 0;
        q.ntiles = shared_tiles(nF);
        q.nslot = shared_slots(q.ntiles, dense);
        // (k_pack_shared lists what lies where: 128 words of weights per tile and K block, two centre tiles per K block)
        q.poly_at = (size_t)q.nkb * q.ntiles * 128;
        q.copy_at = q.poly_at + (size_t)q.ntiles * 64;
        q.norm_at = q.copy_at + (size_t)2 * q.nkb * (kMfmaTileHBytes / 16);
        q.frame_bytes = kSharedFrameBytes * (size_t)q.nslot;
        q.lds_fixed = kSharedFrameBytes * (size_t)q.nslot + (size_t)q.ntiles * 64 * 16;
        q.lds_per_kb = 2 * kMfmaTileHBytes + (size_t)q.ntiles * 128 * 16;
        q.threads = kSharedThreads;
        q.group_vertices = kSharedThreads;          // a wave owns 64
        q.kernel = "k_deform32_tps_shared";
    } else {
        q.nslot = wide_slots(nF);
        q.ntiles = wide_tiles(q.nslot);
        // (k_pack_shared_wide: wide_w16 words of weights and 64 of d2 operands per K block)
        q.poly_at = (size_t)q.nkb * wide_w16(q.ntiles);
        q.copy_at = q.poly_at + (size_t)q.ntiles * 64;
        q.norm_at = q.copy_at + (size_t)q.nkb * 64;
        // the 32-row kernels load all kWideSlots records whatever nslot the pack kernel wrote: the scratch holds that many
        q.frame_bytes = kSharedFrameBytes * (size_t)kWideSlots;
        q.lds_per_kb = (size_t)1024 + (size_t)wide_w16(q.ntiles) * 16;
        // One vertex tile per wave, three waves per SIMD (w1) where the WHOLE model is resident in LDS -- 256 centres at 32
        // frames, 384 at 20; models staged in chunks keep the two-tile kernel, whose 512-vertex groups re-stage a quarter less
        // often.  The pack kernel deals the weight rows out differently for the two, so this is also a property of the scratch.
        const bool w1 = (kSharedLdsBudget - w1_fixed_lds(q.ntiles)) / q.lds_per_kb >= (size_t)q.nkb;
        q.variant = w1 ? 3 : 2;
        q.lds_fixed = w1 ? w1_fixed_lds(q.ntiles)
                         : kSharedFrameBytes * (size_t)kWideSlots + (size_t)q.ntiles * 64 * 16 + 512 * sizeof(unsigned long long) + 16;
        q.threads = 64 * (w1 ? kW1Waves : kWideWaves);
        q.group_vertices = w1 ? kW1Unit * kW1Waves : 64 * kWideWaves;
        q.kernel = w1 ? "k_deform32_shared_w1" : "k_deform32_tps_shared_wide";
    }
    q.wtile_bytes = (q.norm_at + 1) * 16;           // the normalisation is the last 16-byte word
    const size_t fit = (kSharedLdsBudget - q.lds_fixed) / q.lds_per_kb;
    q.kchunk = fit < (size_t)q.nkb ? (int)fit : q.nkb;
    return q;
}

}  // namespace fd
