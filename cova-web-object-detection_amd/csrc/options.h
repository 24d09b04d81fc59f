// The library's process-wide option state (cova_set_option): one struct, one owner (options.hip).
#pragma once
#include <atomic>

struct CovaOptions {
    int grid_cap = 0;        // key 2: > 0 caps the persistent grids (tests force many tiles per block)
    int conv1_f32 = 0;       // key 7: 1 = conv1 forward and weight gradient on the f32 MFMA kernels instead of the bf16-split ones
    int wino4_f32 = 0;       // key 9: 1 = the F(4x4,3x3) main loop in f32 instead of the bf16 split
    int bn1d_variant = 1;    // key 14: != 0 = the float4 row kernels where the operands allow it, 0 = the 128-slice form
    int gat_wide = 1;        // key 16: 1 = the GAT kernels' wide form <KP = 1, ND> where it applies (K <= 64, D <= 512: every 64-channel chunk of a neighbour row in flight), 0 = always the chunk form <KP, ND = 1> (roi_gat.hip, gat_form)
    int sgemm_dma = 1;       // key 22: 1 = the LDS-DMA sgemm kernel wherever the operands allow it
    std::atomic<bool> frozen{false};
};

extern CovaOptions g_cova_options;     // options.hip; only cova_set_option touches it directly

// Every consumer of an option reads through here, so an option cannot be used without the state becoming fixed.
inline const CovaOptions &cova_options()
{
    if (!g_cova_options.frozen.load(std::memory_order_relaxed)) g_cova_options.frozen.store(true, std::memory_order_relaxed);
    return g_cova_options;
}

// min(ntiles, compute units of the current device * blocks_per_cu), under the grid cap (options.hip)
int cova_internal_persistent_grid(int ntiles, int blocks_per_cu = 1);
