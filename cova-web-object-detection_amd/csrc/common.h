// Internal helpers shared by the gfx950 kernels of the CoVA hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>

// The public C ABI, in front of every definition: a COVA_API function that disagrees with its prototype, or has none, does
// not compile (-Werror=missing-prototypes, _build.py).  COVA_ERR_BAD_ARG, COVA_GAT_MAX_K and cova_bn_tail come from it.
#include "../../include/cova_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define COVA_OK 0

#define COVA_LAUNCH_CHECK()                         \
    do {                                            \
        hipError_t e__ = hipGetLastError();         \
        if (e__ != hipSuccess) return (int)e__;     \
    } while (0)

// One kernel launch (no dynamic LDS) and its own check: returns the launch's error from the enclosing function.
#define COVA_LAUNCH(kernel, grid, block, stream, ...)                           \
    do {                                                                        \
        hipLaunchKernelGGL((kernel), grid, block, 0, stream, __VA_ARGS__);      \
        COVA_LAUNCH_CHECK();                                                    \
    } while (0)

#define COVA_REQUIRE(cond)                          \
    do {                                            \
        if (!(cond)) return COVA_ERR_BAD_ARG;       \
    } while (0)

#define COVA_API extern "C" __attribute__((visibility("default")))

// v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32], exact f32 FMA chain.
// lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31];
// D register r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int mfma32_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the 16 lanes of a DPP row (lanes 16r..16r+15); every lane ends up with the row's total.
// Four v_add_f32 with DPP operands (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror) instead of four ds_bpermute round trips through the LDS crossbar.
__device__ __forceinline__ float row16_sum(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// fmaxf form: a NaN operand is dropped, whichever side it is on
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// compare form (f32 compares): an incoming NaN never wins and a lane's own value is kept unless a greater one arrives.
// Not wave_max: the two differ on NaN and on the sign of zero; rank.hip's maxima are defined by this one.
__device__ __forceinline__ float wave_max_gt(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        if (u > v) v = u;
    }
    return v;
}

// the xor butterfly in float64 and in integers: every lane ends with the same bits (loss.hip, rank.hip, optim.hip; the
// counts of eval.hip, mine.hip, sample.hip)
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// 64-bit counter hash: word idx of the stream `seed` (the splitmix64 finaliser over seed + golden * (idx + 1))
__device__ __forceinline__ unsigned long long hash_mix64(unsigned long long seed, unsigned long long idx)
{
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// counter-based uniform in [0,1) of the dropout masks (models.py:84,88): element idx of the stream `seed`
__device__ __forceinline__ float hash_uniform(unsigned long long seed, unsigned long long idx)
{
    return (float)(hash_mix64(seed, idx) >> 40) * (1.0f / 16777216.0f);   // 24 random bits -> [0,1)
}

// Attention dropout of the graph-attention kernels (roi_gat.hip, gat_v2.hip): rate p, inv = 1.f / (1.f - p), stream seed.
// Slot e = i*K + k of the neighbour table is kept when its uniform is >= p (the convention of dropout_fwd_kernel); no mask
// is stored, every kernel that needs it calls gat_dropped() on the same (seed, e).
struct GatDrop {
    float p, inv;
    unsigned long long seed;
};

static inline GatDrop gat_drop_of(float p, unsigned long long seed) { return GatDrop{p, 1.f / (1.f - p), seed}; }

// v * inv on a kept slot, 0 on a dropped one: ONE rounded f32 multiply (never contracted into a neighbouring add), so the
// forward and both sides of the backward form the same dropped weight bit for bit
__device__ __forceinline__ float gat_dropped(const GatDrop &dr, size_t e, float v)
{
    return hash_uniform(dr.seed, e) >= dr.p ? __fmul_rn(v, dr.inv) : 0.f;
}

// Neighbour id of one slot of the table ctx [N,K] (slot = i*K + k), as every wave-per-node GAT kernel reads it: an id >= N
// is memory-safe and acts as a pad (-1), like the table's own -1 entries; ids fit an int (N does).
__device__ __forceinline__ int gat_slot_id(const int64_t *__restrict__ ctx, size_t slot, int N)
{
    const long long j = ctx[slot];
    return j >= N ? -1 : (int)j;
}

// Edge geometry (cova_gat_fwd_edge / cova_gat_bwd_edge, cova_gat2_*): the additive score term of one slot,
// edge_w . phi[slot][0:8], as one fma chain in feature order.  A forward and its source-side backward both call this, so
// the LeakyReLU slope the backward takes is the one the forward took, bit for bit.  phi rows are 32 bytes, 16-byte aligned:
// two 16-byte loads.
__device__ __forceinline__ float gat_edge_term(const float *__restrict__ phi, size_t slot, const float *__restrict__ edge_w)
{
    const float4 p0 = *reinterpret_cast<const float4 *>(phi + slot * 8);
    const float4 p1 = *reinterpret_cast<const float4 *>(phi + slot * 8 + 4);
    float g = edge_w[0] * p0.x;
    g = fmaf(edge_w[1], p0.y, g);
    g = fmaf(edge_w[2], p0.z, g);
    g = fmaf(edge_w[3], p0.w, g);
    g = fmaf(edge_w[4], p1.x, g);
    g = fmaf(edge_w[5], p1.y, g);
    g = fmaf(edge_w[6], p1.z, g);
    g = fmaf(edge_w[7], p1.w, g);
    return g;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

// ---- host-side launch helpers
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// 16-byte accesses of a row-major operand: aligned base, leading dimension a multiple of 4 floats (an absent operand passes)
static inline bool vec4_ok(const void *p, int ld) { return p == nullptr || (aligned16(p) && (ld & 3) == 0); }

// blocks of 256 threads for a grid-stride kernel over n items, at most `cap` blocks and at least one
static inline int capped_grid(long long n, long long cap)
{
    const long long g = cdivll(n, 256);
    return (int)(g > cap ? cap : g < 1 ? 1 : g);
}
static inline int ew_grid(long long n) { return capped_grid(n, 256 * 16); }      // the elementwise kernels of bn.hip and head.hip
static inline int grid_for(long long n) { return capped_grid(n, 256 * 32); }     // the thread-per-item kernels of input.hip and sample.hip
