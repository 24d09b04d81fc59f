// Helpers of the matrix-pipe kernels (conv.hip, conv1x1.hip, conv1x1_lin.hip, conv_wino4.hip, conv_wgrad4.hip, gemm.hip,
// page_attn.hip): the MFMA wrappers next to common.h's mfma32, the global -> LDS copy and the LDS-only barrier.  One
// definition each.
#pragma once
#include "bf3.h"

// v_mfma_f32_16x16x4_f32: D[16x16] += A[16x4] * B[4x16], exact f32 FMA chain
__device__ __forceinline__ f32x4 mfma16x4(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// v_mfma_f32_32x32x16_bf16 on packed bf16 pieces (bf3.h): eight k per lane and operand, four dwords
__device__ __forceinline__ f32x16 mfma32bf(u32x4 a, u32x4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// (unsigned)(size_t)(lds_void *)p: the byte address of a __shared__ object inside the LDS
typedef __attribute__((address_space(3))) void lds_void;

// global -> LDS copy of 16 bytes per lane (lane i lands at lds_base + 16 i; lds_base wave-uniform) as inline asm:
// the compiler then neither knows the copy (no conservative vmcnt(0) in front of every later LDS read, which the
// builtin gets unless each buffer is its own __shared__ object) nor waits for it -- every wait on these copies is
// an explicit s_waitcnt in the kernel.
// Address = wave-uniform base (scalar register pair) + this lane's unsigned 32-bit byte offset: no 64-bit per-lane
// pointers (which the compiler otherwise precomputes per pixel and keeps -- or spills -- across the whole loop).
__device__ __forceinline__ void copy16_to_lds(const void *base, unsigned off_bytes, unsigned lds_base_bytes)
{
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_base_bytes), "v"(off_bytes), "s"(base) : "memory", "m0");
}

// The same copy with an immediate byte offset IMM in the instruction (13-bit signed field).  The hardware adds the field to
// the global address AND to the LDS address: lane i reads base + off_bytes + IMM and lands at lds_base + LDS_ADD + IMM + 16 i.
// LDS_ADD is a constant added while m0 is written (one scalar instruction either way): the destinations of a buffer's
// pieces need ONE scalar register, not one each.
template <int IMM, int LDS_ADD>
__device__ __forceinline__ void copy16_to_lds_imm(const void *base, unsigned off_bytes, unsigned lds_base_bytes)
{
    static_assert(IMM >= 0 && IMM < 4096, "global_load_lds: 13-bit signed immediate offset");
    static_assert(LDS_ADD >= 0 && LDS_ADD < 65536, "LDS byte offset");
    if constexpr (LDS_ADD == 0)
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%3" ::"s"(lds_base_bytes), "v"(off_bytes), "s"(base), "i"(IMM) : "memory", "m0");
    else
        asm volatile("s_add_u32 m0, %0, %4\n\tglobal_load_lds_dwordx4 %1, %2 offset:%3" ::"s"(lds_base_bytes), "v"(off_bytes), "s"(base), "i"(IMM), "i"(LDS_ADD) : "memory", "m0", "scc");
}

// Barrier that orders LDS accesses only: this wave's ds_writes are complete (lgkmcnt(0)) while global -> LDS copies,
// global loads and global stores stay in flight.  __syncthreads() is a release fence over LDS, and a pending copy IS an
// LDS store: it waits vmcnt(0).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
