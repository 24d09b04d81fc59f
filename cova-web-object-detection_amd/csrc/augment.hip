// Page augmentation inside the page gather (include/cova_hip.h, cova_pages_u8_augment_f32 / cova_boxes_translate): the launch
// that reads every uint8 pixel of a step's pages and writes every float32 pixel also shifts the viewport by a per-page integer
// (dx, dy) with a constant fill colour and applies a per-page 3x4 affine colour transform.  The same bytes move as in the plain
// gather (3 in, 12 out per pixel); the parameters are a function of (seed, epoch, page id) computed on the host
// (pipeline.PageAugment) and uploaded once per epoch.  The reference augments nothing: this is an opt-in extension.
#include "common.h"

namespace {

// out = clamp(((m0*t0 + m1*t1) + m2*t2) + m3, 0, 1) of channel row m; every multiply and add rounded on its own (the numpy
// statement is tests/augment_oracle.py); never -0, NaN -> 0.
__device__ __forceinline__ float color_row(const float *m, float t0, float t1, float t2)
{
#pragma clang fp contract(off)
    const float y = ((m[0] * t0 + m[1] * t1) + m[2] * t2) + m[3];
    return y > 0.f ? fminf(y, 1.f) : 0.f;
}

// (float)v / 255.f of a byte, correctly rounded, in three operations instead of the division's ten: the product with the
// rounded reciprocal and one Newton step on the exact residual.  Equal to the IEEE quotient for every v in 0..255 (checked
// exhaustively in exact arithmetic by tests/test_augment_cpu.py, and against the division on the device).
__device__ __forceinline__ float byte_unit(uint32_t v)
{
    const float c = 1.f / 255.f, f = (float)v;
    const float q = f * c;
    return fmaf(fmaf(-255.f, q, f), c, q);
}

// What output page b needs, the same for every thread of the block (b comes from blockIdx.y): false = skip the page.
__device__ __forceinline__ bool page_params(const int *__restrict__ page_idx, int P, const int *__restrict__ shift,
                                            const float *__restrict__ color, int b, long long &sp, int &dx, int &dy, float *m)
{
    sp = page_idx ? (long long)page_idx[b] : (long long)b;
    if (sp < 0 || sp >= P) return false;
    dx = shift ? shift[2 * b] : 0;
    dy = shift ? shift[2 * b + 1] : 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = color ? color[12 * (long long)b + k] : ((k % 5) == 0 ? 1.f : 0.f);
    return true;
}

// 4 consecutive pixels of one output row per thread, one float4 store per channel plane.  W % 4 == 0, src 4-byte and dst
// 16-byte aligned, so every page starts on a dword and the store ends on one.  The 12 source bytes start at byte
// (sy*W + sx0)*3 of the page, any residue r modulo 4: the 3 (r == 0) or 4 aligned dwords that cover them are loaded (one
// dwordx3 load, and one dword load at offset 12 predicated on r != 0) and realigned with v_alignbyte_b32.  The fourth dword is read only when r != 0; it then holds a byte
// of the group's last pixel and so lies inside the store (whose size is a multiple of 4).  A group that straddles the left /
// right edge reads byte by byte, a group wholly outside reads nothing.
// Block = 64 x 4 threads: a wave walks one output row in steps of 64 groups (768 contiguous source bytes), the four waves
// take four rows, blockIdx.x strides over the rows and blockIdx.y over the pages -- no division, and the row test (sy inside
// the page) is the same for a whole wave.
__global__ __launch_bounds__(256) void augment_vec4_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int P,
                                                           int B, int H, int W, const int *__restrict__ page_idx,
                                                           const int *__restrict__ shift, const float *__restrict__ color,
                                                           uint32_t fill)
{
    const long long plane = (long long)H * W;
    const int W4 = W / 4;
    const uint32_t fb[3] = {(fill >> 16) & 255, (fill >> 8) & 255, fill & 255};
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        long long sp;
        int dx, dy;
        float m[12];
        if (!page_params(page_idx, P, shift, color, b, sp, dx, dy, m)) continue;
        const uint8_t *page = src + sp * plane * 3;                  // 64-bit: a store may exceed 4 GiB
        float *out = dst + (long long)b * 3 * plane;
        for (long long y = (long long)blockIdx.x * 4 + threadIdx.y; y < H; y += (long long)gridDim.x * 4) {
            const long long sy = y - dy;                             // 64-bit: any int32 shift
            const bool row_in = sy >= 0 && sy < H;
            const long long row = row_in ? sy * W * 3 : 0;           // byte offset of the source row in the page
            for (int g = threadIdx.x; g < W4; g += 64) {
                const long long sx0 = 4ll * g - dx;
                uint32_t v[12];
                if (row_in && sx0 >= 0 && sx0 + 3 < W) {
                    const long long off = row + sx0 * 3;
                    const uint32_t *a = reinterpret_cast<const uint32_t *>(page + (off & ~3ll));
                    const uint32_t r = (uint32_t)(off & 3);
                    uint32_t d0, d1, d2, d3 = 0u;
                    if (r) {
                        d0 = a[0], d1 = a[1], d2 = a[2], d3 = a[3];
                    } else {
                        d0 = a[0], d1 = a[1], d2 = a[2];
                    }
                    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, r), w1 = __builtin_amdgcn_alignbyte(d2, d1, r),
                                   w2 = __builtin_amdgcn_alignbyte(d3, d2, r);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] = (w0 >> (8 * k)) & 255;
                        v[4 + k] = (w1 >> (8 * k)) & 255;
                        v[8 + k] = (w2 >> (8 * k)) & 255;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const long long sx = sx0 + k;
                        const bool in = row_in && sx >= 0 && sx < W;
                        const long long o = in ? row + sx * 3 : 0;
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[3 * k + c] = in ? (uint32_t)page[o + c] : fb[c];
                    }
                }
                float t[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) t[k] = byte_unit(v[k]);
                float *d = out + y * W + 4 * g;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    *reinterpret_cast<float4 *>(d + c * plane) =
                        make_float4(color_row(m + 4 * c, t[0], t[1], t[2]), color_row(m + 4 * c, t[3], t[4], t[5]),
                                    color_row(m + 4 * c, t[6], t[7], t[8]), color_row(m + 4 * c, t[9], t[10], t[11]));
            }
        }
    }
}

// one pixel per thread: any W, any alignment, the same bytes out
__global__ __launch_bounds__(256) void augment_scalar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int P,
                                                             int B, int H, int W, const int *__restrict__ page_idx,
                                                             const int *__restrict__ shift, const float *__restrict__ color,
                                                             uint32_t fill)
{
    const long long plane = (long long)H * W;
    const uint32_t fb[3] = {(fill >> 16) & 255, (fill >> 8) & 255, fill & 255};
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        long long sp;
        int dx, dy;
        float m[12];
        if (!page_params(page_idx, P, shift, color, b, sp, dx, dy, m)) continue;
        const uint8_t *page = src + sp * plane * 3;
        float *out = dst + (long long)b * 3 * plane;
        for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < plane;
             q += (long long)gridDim.x * blockDim.x) {
            const long long y = q / W, x = q - y * W;
            const long long sy = y - dy, sx = x - dx;
            const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
            const long long o = in ? (sy * W + sx) * 3 : 0;
            float t[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = byte_unit(in ? (uint32_t)page[o + c] : fb[c]);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * plane + q] = color_row(m + 4 * c, t[0], t[1], t[2]);
        }
    }
}

// one thread per box: the page column selects the shift
__global__ __launch_bounds__(256) void boxes_translate_kernel(float *__restrict__ bboxes, int N,
                                                              const int *__restrict__ shift, int B)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    float *r = bboxes + (long long)g * 5;
    const float pf = r[0];
    if (!(pf > -1.f && pf < 2147483648.f)) return;                   // (int)pf is defined and >= 0 exactly here; NaN fails
    const int p = (int)pf;
    if (p >= B) return;
    const float fx = (float)shift[2 * p], fy = (float)shift[2 * p + 1];
    r[1] += fx;
    r[2] += fy;
    r[3] += fx;
    r[4] += fy;
}

}  // namespace

COVA_API int cova_pages_u8_augment_f32(const uint8_t *store_u8, const int *page_idx, int P, int B, int H, int W,
                                       const int *shift, const float *color, int fill_rgb, float *f32_nchw, void *stream)
{
    COVA_REQUIRE(store_u8 && f32_nchw && P > 0 && B >= 0 && H > 0 && W > 0);
    COVA_REQUIRE(page_idx || P >= B);
    if (B == 0) return COVA_OK;
    const long long plane = (long long)H * W;
    const bool vec = W % 4 == 0 && ((uintptr_t)store_u8 & 3) == 0 && ((uintptr_t)f32_nchw & 15) == 0;
    const long long work = vec ? ((long long)H + 3) / 4 : (plane + 255) / 256;       // blocks that cover a page once
    const int gy = B < 65535 ? B : 65535;
    const long long cap = 8192 / gy > 0 ? 8192 / gy : 1;             // as many blocks as the plain gather launches
    const long long gx = work < cap ? work : cap;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(augment_vec4_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(64, 4), 0, st, store_u8, f32_nchw, P, B,
                           H, W, page_idx, shift, color, (uint32_t)fill_rgb);
    else
        hipLaunchKernelGGL(augment_scalar_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, store_u8, f32_nchw, P,
                           B, H, W, page_idx, shift, color, (uint32_t)fill_rgb);
    COVA_LAUNCH_CHECK();
    return COVA_OK;
}

COVA_API int cova_boxes_translate(float *bboxes, int N, const int *shift, int B, void *stream)
{
    COVA_REQUIRE(N >= 0 && B >= 0);
    if (N == 0) return COVA_OK;
    COVA_REQUIRE(bboxes && shift && B > 0);
    hipLaunchKernelGGL(boxes_translate_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, bboxes, N,
                       shift, B);
    COVA_LAUNCH_CHECK();
    return COVA_OK;
}
