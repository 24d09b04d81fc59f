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

// ---------------------------------------------------------------------------------------------------------------- page zoom
// cova_pages_u8_resample_f32 (include/cova_hip.h): the gather as a bilinear resample in 16.16 fixed point with 8-bit weights.
// Everything up to the quotient is integer arithmetic: q = sum over the four taps of wy*wx*byte <= 255*65536 < 2^24.

constexpr float RS_DEN = 16711680.f;                     // 255 * 65536
constexpr int RS_MAX_FAST_INV = 131072;                  // the staged form serves steps of at most two source pixels
constexpr int RS_CAP = 516;                              // source pixels of a row that 256 output pixels can touch at that step
constexpr int RS_PAD = 8;                                // bytes in front of a staged segment: two fill pixels and a dword start
constexpr int RS_ROW_DW = 396;                           // RS_PAD + 3 (residue) + RS_CAP*3 bytes + the 12 a lane reads from its tap on

// (float)q / 16711680.f, correctly rounded, as byte_unit: checked against the exact quotient for every q in 0..16711680 by
// tests/test_resample_cpu.py.
__device__ __forceinline__ float tap_unit(uint32_t q)
{
    const float c = 1.f / RS_DEN, f = (float)q;
    const float t = f * c;
    return fmaf(fmaf(-RS_DEN, t, f), c, t);
}

__device__ __forceinline__ uint32_t tap_sum(uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11, uint32_t fx, uint32_t fy)
{
    return (256u - fy) * ((256u - fx) * a00 + fx * a01) + fy * ((256u - fx) * a10 + fx * a11);
}

__device__ __forceinline__ bool resample_page_params(const int *__restrict__ page_idx, int P, const int *__restrict__ step,
                                                     const long long *__restrict__ origin, const float *__restrict__ color,
                                                     int b, long long &sp, int &ivx, int &ivy, long long &ox, long long &oy,
                                                     float *m)
{
    sp = page_idx ? (long long)page_idx[b] : (long long)b;
    if (sp < 0 || sp >= P) return false;
    ivx = step[2 * b], ivy = step[2 * b + 1];
    ox = origin[2 * b], oy = origin[2 * b + 1];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = color ? color[12 * (long long)b + k] : ((k % 5) == 0 ? 1.f : 0.f);
    return true;
}

// The two horizontal taps of one pixel out of a staged row: their 6 bytes start at byte ``at`` of the row, at any residue, so
// the three dwords that cover them are read (aligned, two LDS instructions) and realigned as the shift kernel realigns its
// global dwords.  h[c] = (256 - fx)*tap0[c] + fx*tap1[c].
__device__ __forceinline__ void staged_taps(const uint32_t *row, int at, uint32_t fx, uint32_t *h)
{
    const uint32_t *w = row + (at >> 2);
    const uint32_t sh = (uint32_t)at & 3u;
    const uint32_t d0 = w[0], d1 = w[1], d2 = w[2];
    const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, sh), hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
    const uint32_t a[6] = {lo & 255u, (lo >> 8) & 255u, (lo >> 16) & 255u, lo >> 24, hi & 255u, (hi >> 8) & 255u};
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = (256u - fx) * a[c] + fx * a[3 + c];
}

// the four taps of one output pixel straight from the store, every tap tested against the page: any step, any origin
__device__ __forceinline__ void resample_pixel_global(const uint8_t *__restrict__ page, int H, int W, long long px,
                                                      long long iy, uint32_t fy, const uint32_t *fb, uint32_t *q)
{
    const long long ix = px >> 16;
    const uint32_t fx = (uint32_t)(px >> 8) & 255u;
    uint32_t a[2][2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const long long ty = iy + r, tx = ix + s;
            const bool in = ty >= 0 && ty < H && tx >= 0 && tx < W;
            const long long o = in ? (ty * W + tx) * 3 : 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) a[r][s][c] = in ? (uint32_t)page[o + c] : fb[c];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = tap_sum(a[0][0][c], a[0][1][c], a[1][0][c], a[1][1][c], fx, fy);
}

// The launch geometry of augment_vec4_kernel: 4 consecutive pixels of one output row per thread, one float4 store per plane,
// a wave walks its row in trips of 64 groups, the four waves of a block take four rows.  W % 4 == 0, src 4-byte and dst
// 16-byte aligned.  p_y, and with it the row pair, its weights and the rows' inside tests, is the same for a whole wave.
// With inv_x <= 131072 the 256 output pixels of a trip touch at most RS_CAP consecutive source pixels of a row: the wave
// copies that segment of both rows (clipped to the page, widened to whole dwords -- rows start on a dword, so the widened
// segment stays inside its row) into its own LDS rows with coalesced dword loads, and every lane reads its taps from there
// as bytes.  Pixel j of the n staged ones lies at byte RS_PAD + r + 3*j (r = the segment's byte residue, the same for both
// rows).  Behind the copy twelve lanes write the fill colour as pixels -2, -1 and n, n+1; a lane's first tap is clamped to
// [-2, n], so a tap left or right of the page reads the fill colour and no tap is tested on its own.  (A segment clipped
// inside the page ends where the wave's taps end: the pads next to it are never read.)  A row outside the page
// contributes 256 * fill without a read, a second row of weight 0 is neither staged nor read; both are branches on
// scalars.  Behind the window's 64-bit origin a pixel's position is 32-bit arithmetic.  A page with a larger (or
// non-positive) inv_x reads its taps from the store one by one, each tested against the page.
__global__ __launch_bounds__(256) void resample_vec4_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int P,
                                                            int B, int H, int W, const int *__restrict__ page_idx,
                                                            const int *__restrict__ step,
                                                            const long long *__restrict__ origin,
                                                            const float *__restrict__ color, uint32_t fill)
{
    __shared__ uint32_t seg[4][2][RS_ROW_DW];
    const long long plane = (long long)H * W;
    const int W4 = W / 4, lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);   // 64 x 4 threads: a scalar, and so is all that hangs on the row
    const uint32_t fb[3] = {(fill >> 16) & 255, (fill >> 8) & 255, fill & 255};
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        long long sp, ox, oy;
        int ivx, ivy;
        float m[12];
        if (!resample_page_params(page_idx, P, step, origin, color, b, sp, ivx, ivy, ox, oy, m)) continue;
        const uint8_t *page = src + sp * plane * 3;                  // 64-bit: a store may exceed 4 GiB
        float *out = dst + (long long)b * 3 * plane;
        const bool staged = ivx >= 1 && ivx <= RS_MAX_FAST_INV;
        for (long long y0 = (long long)blockIdx.x * 4; y0 < H; y0 += (long long)gridDim.x * 4) {   // the same trips for the block
            const long long y = y0 + wave;
            const bool row_live = y < H;
            const long long py = oy + y * ivy, iy = py >> 16;
            const uint32_t fy = (uint32_t)(py >> 8) & 255u;
            const bool in_r0 = iy >= 0 && iy < H, in_r1 = iy >= -1 && iy < H - 1;
            for (int g0 = 0; g0 < W4; g0 += 64) {
                const int g = g0 + lane;
                uint32_t q[12];
                if (staged) {
                    // the trip's source window, the same for the whole wave: 64-bit once, 32-bit per pixel behind it
                    const int x_first = 4 * g0, x_last = min(x_first + 255, W - 1);
                    const long long p_first = ox + (long long)x_first * ivx;
                    const long long ix_lo = p_first >> 16;
                    const long long ix_hi = ((p_first + (long long)(x_last - x_first) * ivx) >> 16) + 1;
                    const long long lo = ix_lo > 0 ? ix_lo : 0, hi = ix_hi < W - 1 ? ix_hi : W - 1;
                    const long long n64 = hi - lo + 1;               // source pixels of the segment inside the page
                    const int n = n64 < 0 ? 0 : (n64 > RS_CAP ? RS_CAP : (int)n64);   // <= 512 by the step bound: no cap bites
                    const uint32_t r = (uint32_t)(lo * 3) & 3u;
                    const int left = ix_lo < -(1 << 20) ? -(1 << 20) : (ix_lo < 0 ? (int)ix_lo : 0);   // ix_lo - lo, held in 32 bits
                    if (row_live) {
#pragma unroll
                        for (int s = 0; s < 2; ++s) {
                            if (s == 0 ? !in_r0 : !(in_r1 && fy != 0)) continue;
                            if (n > 0) {
                                const int ndw = (int)((r + n * 3 + 3) >> 2);
                                const uint32_t *a =
                                    reinterpret_cast<const uint32_t *>(page + ((iy + s) * W + lo) * 3 - r);
                                for (int d = lane; d < ndw; d += 64) seg[wave][s][RS_PAD / 4 + d] = a[d];
                            }
                            if (lane < 12) {                         // behind the copy: the fill pixels -2, -1 and n, n+1
                                const int c = lane % 3;
                                reinterpret_cast<uint8_t *>(seg[wave][s])[RS_PAD + r + (lane < 6 ? lane - 6 : 3 * n + lane - 6)] =
                                    (uint8_t)(c == 0 ? fb[0] : (c == 1 ? fb[1] : fb[2]));
                            }
                        }
                    }
                    __syncthreads();
                    if (row_live && g < W4) {
                        const uint32_t u0 = ((uint32_t)p_first & 0xFFFFu) + (uint32_t)(4 * lane) * (uint32_t)ivx;   // < 2^16 + 2^25
                        int j[4];
                        uint32_t fx[4], top[12], bot[12];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t u = u0 + (uint32_t)k * (uint32_t)ivx;     // p_x - (ix_lo << 16)
                            fx[k] = (u >> 8) & 255u;
                            const int jj = (int)(u >> 16) + left;                    // i_x - lo, or far enough left of it
                            j[k] = RS_PAD + (int)r + 3 * max(-2, min(jj, n));        // the byte of the first tap in the row
                        }
                        if (in_r0) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) staged_taps(seg[wave][0], j[k], fx[k], top + 3 * k);
                        } else {
#pragma unroll
                            for (int k = 0; k < 12; ++k) top[k] = 256u * fb[k % 3];
                        }
                        if (fy == 0) {                               // the second row weighs nothing: q = 256 * top
#pragma unroll
                            for (int k = 0; k < 12; ++k) q[k] = top[k] << 8;
                        } else {
                            if (in_r1) {
#pragma unroll
                                for (int k = 0; k < 4; ++k) staged_taps(seg[wave][1], j[k], fx[k], bot + 3 * k);
                            } else {
#pragma unroll
                                for (int k = 0; k < 12; ++k) bot[k] = 256u * fb[k % 3];
                            }
#pragma unroll
                            for (int k = 0; k < 12; ++k) q[k] = (256u - fy) * top[k] + fy * bot[k];
                        }
                    }
                    __syncthreads();                                 // the next trip writes the rows this one read
                } else if (row_live && g < W4) {                     // rare: small code, a pixel at a time, the same bytes
#pragma unroll 1
                    for (int k = 0; k < 4; ++k) {
                        uint32_t q1[3];
                        resample_pixel_global(page, H, W, ox + (long long)(4 * g + k) * ivx, iy, fy, fb, q1);
                        const float t0 = tap_unit(q1[0]), t1 = tap_unit(q1[1]), t2 = tap_unit(q1[2]);
                        float *d = out + y * W + 4 * g + k;
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[c * plane] = color_row(m + 4 * c, t0, t1, t2);
                    }
                }
                if (staged && row_live && g < W4) {
                    float t[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) t[k] = tap_unit(q[k]);
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
}

// one pixel per thread: any W, any alignment, any step, the same bytes out
__global__ __launch_bounds__(256) void resample_scalar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int P,
                                                              int B, int H, int W, const int *__restrict__ page_idx,
                                                              const int *__restrict__ step,
                                                              const long long *__restrict__ origin,
                                                              const float *__restrict__ color, uint32_t fill)
{
    const long long plane = (long long)H * W;
    const uint32_t fb[3] = {(fill >> 16) & 255, (fill >> 8) & 255, fill & 255};
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        long long sp, ox, oy;
        int ivx, ivy;
        float m[12];
        if (!resample_page_params(page_idx, P, step, origin, color, b, sp, ivx, ivy, ox, oy, m)) continue;
        const uint8_t *page = src + sp * plane * 3;
        float *out = dst + (long long)b * 3 * plane;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < plane;
             i += (long long)gridDim.x * blockDim.x) {
            const long long y = i / W, x = i - y * W;
            const long long py = oy + y * ivy;
            uint32_t q[3];
            resample_pixel_global(page, H, W, ox + x * ivx, py >> 16, (uint32_t)(py >> 8) & 255u, fb, q);
            const float t0 = tap_unit(q[0]), t1 = tap_unit(q[1]), t2 = tap_unit(q[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * plane + i] = color_row(m + 4 * c, t0, t1, t2);
        }
    }
}

// one thread per box: the page column selects the map; one multiply, then one add, each rounded on its own
__global__ __launch_bounds__(256) void boxes_affine_kernel(float *__restrict__ bboxes, int N, const float *__restrict__ affine,
                                                           int B)
{
#pragma clang fp contract(off)
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    float *r = bboxes + (long long)g * 5;
    const float pf = r[0];
    if (!(pf > -1.f && pf < 2147483648.f)) return;                   // as boxes_translate_kernel
    const int p = (int)pf;
    if (p >= B) return;
    const float sx = affine[4 * p], sy = affine[4 * p + 1], tx = affine[4 * p + 2], ty = affine[4 * p + 3];
    r[1] = r[1] * sx + tx;
    r[2] = r[2] * sy + ty;
    r[3] = r[3] * sx + tx;
    r[4] = r[4] * sy + ty;
}

}  // namespace

COVA_API int cova_pages_u8_resample_f32(const uint8_t *store_u8, const int *page_idx, int P, int B, int H, int W,
                                        const int *step, const long long *origin, const float *color, int fill_rgb,
                                        float *f32_nchw, void *stream)
{
    COVA_REQUIRE(store_u8 && f32_nchw && P > 0 && B >= 0 && H > 0 && W > 0);
    COVA_REQUIRE(page_idx || P >= B);
    if (B == 0) return COVA_OK;
    COVA_REQUIRE(step && origin);
    const long long plane = (long long)H * W;
    const bool vec = W % 4 == 0 && ((uintptr_t)store_u8 & 3) == 0 && ((uintptr_t)f32_nchw & 15) == 0;
    const long long work = vec ? ((long long)H + 3) / 4 : (plane + 255) / 256;       // blocks that cover a page once
    const int gy = B < 65535 ? B : 65535;
    const long long cap = 8192 / gy > 0 ? 8192 / gy : 1;             // the grid of cova_pages_u8_augment_f32
    const long long gx = work < cap ? work : cap;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        COVA_LAUNCH(resample_vec4_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(64, 4), st, store_u8, f32_nchw, P,
                    B, H, W, page_idx, step, origin, color, (uint32_t)fill_rgb);
    else
        COVA_LAUNCH(resample_scalar_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), st, store_u8, f32_nchw, P,
                    B, H, W, page_idx, step, origin, color, (uint32_t)fill_rgb);
    return COVA_OK;
}

COVA_API int cova_boxes_affine(float *bboxes, int N, const float *affine, int B, void *stream)
{
    COVA_REQUIRE(N >= 0 && B >= 0);
    if (N == 0) return COVA_OK;
    COVA_REQUIRE(bboxes && affine && B > 0);
    COVA_LAUNCH(boxes_affine_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), (hipStream_t)stream, bboxes, N,
                affine, B);
    return COVA_OK;
}

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
        COVA_LAUNCH(augment_vec4_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(64, 4), st, store_u8, f32_nchw, P, B,
                    H, W, page_idx, shift, color, (uint32_t)fill_rgb);
    else
        COVA_LAUNCH(augment_scalar_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), st, store_u8, f32_nchw, P,
                    B, H, W, page_idx, shift, color, (uint32_t)fill_rgb);
    return COVA_OK;
}

COVA_API int cova_boxes_translate(float *bboxes, int N, const int *shift, int B, void *stream)
{
    COVA_REQUIRE(N >= 0 && B >= 0);
    if (N == 0) return COVA_OK;
    COVA_REQUIRE(bboxes && shift && B > 0);
    COVA_LAUNCH(boxes_translate_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), (hipStream_t)stream, bboxes, N,
                shift, B);
    return COVA_OK;
}
