// Channel-generic NHWC convolutions of the optional layer2 stage (ResNet-18 children()[:-4]; models.py:49-51 keeps one
// stage less):
//   3x3 stride 2 pad 1, 64 -> 128   (block 0 conv1)
//   3x3 stride 1 pad 1, 128 -> 128  (block 0 conv2, block 1 conv1 / conv2)
//   1x1 stride 2 pad 0, 64 -> 128   (block 0 downsample)
// forward, data gradient and weight gradient of each, as implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact f32 products,
// one rounding per accumulation step: the error class of a plain f32 FMA loop).
//
// Forward and data gradient share one kernel.  An output pixel is gathered from a short list of taps, each a shifted
// window of a source map times a [Cs][N] slice of a K-major weight matrix.  The forward has one pixel class
// (output (y,x) reads source (s*y + ky - p, s*x + kx - p)); the stride-2 data gradient splits the input-gradient map
// into its four (y&1, x&1) parity classes, each of which reads only the taps whose stride phase matches -- no zero
// products -- and, when given a second source (the 1x1 downsample's output gradient), adds it as one more tap of class
// (0,0).  Classes without any tap (odd positions of a 1x1-only gradient) are written as zeros by the same launch.
//
// The weight gradient splits the pixel reduction into partial sums per block and folds them in a fixed order in a
// second launch (no float atomics: the step stays bit-reproducible).
//
// Every pixel / element offset is 64-bit (size_t): a 176-page batch at 1280^2 has 176*320*320*64 = 1.15e9 floats in
// layer1's output.
#include "common.h"

namespace {

constexpr int KC = 32;          // reduction chunk (channels of one tap; pixels in the weight gradient)
constexpr int MAXTAP = 10;      // nine 3x3 taps + one 1x1 tap
constexpr int NTHREADS = 256;   // four waves

struct Tap {
    int src;                    // 0 | 1: which source map / weight
    int dy, dx;                 // source offset added to (sm*jy, sm*jx)
    int wrow;                   // first row of the tap's [Cs][N] weight slice
};

struct Plan {
    int ncls;                   // pixel classes (1 forward, 4 stride-2 data gradient)
    int mul;                    // output pixel (y, x) = (mul*jy + oy, mul*jx + ox)
    int sm;                     // source pixel = (sm*jy + dy, sm*jx + dx)
    int oy[4], ox[4];
    int ntap[4];
    Tap tap[4][MAXTAP];
};

// out[b, y, x, n] = sum over the class's taps t, c < Cs of src_t[b, sm*jy + dy_t, sm*jx + dx_t, c] * w_t[wrow_t + c][n]
// (+ addend[b, y, x, n]).  Block tile BM pixels x BN outputs (BM * BN = 8192); each wave owns 32 pixels x 64 outputs
// in two 32x32 accumulators.  Global loads of the next chunk are issued before the MFMAs of the current one.
template <int BN>
__global__ void __launch_bounds__(NTHREADS) conv_nhwc_gather_kernel(
    const float *__restrict__ src0, const float *__restrict__ src1, const float *__restrict__ w0,
    const float *__restrict__ w1, const float *__restrict__ addend, float *__restrict__ out, Plan plan, int B,
    int Hs, int Ws, int Cs, int Ho, int Wo, int N)
{
    constexpr int BM = 8192 / BN;
    constexpr int A_PER = BM * KC / NTHREADS;    // floats per thread: 8 (BN=128) | 16 (BN=64)
    constexpr int B_PER = KC * BN / NTHREADS;    // 16 | 8
    constexpr int WM = BM / 32;                  // waves along pixels: 2 | 4
    __shared__ __align__(16) float As[BM][KC + 1];             // [pixel][channel]: lanes of an MFMA read 32 pixels of one channel
    __shared__ __align__(16) float Bs[KC][BN];                 // [channel][output]

    const int cls = blockIdx.z;
    const int Hc = (Ho - plan.oy[cls] + plan.mul - 1) / plan.mul;
    const int Wc = (Wo - plan.ox[cls] + plan.mul - 1) / plan.mul;
    const long long Mc = (long long)B * Hc * Wc;
    const long long m0 = (long long)blockIdx.x * BM;
    if (Hc <= 0 || Wc <= 0 || m0 >= Mc) return;
    const int n0 = blockIdx.y * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;

    // this thread's A rows: pixel ap (all A_PER channels of it are consecutive)
    constexpr int A_THR_PER_PIX = KC / A_PER;    // 4 | 2
    const int ap = tid / A_THR_PER_PIX, ac = (tid % A_THR_PER_PIX) * A_PER;
    const long long am = m0 + ap;
    const bool a_ok = am < Mc;
    int ab = 0, ajy = 0, ajx = 0;
    if (a_ok) {
        ab = (int)(am / ((long long)Hc * Wc));
        const int r = (int)(am - (long long)ab * Hc * Wc);
        ajy = r / Wc;
        ajx = r - ajy * Wc;
    }
    // this thread's B elements: row br, outputs bc .. bc + B_PER
    constexpr int B_THR_PER_ROW = BN / B_PER;
    const int br = tid / B_THR_PER_ROW, bc = (tid % B_THR_PER_ROW) * B_PER;

    const int ntap = plan.ntap[cls];
    const int chunks = Cs / KC;
    const int nsteps = ntap * chunks;
    f32x16 acc0 = {}, acc1 = {};
    float ra[A_PER], rb[B_PER];

    auto load = [&](int s) {
        const Tap t = plan.tap[cls][s / chunks];
        const int c0 = (s % chunks) * KC;
        const float *src = t.src ? src1 : src0;
        const float *w = t.src ? w1 : w0;
        const int sy = plan.sm * ajy + t.dy, sx = plan.sm * ajx + t.dx;
        if (a_ok && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) {
            const float4 *p = reinterpret_cast<const float4 *>(
                src + (((size_t)ab * Hs + sy) * Ws + sx) * Cs + c0 + ac);
#pragma unroll
            for (int i = 0; i < A_PER / 4; ++i) {
                const float4 v = p[i];
                ra[4 * i] = v.x; ra[4 * i + 1] = v.y; ra[4 * i + 2] = v.z; ra[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < A_PER; ++i) ra[i] = 0.f;
        }
        const float4 *q = reinterpret_cast<const float4 *>(w + (size_t)(t.wrow + c0 + br) * N + n0 + bc);
#pragma unroll
        for (int i = 0; i < B_PER / 4; ++i) {
            const float4 v = q[i];
            rb[4 * i] = v.x; rb[4 * i + 1] = v.y; rb[4 * i + 2] = v.z; rb[4 * i + 3] = v.w;
        }
    };

    if (nsteps > 0) load(0);
    for (int s = 0; s < nsteps; ++s) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) As[ap][ac + i] = ra[i];
#pragma unroll
        for (int i = 0; i < B_PER; i += 4)
            *reinterpret_cast<float4 *>(&Bs[br][bc + i]) = make_float4(rb[i], rb[i + 1], rb[i + 2], rb[i + 3]);
        __syncthreads();
        if (s + 1 < nsteps) load(s + 1);
        const int li = lane & 31, hi = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk) {
            const int k = 2 * kk + hi;
            const float a = As[wm * 32 + li][k];
            acc0 = mfma32(a, Bs[k][wn * 64 + li], acc0);
            acc1 = mfma32(a, Bs[k][wn * 64 + 32 + li], acc1);
        }
        __syncthreads();
    }

    // epilogue: D register r of lane l = pixel mfma32_row(r, l) of the wave's 32, output (l & 31) of each 32-block
    const int li = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long m = m0 + wm * 32 + mfma32_row(r, lane);
        if (m >= Mc) continue;
        const int b = (int)(m / ((long long)Hc * Wc));
        const int rr = (int)(m - (long long)b * Hc * Wc);
        const int jy = rr / Wc, jx = rr - jy * Wc;
        const int y = plan.mul * jy + plan.oy[cls], x = plan.mul * jx + plan.ox[cls];
        const size_t o = (((size_t)b * Ho + y) * Wo + x) * N + n0 + wn * 64 + li;
        float v0 = acc0[r], v1 = acc1[r];
        if (addend != nullptr) {
            v0 += addend[o];
            v1 += addend[o + 32];
        }
        out[o] = v0;
        out[o + 32] = v1;
    }
}

// w [Co][Ci][k][k] (OIHW) -> forward operand wf [(tap*Ci + ci)][Co] and data-gradient operand wd [(tap*Co + co)][Ci]
__global__ void conv_nhwc_prep_kernel(const float *__restrict__ w, float *__restrict__ wf, float *__restrict__ wd,
                                      int Co, int Ci, int kk)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Co * Ci * kk) return;
    const int tap = i % kk, ci = (i / kk) % Ci, co = i / (kk * Ci);
    const float v = w[i];
    if (wf != nullptr) wf[((size_t)tap * Ci + ci) * Co + co] = v;
    if (wd != nullptr) wd[((size_t)tap * Co + co) * Ci + ci] = v;
}

// Weight gradient, first stage: ws[part][(tap*Ci + ci)][co] = sum over the part's pixels m of
// x[b, s*oy + ky - p, s*ox + kx - p, ci] * dy[m][co].  Block tile 64 rows (one tap, 64 input channels) x 128 outputs;
// each wave owns 32 rows x 64 outputs.  Pixels come in chunks of 32 (the MFMA's k).
constexpr int WG_ROWS = 64, WG_COLS = 128;

__global__ void __launch_bounds__(NTHREADS) conv_nhwc_wgrad_partial_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ ws, int B, int H, int W, int Ci,
    int Ho, int Wo, int Co, int k, int stride, int pad, long long per_part)
{
    __shared__ __align__(16) float Xs[KC][WG_ROWS];            // [pixel][input channel]
    __shared__ __align__(16) float Ds[KC][WG_COLS];            // [pixel][output channel]
    const int rt = blockIdx.x;                   // row tile: tap rt / (Ci/64), channels (rt % (Ci/64)) * 64
    const int n0 = blockIdx.y * WG_COLS;
    const int part = blockIdx.z;
    const int tiles_per_tap = Ci / WG_ROWS;
    const int tap = rt / tiles_per_tap, ci0 = (rt % tiles_per_tap) * WG_ROWS;
    const int ky = tap / k, kx = tap % k;
    const long long M = (long long)B * Ho * Wo;
    const long long mbeg = (long long)part * per_part;
    const long long mend = mbeg + per_part < M ? mbeg + per_part : M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;

    // loads: X chunk 32 pixels x 64 channels (8 floats / thread), dy chunk 32 x 128 (16 floats / thread)
    const int xp = tid >> 3, xc = (tid & 7) * 8;
    const int dp = tid >> 3, dc = (tid & 7) * 16;
    float rx[8], rd[16];
    auto load = [&](long long mc) {
        const long long m = mc + xp;
        bool ok = m < mend;
        size_t xo = 0, dyo = 0;
        if (ok) {
            const int b = (int)(m / ((long long)Ho * Wo));
            const int r = (int)(m - (long long)b * Ho * Wo);
            const int oy = r / Wo, ox = r - oy * Wo;
            const int sy = stride * oy + ky - pad, sx = stride * ox + kx - pad;
            dyo = (size_t)m * Co + n0 + dc;
            ok = sy >= 0 && sy < H && sx >= 0 && sx < W;
            xo = (((size_t)b * H + (ok ? sy : 0)) * W + (ok ? sx : 0)) * Ci + ci0 + xc;
            const float4 *q = reinterpret_cast<const float4 *>(dy + dyo);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 v = q[i];
                rd[4 * i] = v.x; rd[4 * i + 1] = v.y; rd[4 * i + 2] = v.z; rd[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) rd[i] = 0.f;
        }
        if (ok) {
            const float4 *p = reinterpret_cast<const float4 *>(x + xo);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 v = p[i];
                rx[4 * i] = v.x; rx[4 * i + 1] = v.y; rx[4 * i + 2] = v.z; rx[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) rx[i] = 0.f;
        }
    };

    f32x16 acc0 = {}, acc1 = {};
    if (mbeg < mend) load(mbeg);
    for (long long mc = mbeg; mc < mend; mc += KC) {
#pragma unroll
        for (int i = 0; i < 8; i += 4)
            *reinterpret_cast<float4 *>(&Xs[xp][xc + i]) = make_float4(rx[i], rx[i + 1], rx[i + 2], rx[i + 3]);
#pragma unroll
        for (int i = 0; i < 16; i += 4)
            *reinterpret_cast<float4 *>(&Ds[dp][dc + i]) = make_float4(rd[i], rd[i + 1], rd[i + 2], rd[i + 3]);
        __syncthreads();
        if (mc + KC < mend) load(mc + KC);
        const int li = lane & 31, hi = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk) {
            const int kp = 2 * kk + hi;
            const float a = Xs[kp][wm * 32 + li];
            acc0 = mfma32(a, Ds[kp][wn * 64 + li], acc0);
            acc1 = mfma32(a, Ds[kp][wn * 64 + 32 + li], acc1);
        }
        __syncthreads();
    }
    // D register r of lane l = row mfma32_row(r, l) (input channel), column l & 31 (output channel)
    const int K = k * k * Ci;
    float *dst = ws + (size_t)part * K * Co;
    const int li = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = tap * Ci + ci0 + wm * 32 + mfma32_row(r, lane);
        const size_t o = (size_t)row * Co + n0 + wn * 64 + li;
        dst[o] = acc0[r];
        dst[o + 32] = acc1[r];
    }
}

// second stage: dw[co][ci][ky][kx] = sum over parts, in part order, of ws[part][(tap*Ci + ci)][co]
__global__ void conv_nhwc_wgrad_finish_kernel(const float *__restrict__ ws, float *__restrict__ dw, int nparts, int Ci,
                                              int Co, int kk)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int K = kk * Ci;
    if (i >= K * Co) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += ws[(size_t)p * K * Co + i];
    const int co = i % Co, row = i / Co;
    const int tap = row / Ci, ci = row % Ci;
    dw[((size_t)co * Ci + ci) * kk + tap] = s;
}

bool shape_ok(int Ci, int Co, int k, int stride, int pad)
{
    return Ci > 0 && Co > 0 && Ci % 64 == 0 && Co % 64 == 0 && (k == 1 || k == 3) && (stride == 1 || stride == 2) &&
           pad >= 0 && pad < k;
}

long long wgrad_per_part(long long M, int row_tiles, int col_tiles)
{
    // ~2048 blocks in all, at least 256 pixels per part; a multiple of the 32-pixel chunk
    long long parts = cdivll(2048, (long long)row_tiles * col_tiles);
    const long long cap = cdivll(M, 256);
    if (parts > cap) parts = cap;
    if (parts < 1) parts = 1;
    long long per = cdivll(M, parts);
    return cdivll(per, KC) * KC;
}

template <int BN>
int launch_gather(const float *src0, const float *src1, const float *w0, const float *w1, const float *addend,
                  float *out, const Plan &plan, int B, int Hs, int Ws, int Cs, int Ho, int Wo, int N,
                  hipStream_t stream)
{
    constexpr int BM = 8192 / BN;
    long long mmax = 0;
    for (int c = 0; c < plan.ncls; ++c) {
        const long long hc = (Ho - plan.oy[c] + plan.mul - 1) / plan.mul, wc = (Wo - plan.ox[c] + plan.mul - 1) / plan.mul;
        if (hc > 0 && wc > 0 && (long long)B * hc * wc > mmax) mmax = (long long)B * hc * wc;
    }
    if (mmax == 0) return COVA_OK;
    const long long gx = cdivll(mmax, BM);
    if (gx > 0x7fffffffLL) return COVA_ERR_BAD_ARG;
    COVA_LAUNCH(conv_nhwc_gather_kernel<BN>, dim3((unsigned)gx, N / BN, plan.ncls), dim3(NTHREADS), stream,
                src0, src1, w0, w1, addend, out, plan, B, Hs, Ws, Cs, Ho, Wo, N);
    return COVA_OK;
}

int gather(const float *src0, const float *src1, const float *w0, const float *w1, const float *addend, float *out,
           const Plan &plan, int B, int Hs, int Ws, int Cs, int Ho, int Wo, int N, hipStream_t stream)
{
    if (N % 128 == 0)
        return launch_gather<128>(src0, src1, w0, w1, addend, out, plan, B, Hs, Ws, Cs, Ho, Wo, N, stream);
    return launch_gather<64>(src0, src1, w0, w1, addend, out, plan, B, Hs, Ws, Cs, Ho, Wo, N, stream);
}

}  // namespace

COVA_API int cova_conv_nhwc_prep(const float *w_oihw, float *w_fwd, float *w_dgrad, int Co, int Ci, int k,
                                 void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    COVA_REQUIRE(w_oihw != nullptr && Co > 0 && Ci > 0 && k > 0);
    const int n = Co * Ci * k * k;
    COVA_LAUNCH(conv_nhwc_prep_kernel, dim3(cdiv(n, 256)), dim3(256), stream, w_oihw, w_fwd, w_dgrad, Co, Ci,
                k * k);
    return COVA_OK;
}

COVA_API int cova_conv_nhwc_fwd(const float *in, const float *w_fwd, float *out, int B, int H, int W, int Ci, int Co,
                                int k, int stride, int pad, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    COVA_REQUIRE(in != nullptr && w_fwd != nullptr && out != nullptr && B >= 0 && H > 0 && W > 0);
    COVA_REQUIRE(shape_ok(Ci, Co, k, stride, pad));
    // (integer division truncates towards zero: a map smaller than the kernel would pass as Ho = 1 at stride 2)
    COVA_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    COVA_REQUIRE(Ho > 0 && Wo > 0);
    if (B == 0) return COVA_OK;
    Plan plan = {};
    plan.ncls = 1;
    plan.mul = 1;
    plan.sm = stride;
    for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
            plan.tap[0][plan.ntap[0]++] = Tap{0, ky - pad, kx - pad, (ky * k + kx) * Ci};
    return gather(in, nullptr, w_fwd, nullptr, nullptr, out, plan, B, H, W, Ci, Ho, Wo, Co, stream);
}

COVA_API int cova_conv_nhwc_dgrad(const float *dy, const float *w_dgrad, const float *dy2, const float *w2_dgrad,
                                  const float *addend, float *dx, int B, int H, int W, int Ci, int Co, int k, int stride,
                                  int pad, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    COVA_REQUIRE(dy != nullptr && w_dgrad != nullptr && dx != nullptr && B >= 0 && H > 0 && W > 0);
    COVA_REQUIRE(shape_ok(Ci, Co, k, stride, pad));
    COVA_REQUIRE((dy2 == nullptr) == (w2_dgrad == nullptr));
    // (integer division truncates towards zero: a map smaller than the kernel would pass as Ho = 1 at stride 2)
    COVA_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    COVA_REQUIRE(Ho > 0 && Wo > 0);
    // the second source is a 1x1 pad-0 convolution of the same stride: same output grid
    COVA_REQUIRE(dy2 == nullptr || (W - 1) / stride + 1 == Wo);
    COVA_REQUIRE(dy2 == nullptr || (H - 1) / stride + 1 == Ho);
    if (B == 0) return COVA_OK;
    Plan plan = {};
    plan.ncls = stride * stride;
    plan.mul = stride;
    plan.sm = 1;
    for (int c = 0; c < plan.ncls; ++c) {
        const int py = c / stride, px = c % stride;
        plan.oy[c] = py;
        plan.ox[c] = px;
        // input (stride*jy + py) receives output oy = jy + (py + pad - ky) / stride when the division is exact
        for (int ky = 0; ky < k; ++ky) {
            const int ty = py + pad - ky;
            if (((ty % stride) + stride) % stride) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int tx = px + pad - kx;
                if (((tx % stride) + stride) % stride) continue;
                plan.tap[c][plan.ntap[c]++] = Tap{0, ty / stride, tx / stride, (ky * k + kx) * Co};
            }
        }
        if (dy2 != nullptr && py == 0 && px == 0) plan.tap[c][plan.ntap[c]++] = Tap{1, 0, 0, 0};
    }
    return gather(dy, dy2, w_dgrad, w2_dgrad, addend, dx, plan, B, Ho, Wo, Co, H, W, Ci, stream);
}

COVA_API int cova_conv_nhwc_wgrad_num_partials(int B, int Ho, int Wo, int Ci, int Co, int k)
{
    if (B <= 0 || Ho <= 0 || Wo <= 0 || Ci % 64 || Co % 128) return 1;
    const long long M = (long long)B * Ho * Wo;
    const long long per = wgrad_per_part(M, k * k * Ci / WG_ROWS, Co / WG_COLS);
    return (int)cdivll(M, per);
}

COVA_API int cova_conv_nhwc_wgrad_workspace_floats(int B, int Ho, int Wo, int Ci, int Co, int k)
{
    return cova_conv_nhwc_wgrad_num_partials(B, Ho, Wo, Ci, Co, k) * k * k * Ci * Co;
}

COVA_API int cova_conv_nhwc_wgrad(const float *in, const float *dy, float *dw /*OIHW*/, float *ws, int B, int H, int W,
                                  int Ci, int Co, int k, int stride, int pad, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    COVA_REQUIRE(in != nullptr && dy != nullptr && dw != nullptr && ws != nullptr && B >= 0 && H > 0 && W > 0);
    COVA_REQUIRE(shape_ok(Ci, Co, k, stride, pad) && Co % WG_COLS == 0);
    // (integer division truncates towards zero: a map smaller than the kernel would pass as Ho = 1 at stride 2)
    COVA_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    COVA_REQUIRE(Ho > 0 && Wo > 0);
    const int K = k * k * Ci;
    if (B == 0) {
        COVA_LAUNCH_CHECK();
        return (int)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)K * Co, stream);
    }
    const long long M = (long long)B * Ho * Wo;
    const int row_tiles = K / WG_ROWS, col_tiles = Co / WG_COLS;
    const long long per = wgrad_per_part(M, row_tiles, col_tiles);
    const int parts = (int)cdivll(M, per);
    COVA_LAUNCH(conv_nhwc_wgrad_partial_kernel, dim3(row_tiles, col_tiles, parts), dim3(NTHREADS), stream,
                in, dy, ws, B, H, W, Ci, Ho, Wo, Co, k, stride, pad, per);
    COVA_LAUNCH(conv_nhwc_wgrad_finish_kernel, dim3(cdiv(K * Co, 256)), dim3(256), stream, ws, dw, parts, Ci,
                Co, k * k);
    return COVA_OK;
}
