// Row kernels of the page encoder: LayerNorm forward / backward and the exact (erf) GELU forward /
// backward around the page attention and the GEMMs of a pre-LN transformer block.
//
// LayerNorm: one wave per row, a block's LN_WAVES waves stride over rows; lanes sit over channels (float4 chunks lane,
// lane + 64 when C % 4 == 0 and every base and leading dimension is 16-byte aligned, scalar channels lane, lane + 64, ...
// otherwise).  The row stays in registers (two float4 or eight floats per lane, C <= 512); the forward uses no LDS, the
// backward only for the combine of its waves.
//   mean          a lane's channels ascending (plain adds from +0), the xor butterfly (offsets 32, 16, .., 1), / C
//   rstd          d = x - mean per channel, a lane's d*d ascending as one fma chain from +0, the butterfly, / C, + eps,
//                 1 / sqrt: the variance in two passes over the registers, never E[x^2] - mean^2
//   out           fma((x - mean) * rstd, weight, bias)
// Backward, with xhat = (x - mean) * rstd re-formed from the saved mean and rstd by the forward's operations, gw = g * weight:
//   m1 = sum_c gw / C, m2 = sum_c gw * xhat / C    (lane ascending, adds for m1, an fma chain for m2, the butterfly)
//   dx = (res ? res : 0) + rstd * ((gw - m1) - xhat * m2)
//   dweight, dbias   block b owns the rows [b * LN_BWD_ROWS, (b + 1) * LN_BWD_ROWS), LN_BWD_ROWS = 32; wave w adds the rows
//                 b * 32 + w, + 4, ... ascending per channel (fma(g, xhat, .) and plain adds), the waves combine in wave
//                 order through LDS into ws [blocks][2][C]; layernorm_fold_kernel sums the blocks ascending.
// Every order is a function of (R, C) alone and a row's out, mean, rstd and dx are formed by its own wave from its own
// values: reruns are bit-identical and a row keeps its bits whatever rows surround it.
//
// GELU: elementwise, out = 0.5 z (1 + erff(z / sqrt 2)), dz = g (0.5 (1 + erff(z / sqrt 2)) + z expf(-z^2 / 2) / sqrt(2 pi));
// float4 chunks under the same alignment rule, grid-stride.
//
// Dropout of the encoder's sites 1 to 3: torch's inverted dropout, rate p, inv = 1.f / (1.f - p), stream
// seed.  Element (r, c) of an [R, C] operand is kept when hash_uniform(seed, r * C + c) >= p (f32 compare; the convention of
// dropout_fwd_kernel); no mask is stored, the backward regenerates it from the same (seed, r * C + c).
//   cova_gelu_fwd_drop       f  = keep ? gelu(z) * inv : 0        the DROP flag of the GELU forward; z stays the saved tensor
//   cova_gelu_bwd_drop       dz = keep ? (g * inv) * gelu'(z) : 0 the DROP flag of the GELU backward
//   cova_dropout_add_fwd     out = x + (keep ? y * inv : 0)       two roundings: the scaled value, then the residual add
//   cova_dropout_regen_bwd   dy = keep ? g * inv : 0
// Every `* inv` is one rounded multiply (__fmul_rn).  Same access rule and grid-stride launch as the GELU kernels.
#include "rows.h"

// the orders above count one rounding per written operation: only the fmaf calls fuse
#pragma clang fp contract(off)

namespace {

constexpr int LN_MAX_C = 512;
constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int LN_BWD_ROWS = 32;           // rows of one backward block (a wave adds eight of them)
constexpr int LN_FWD_MAX_BLOCKS = 2048;

template <int V>
__global__ __launch_bounds__(LN_THREADS) void layernorm_fwd_kernel(
    const float *__restrict__ x, int ldx, int R, int C, const float *__restrict__ weight, const float *__restrict__ bias,
    float eps, float *__restrict__ out, int ldo, float *__restrict__ mean, float *__restrict__ rstd)
{
    constexpr int NCH = LN_MAX_C / (64 * V);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float w[NCH][V], b[NCH][V];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) w[k][v] = b[k][v] = 0.f;
        if (c < C) {
            ro_load<V>(weight + c, w[k]);
            ro_load<V>(bias + c, b[k]);
        }
    }
    const float fC = (float)C;
    for (long long r = (long long)blockIdx.x * LN_WAVES + wave; r < R; r += (long long)gridDim.x * LN_WAVES) {
        const float *row = x + (size_t)r * ldx;
        float d[NCH][V];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
#pragma unroll
            for (int v = 0; v < V; ++v) d[k][v] = 0.f;
            if (c < C) {
                ro_load<V>(row + c, d[k]);
#pragma unroll
                for (int v = 0; v < V; ++v) s += d[k][v];
            }
        }
        const float mu = wave_sum(s) / fC;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < C) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    d[k][v] = d[k][v] - mu;
                    q = fmaf(d[k][v], d[k][v], q);
                }
            }
        }
        const float rs = 1.f / sqrtf(wave_sum(q) / fC + eps);
        float *orow = out + (size_t)r * ldo;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < C) {
                float o[V];
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = fmaf(d[k][v] * rs, w[k][v], b[k][v]);
                ro_store<V>(orow + c, o);
            }
        }
        if (lane == 0) {
            mean[r] = mu;
            rstd[r] = rs;
        }
    }
}

// res and dx may be the same buffer (the residual stream's gradient, updated in place): every element is read and written
// by the one lane that owns it.
template <int V>
__global__ __launch_bounds__(LN_THREADS) void layernorm_bwd_kernel(
    const float *__restrict__ g, int ldg, const float *__restrict__ x, int ldx, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ weight, int R, int C, const float *res, int ldr, float *dx,
    int lddx, float *__restrict__ ws)
{
    constexpr int NCH = LN_MAX_C / (64 * V);
    __shared__ __attribute__((aligned(16))) float part[LN_WAVES][2][LN_MAX_C];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long r0 = (long long)blockIdx.x * LN_BWD_ROWS;          // (64-bit: r0 + 32 and r + 4 stay in range for any R)
    const long long r1 = r0 + LN_BWD_ROWS < R ? r0 + LN_BWD_ROWS : R;
    float w[NCH][V], dw[NCH][V], db[NCH][V];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) w[k][v] = dw[k][v] = db[k][v] = 0.f;
        if (c < C) ro_load<V>(weight + c, w[k]);
    }
    const float fC = (float)C;
    for (long long r = r0 + wave; r < r1; r += LN_WAVES) {
        const float mu = mean[r], rs = rstd[r];
        const float *grow = g + (size_t)r * ldg, *xrow = x + (size_t)r * ldx;
        float xh[NCH][V], gw[NCH][V];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
#pragma unroll
            for (int v = 0; v < V; ++v) xh[k][v] = gw[k][v] = 0.f;
            if (c < C) {
                float gv[V];
                ro_load<V>(grow + c, gv);
                ro_load<V>(xrow + c, xh[k]);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    xh[k][v] = (xh[k][v] - mu) * rs;
                    gw[k][v] = gv[v] * w[k][v];
                    s1 += gw[k][v];
                    s2 = fmaf(gw[k][v], xh[k][v], s2);
                    dw[k][v] = fmaf(gv[v], xh[k][v], dw[k][v]);
                    db[k][v] += gv[v];
                }
            }
        }
        const float m1 = wave_sum(s1) / fC, m2 = wave_sum(s2) / fC;
        float *drow = dx + (size_t)r * lddx;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < C) {
                float o[V];
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = rs * ((gw[k][v] - m1) - xh[k][v] * m2);
                if (res) {
                    float rv[V];
                    ro_load<V>(res + (size_t)r * ldr + c, rv);
#pragma unroll
                    for (int v = 0; v < V; ++v) o[v] = rv[v] + o[v];
                }
                ro_store<V>(drow + c, o);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < C) {
            ro_store<V>(&part[wave][0][c], dw[k]);
            ro_store<V>(&part[wave][1][c], db[k]);
        }
    }
    __syncthreads();
    float *wsb = ws + (size_t)blockIdx.x * 2 * C;
    for (int c = tid; c < C; c += LN_THREADS) {
        float a = part[0][0][c], b = part[0][1][c];
#pragma unroll
        for (int u = 1; u < LN_WAVES; ++u) {
            a += part[u][0][c];
            b += part[u][1][c];
        }
        wsb[c] = a;
        wsb[C + c] = b;
    }
}

// entry t of the per-block partials [blocks][2][C], blocks in ascending order.  One thread walks a column of the workspace:
// eight loads are put in flight before their eight adds (the same order of adds; the walk is bound by load latency).
constexpr int LN_FOLD_THREADS = 64;

__global__ __launch_bounds__(LN_FOLD_THREADS) void layernorm_fold_kernel(const float *__restrict__ ws, int blocks, int C,
                                                                         float *__restrict__ dweight,
                                                                         float *__restrict__ dbias)
{
    const int t = blockIdx.x * LN_FOLD_THREADS + threadIdx.x;
    if (t >= 2 * C) return;
    const size_t stride = (size_t)2 * C;
    const float *col = ws + t;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= blocks; b += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(size_t)(b + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < blocks; ++b) s += col[(size_t)b * stride];
    if (t < C) dweight[t] = s;
    else dbias[t - C] = s;
}

constexpr float GELU_RSQRT2 = 0.70710678118654752440f;      // 1 / sqrt 2
constexpr float GELU_RSQRT2PI = 0.39894228040143267794f;    // 1 / sqrt(2 pi)

__device__ __forceinline__ float gelu_cdf(float z) { return 0.5f * (1.f + erff(z * GELU_RSQRT2)); }

// operands of the row dropout; the plain instantiations carry the empty form
template <bool DROP>
struct RowDrop {};

template <>
struct RowDrop<true> {
    float p, inv;                          // rate, 1.f / (1.f - p)
    unsigned long long seed;
};

// element idx = r * C + c is kept: the forward and the regenerating backward ask with the same (seed, idx)
__device__ __forceinline__ bool row_kept(const RowDrop<true> &dr, unsigned long long idx)
{
    return hash_uniform(dr.seed, idx) >= dr.p;
}

template <int V, bool DROP>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float *__restrict__ z, int ldz, long long R, int C,
                                                       float *__restrict__ out, int ldo, RowDrop<DROP> dr)
{
    const int cpr = C / V;
    const long long total = R * cpr;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long r = t / cpr;
        const int c = (int)(t - r * cpr) * V;
        float a[V], o[V];
        ro_load<V>(z + (size_t)r * ldz + c, a);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            o[v] = a[v] * gelu_cdf(a[v]);
            if constexpr (DROP) o[v] = row_kept(dr, (unsigned long long)r * C + c + v) ? __fmul_rn(o[v], dr.inv) : 0.f;
        }
        ro_store<V>(out + (size_t)r * ldo + c, o);
    }
}

template <int V, bool DROP>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float *__restrict__ g, int ldg, const float *__restrict__ z,
                                                       int ldz, long long R, int C, float *__restrict__ dz, int lddz,
                                                       RowDrop<DROP> dr)
{
    const int cpr = C / V;
    const long long total = R * cpr;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long r = t / cpr;
        const int c = (int)(t - r * cpr) * V;
        float a[V], gv[V], o[V];
        ro_load<V>(z + (size_t)r * ldz + c, a);
        ro_load<V>(g + (size_t)r * ldg + c, gv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float d = gelu_cdf(a[v]) + a[v] * expf(-0.5f * a[v] * a[v]) * GELU_RSQRT2PI;
            if constexpr (DROP) o[v] = row_kept(dr, (unsigned long long)r * C + c + v) ? __fmul_rn(gv[v], dr.inv) * d : 0.f;
            else o[v] = gv[v] * d;
        }
        ro_store<V>(dz + (size_t)r * lddz + c, o);
    }
}

// out = x + (keep ? y * inv : 0): the residual add behind a dropped sublayer output
template <int V>
__global__ __launch_bounds__(256) void dropout_add_fwd_kernel(const float *__restrict__ y, int ldy,
                                                              const float *__restrict__ x, int ldx, long long R, int C,
                                                              float *__restrict__ out, int ldo, RowDrop<true> dr)
{
    const int cpr = C / V;
    const long long total = R * cpr;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long r = t / cpr;
        const int c = (int)(t - r * cpr) * V;
        float a[V], b[V], o[V];
        ro_load<V>(y + (size_t)r * ldy + c, a);
        ro_load<V>(x + (size_t)r * ldx + c, b);
#pragma unroll
        for (int v = 0; v < V; ++v)
            o[v] = b[v] + (row_kept(dr, (unsigned long long)r * C + c + v) ? __fmul_rn(a[v], dr.inv) : 0.f);
        ro_store<V>(out + (size_t)r * ldo + c, o);
    }
}

// dy = keep ? g * inv : 0 with the forward's mask regenerated
template <int V>
__global__ __launch_bounds__(256) void dropout_regen_bwd_kernel(const float *__restrict__ g, int ldg, long long R, int C,
                                                                float *__restrict__ dy, int lddy, RowDrop<true> dr)
{
    const int cpr = C / V;
    const long long total = R * cpr;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long r = t / cpr;
        const int c = (int)(t - r * cpr) * V;
        float a[V], o[V];
        ro_load<V>(g + (size_t)r * ldg + c, a);
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = row_kept(dr, (unsigned long long)r * C + c + v) ? __fmul_rn(a[v], dr.inv) : 0.f;
        ro_store<V>(dy + (size_t)r * lddy + c, o);
    }
}

}  // namespace

// floats of cova_layernorm_bwd's workspace: 2 * C partial sums (dweight | dbias) per block of LN_BWD_ROWS rows
COVA_API int cova_layernorm_workspace_floats(int R, int C)
{
    if (R <= 0 || C < 1 || C > LN_MAX_C) return 0;
    const long long n = (long long)cdiv(R, LN_BWD_ROWS) * 2 * C;
    return n > 0x7fffffffLL ? -1 : (int)n;
}

COVA_API int cova_layernorm_fwd(const float *x, int ldx, int R, int C, const float *weight, const float *bias, float eps,
                                float *out, int ldo, float *mean, float *rstd, void *stream)
{
    COVA_REQUIRE(C >= 1 && C <= LN_MAX_C && R >= 0 && ldx >= C && ldo >= C && eps >= 0.f);
    if (R == 0) return COVA_OK;
    COVA_REQUIRE(x && weight && bias && out && mean && rstd);
    const bool v4 = C % 4 == 0 && vec4_ok(x, ldx) && vec4_ok(out, ldo) && aligned16(weight) && aligned16(bias);
    const int grid = cdiv(R, LN_WAVES) < LN_FWD_MAX_BLOCKS ? cdiv(R, LN_WAVES) : LN_FWD_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(layernorm_fwd_kernel<4>, dim3(grid), dim3(LN_THREADS), st, x, ldx, R, C, weight, bias, eps, out,
                    ldo, mean, rstd);
    else
        COVA_LAUNCH(layernorm_fwd_kernel<1>, dim3(grid), dim3(LN_THREADS), st, x, ldx, R, C, weight, bias, eps, out,
                    ldo, mean, rstd);
    return COVA_OK;
}

COVA_API int cova_layernorm_bwd(const float *g, int ldg, const float *x, int ldx, const float *mean, const float *rstd,
                                const float *weight, int R, int C, const float *res, int ldr, float *dx, int lddx,
                                float *dweight, float *dbias, float *ws, void *stream)
{
    COVA_REQUIRE(C >= 1 && C <= LN_MAX_C && R >= 0 && ldg >= C && ldx >= C && lddx >= C && (!res || ldr >= C));
    if (R == 0) return COVA_OK;
    COVA_REQUIRE(g && x && mean && rstd && weight && dx && dweight && dbias && ws);
    COVA_REQUIRE(cova_layernorm_workspace_floats(R, C) > 0);
    const bool v4 = C % 4 == 0 && vec4_ok(g, ldg) && vec4_ok(x, ldx) && vec4_ok(res, ldr) && vec4_ok(dx, lddx) &&
                    aligned16(weight);
    const int blocks = cdiv(R, LN_BWD_ROWS);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(layernorm_bwd_kernel<4>, dim3(blocks), dim3(LN_THREADS), st, g, ldg, x, ldx, mean, rstd, weight,
                    R, C, res, ldr, dx, lddx, ws);
    else
        COVA_LAUNCH(layernorm_bwd_kernel<1>, dim3(blocks), dim3(LN_THREADS), st, g, ldg, x, ldx, mean, rstd, weight,
                    R, C, res, ldr, dx, lddx, ws);
    COVA_LAUNCH(layernorm_fold_kernel, dim3(cdiv(2 * C, LN_FOLD_THREADS)), dim3(LN_FOLD_THREADS), st, ws, blocks, C,
                dweight, dbias);
    return COVA_OK;
}

template <bool DROP>
static int gelu_fwd(const float *z, int ldz, long long R, int C, float *out, int ldo, RowDrop<DROP> dr, void *stream)
{
    COVA_REQUIRE(C >= 1 && R >= 0 && ldz >= C && ldo >= C);
    if (R == 0) return COVA_OK;
    COVA_REQUIRE(z && out);
    const bool v4 = C % 4 == 0 && vec4_ok(z, ldz) && vec4_ok(out, ldo);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(HIP_KERNEL_NAME(gelu_fwd_kernel<4, DROP>), dim3(ew_grid(R * (C / 4))), dim3(256), st, z, ldz, R, C,
                    out, ldo, dr);
    else
        COVA_LAUNCH(HIP_KERNEL_NAME(gelu_fwd_kernel<1, DROP>), dim3(ew_grid(R * C)), dim3(256), st, z, ldz, R, C, out,
                    ldo, dr);
    return COVA_OK;
}

template <bool DROP>
static int gelu_bwd(const float *g, int ldg, const float *z, int ldz, long long R, int C, float *dz, int lddz,
                    RowDrop<DROP> dr, void *stream)
{
    COVA_REQUIRE(C >= 1 && R >= 0 && ldg >= C && ldz >= C && lddz >= C);
    if (R == 0) return COVA_OK;
    COVA_REQUIRE(g && z && dz);
    const bool v4 = C % 4 == 0 && vec4_ok(g, ldg) && vec4_ok(z, ldz) && vec4_ok(dz, lddz);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(HIP_KERNEL_NAME(gelu_bwd_kernel<4, DROP>), dim3(ew_grid(R * (C / 4))), dim3(256), st, g, ldg, z,
                    ldz, R, C, dz, lddz, dr);
    else
        COVA_LAUNCH(HIP_KERNEL_NAME(gelu_bwd_kernel<1, DROP>), dim3(ew_grid(R * C)), dim3(256), st, g, ldg, z, ldz, R,
                    C, dz, lddz, dr);
    return COVA_OK;
}

COVA_API int cova_gelu_fwd(const float *z, int ldz, long long R, int C, float *out, int ldo, void *stream)
{
    return gelu_fwd<false>(z, ldz, R, C, out, ldo, RowDrop<false>{}, stream);
}

COVA_API int cova_gelu_bwd(const float *g, int ldg, const float *z, int ldz, long long R, int C, float *dz, int lddz,
                           void *stream)
{
    return gelu_bwd<false>(g, ldg, z, ldz, R, C, dz, lddz, RowDrop<false>{}, stream);
}

// 0 < p < 1: a NaN fails both compares
static bool row_drop_ok(float p) { return p > 0.f && p < 1.f; }

static RowDrop<true> row_drop_of(float p, unsigned long long seed) { return RowDrop<true>{p, 1.f / (1.f - p), seed}; }

COVA_API int cova_gelu_fwd_drop(const float *z, int ldz, long long R, int C, float *out, int ldo, float p,
                                unsigned long long seed, void *stream)
{
    COVA_REQUIRE(row_drop_ok(p));
    return gelu_fwd<true>(z, ldz, R, C, out, ldo, row_drop_of(p, seed), stream);
}

COVA_API int cova_gelu_bwd_drop(const float *g, int ldg, const float *z, int ldz, long long R, int C, float *dz, int lddz,
                                float p, unsigned long long seed, void *stream)
{
    COVA_REQUIRE(row_drop_ok(p));
    return gelu_bwd<true>(g, ldg, z, ldz, R, C, dz, lddz, row_drop_of(p, seed), stream);
}

COVA_API int cova_dropout_add_fwd(const float *y, int ldy, const float *x, int ldx, float *out, int ldo, long long R, int C,
                                  float p, unsigned long long seed, void *stream)
{
    COVA_REQUIRE(row_drop_ok(p) && C >= 1 && R >= 0 && ldy >= C && ldx >= C && ldo >= C);
    if (R == 0) return COVA_OK;
    COVA_REQUIRE(y && x && out && out != y && out != x);
    const bool v4 = C % 4 == 0 && vec4_ok(y, ldy) && vec4_ok(x, ldx) && vec4_ok(out, ldo);
    const RowDrop<true> dr = row_drop_of(p, seed);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(dropout_add_fwd_kernel<4>, dim3(ew_grid(R * (C / 4))), dim3(256), st, y, ldy, x, ldx, R, C, out,
                    ldo, dr);
    else
        COVA_LAUNCH(dropout_add_fwd_kernel<1>, dim3(ew_grid(R * C)), dim3(256), st, y, ldy, x, ldx, R, C, out, ldo,
                    dr);
    return COVA_OK;
}

COVA_API int cova_dropout_regen_bwd(const float *g, int ldg, float *dy, int lddy, long long R, int C, float p,
                                    unsigned long long seed, void *stream)
{
    COVA_REQUIRE(row_drop_ok(p) && C >= 1 && R >= 0 && ldg >= C && lddy >= C);
    if (R == 0) return COVA_OK;
    COVA_REQUIRE(g && dy && g != dy);
    const bool v4 = C % 4 == 0 && vec4_ok(g, ldg) && vec4_ok(dy, lddy);
    const RowDrop<true> dr = row_drop_of(p, seed);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(dropout_regen_bwd_kernel<4>, dim3(ew_grid(R * (C / 4))), dim3(256), st, g, ldg, R, C, dy, lddy,
                    dr);
    else
        COVA_LAUNCH(dropout_regen_bwd_kernel<1>, dim3(ew_grid(R * C)), dim3(256), st, g, ldg, R, C, dy, lddy, dr);
    return COVA_OK;
}
