// Page readout: the attention-pooled page vector every box of a page receives as context,
//   u_i = a . P_i + b,  e_i = u_i > 0 ? u_i : alpha * u_i,  beta = softmax of e over the page's rows,  r_p = sum beta_i P_i,
// and its hand-written backward.  One block of sixteen waves per page (page_rows(), rows.h: both ends clamped into [0, N]);
// waves stride over the page's rows, lanes sit over channels (float4 chunks lane, lane + 64 when G % 4 == 0 and every
// leading dimension and base is 16-byte aligned, scalar channels lane, lane + 64, ... otherwise).  u and beta live in
// global memory, LDS holds RO_WAVES + 1 rows of 512 floats: a page of any size runs.
//
// Summation orders (all f32, every one a function of the page's own row count and G alone; no atomics, no host read):
//   a . P_i, gr . P_i, gr . r_p   a lane's channels in ascending order as one fma chain from -0 (the additive identity: a
//                          sum of signed zeros keeps its sign), then the xor butterfly (offsets 32, 16, .., 1)
//   max_p e                wave w keeps the maximum of rows w, w + 16, ... (f32 compares, a NaN never wins), then waves 0..15
//   sum_p exp(e - max)     thread t adds rows t, t + 1024, ... in turn, the butterfly, then the tree of adjacent pairs over
//                          the waves, ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) ... (ro_tree)
//   r_p, gr_p, d_att partials   wave w accumulates rows w, w + 16, ... in turn per channel (fma for the weighted sums, plain
//                          adds for gr_p and d_att_b), then the same tree over the waves
//   d_att_w, d_att_b       per-page partials in ws [B, G + 1], folded by readout_fold_kernel over pages 0, 1, .., B - 1
// The per-page outputs (u, beta, r, out, dP) therefore keep their bits whatever other pages share the batch.
#include "rows.h"

// the orders above count one rounding per written operation: only the fmaf calls fuse
#pragma clang fp contract(off)

namespace {

constexpr int RO_THREADS = 1024;          // 16 waves: a page is one block, its rows are the only parallelism it has
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_MAX_G = 512;

// x . y over the wave's channels; absent chunks hold zeros in x
template <int V, int NCH>
__device__ __forceinline__ float ro_dot(const float (&x)[NCH][V], const float *__restrict__ row, int lane, int G)
{
    float d = -0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < G) {
            float y[V];
            ro_load<V>(row + c, y);
#pragma unroll
            for (int v = 0; v < V; ++v) d = fmaf(x[k][v], y[v], d);
        }
    }
    return wave_sum(d);
}

// one value per wave, folded as a tree of adjacent pairs: ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) ...
__device__ __forceinline__ float ro_tree(float (&v)[RO_WAVES])
{
#pragma unroll
    for (int h = RO_WAVES / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int w = 0; w < h; ++w) v[w] = v[2 * w] + v[2 * w + 1];
    return v[0];
}

// channel c of the waves' rows of `part`
__device__ __forceinline__ float ro_fold(const float (*part)[RO_MAX_G], int c)
{
    float v[RO_WAVES];
#pragma unroll
    for (int w = 0; w < RO_WAVES; ++w) v[w] = part[w][c];
    return ro_tree(v);
}

__device__ __forceinline__ float ro_fold_scalar(const float *red)
{
    float v[RO_WAVES];
#pragma unroll
    for (int w = 0; w < RO_WAVES; ++w) v[w] = red[w];
    return ro_tree(v);
}

__device__ __forceinline__ float ro_lrelu(float u, float alpha) { return u > 0.f ? u : alpha * u; }

template <int V>
__global__ __launch_bounds__(RO_THREADS) void readout_fwd_kernel(
    const float *__restrict__ P, int ldp, const float *__restrict__ att_w, const float *__restrict__ att_b,
    const int64_t *__restrict__ page_start, int N, int G, float alpha, float *u, float *__restrict__ beta,
    float *__restrict__ r, float *__restrict__ out, int ldo)
{
    constexpr int NCH = RO_MAX_G / (64 * V);
    __shared__ __attribute__((aligned(16))) float part[RO_WAVES][RO_MAX_G];
    __shared__ __attribute__((aligned(16))) float whole[RO_MAX_G];
    __shared__ float red[RO_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const PageRows pr = page_rows(page_start, p, N);
    const int base = pr.base, n = pr.end - pr.base;
    if (n == 0) return;                                  // an empty page writes nothing (block-uniform)

    float a[NCH][V];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) a[k][v] = 0.f;
        if (c < G) ro_load<V>(att_w + c, a[k]);
    }
    const float b = att_b[0];

    // scores and the page's maximum
    float m = -INFINITY;
    for (int i = wave; i < n; i += RO_WAVES) {
        const float ui = ro_dot<V, NCH>(a, P + (size_t)(base + i) * ldp, lane, G) + b;
        if (lane == 0) u[base + i] = ui;
        const float e = ro_lrelu(ui, alpha);
        if (e > m) m = e;
    }
    if (lane == 0) red[wave] = m;
    __syncthreads();                                     // (also orders the u stores before the reads below)
    m = red[0];
#pragma unroll
    for (int w = 1; w < RO_WAVES; ++w)
        if (red[w] > m) m = red[w];
    __syncthreads();

    // the softmax denominator
    float s = 0.f;
    for (int i = tid; i < n; i += RO_THREADS) s += expf(ro_lrelu(u[base + i], alpha) - m);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = ro_fold_scalar(red);

    // beta and the weighted row sum
    float acc[NCH][V];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[k][v] = 0.f;
    for (int i = wave; i < n; i += RO_WAVES) {
        const float bi = expf(ro_lrelu(u[base + i], alpha) - m) / s;
        if (lane == 0) beta[base + i] = bi;
        const float *row = P + (size_t)(base + i) * ldp;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < G) {
                float x[V];
                ro_load<V>(row + c, x);
#pragma unroll
                for (int v = 0; v < V; ++v) acc[k][v] = fmaf(bi, x[v], acc[k][v]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < G) ro_store<V>(&part[wave][c], acc[k]);
    }
    __syncthreads();
    for (int c = tid; c < G; c += RO_THREADS) whole[c] = r[(size_t)p * G + c] = ro_fold(part, c);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < G) ro_load<V>(&whole[c], acc[k]);
    }

    // every box of the page gets the page's vector
    for (int i = wave; i < n; i += RO_WAVES) {
        float *row = out + (size_t)(base + i) * ldo;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < G) ro_store<V>(row + c, acc[k]);
        }
    }
}

template <int V>
__global__ __launch_bounds__(RO_THREADS) void readout_bwd_kernel(
    const float *__restrict__ g, int ldg, const float *__restrict__ P, int ldp, const float *__restrict__ u,
    const float *__restrict__ beta, const float *__restrict__ r, const float *__restrict__ att_w,
    const int64_t *__restrict__ page_start, int N, int G, float alpha, float *__restrict__ dP, int lddp,
    float *__restrict__ ws)
{
    constexpr int NCH = RO_MAX_G / (64 * V);
    __shared__ __attribute__((aligned(16))) float part[RO_WAVES][RO_MAX_G];
    __shared__ __attribute__((aligned(16))) float whole[RO_MAX_G];
    __shared__ float red[RO_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const PageRows pr = page_rows(page_start, p, N);
    const int base = pr.base, n = pr.end - pr.base;
    float *wsp = ws + (size_t)p * (G + 1);
    if (n == 0) {                                        // an empty page adds nothing to d_att_w / d_att_b
        for (int c = tid; c <= G; c += RO_THREADS) wsp[c] = 0.f;
        return;
    }

    // gr_p = sum of the page's incoming gradient rows
    float gr[NCH][V];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int v = 0; v < V; ++v) gr[k][v] = 0.f;
    for (int i = wave; i < n; i += RO_WAVES) {
        const float *row = g + (size_t)(base + i) * ldg;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < G) {
                float x[V];
                ro_load<V>(row + c, x);
#pragma unroll
                for (int v = 0; v < V; ++v) gr[k][v] += x[v];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < G) ro_store<V>(&part[wave][c], gr[k]);
    }
    __syncthreads();
    for (int c = tid; c < G; c += RO_THREADS) whole[c] = ro_fold(part, c);
    __syncthreads();                                     // (part is written again below)
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < G) ro_load<V>(&whole[c], gr[k]);
    }

    const float c0 = ro_dot<V, NCH>(gr, r + (size_t)p * G, lane, G);      // gr_p . r_p, the same bits in every wave
    float a[NCH][V], da[NCH][V];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) a[k][v] = da[k][v] = 0.f;
        if (c < G) ro_load<V>(att_w + c, a[k]);
    }

    // a wave per row: dP_i = beta_i gr_p + du_i a; the page's d_att partials
    float db = 0.f;
    for (int i = wave; i < n; i += RO_WAVES) {
        const float *row = P + (size_t)(base + i) * ldp;
        float x[NCH][V];
        float d = -0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
#pragma unroll
            for (int v = 0; v < V; ++v) x[k][v] = 0.f;
            if (c < G) {
                ro_load<V>(row + c, x[k]);
#pragma unroll
                for (int v = 0; v < V; ++v) d = fmaf(gr[k][v], x[k][v], d);
            }
        }
        const float dbeta = wave_sum(d);
        const float bi = beta[base + i], ui = u[base + i];
        const float de = bi * (dbeta - c0);
        const float du = de * (ui > 0.f ? 1.f : alpha);
        db += du;
        float *drow = dP + (size_t)(base + i) * lddp;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = (lane + 64 * k) * V;
            if (c < G) {
                float o[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    o[v] = fmaf(du, a[k][v], bi * gr[k][v]);
                    da[k][v] = fmaf(du, x[k][v], da[k][v]);
                }
                ro_store<V>(drow + c, o);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = (lane + 64 * k) * V;
        if (c < G) ro_store<V>(&part[wave][c], da[k]);
    }
    if (lane == 0) red[wave] = db;
    __syncthreads();
    for (int c = tid; c < G; c += RO_THREADS) wsp[c] = ro_fold(part, c);
    if (tid == 0) wsp[G] = ro_fold_scalar(red);
}

// column c of the per-page partials, pages in ascending order
__global__ __launch_bounds__(RO_THREADS) void readout_fold_kernel(const float *__restrict__ ws, int B, int G,
                                                                  float *__restrict__ d_att_w, float *__restrict__ d_att_b)
{
    const int c = blockIdx.x * RO_THREADS + threadIdx.x;
    if (c > G) return;
    float s = 0.f;
    for (int p = 0; p < B; ++p) s += ws[(size_t)p * (G + 1) + c];
    if (c < G) d_att_w[c] = s;
    else d_att_b[0] = s;
}

}  // namespace

// floats of cova_page_readout_bwd's workspace: G + 1 partial sums (d_att_w | d_att_b) per page
COVA_API int cova_page_readout_workspace_floats(int B, int G)
{
    if (B <= 0 || G < 1 || G > RO_MAX_G) return 0;
    const long long n = (long long)B * (G + 1);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

COVA_API int cova_page_readout_fwd(const float *P, int ldp, const float *att_w, const float *att_b,
                                   const int64_t *page_start, int B, int N, int G, float alpha, float *u, float *beta,
                                   float *r, float *out, int ldo, void *stream)
{
    COVA_REQUIRE(G >= 1 && G <= RO_MAX_G && N >= 0 && B >= 0 && ldp >= G && ldo >= G);
    if (N == 0 || B == 0) return COVA_OK;
    COVA_REQUIRE(P && att_w && att_b && page_start && u && beta && r && out);
    const bool v4 = G % 4 == 0 && vec4_ok(P, ldp) && vec4_ok(out, ldo) && aligned16(att_w) && aligned16(r);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(readout_fwd_kernel<4>, dim3(B), dim3(RO_THREADS), st, P, ldp, att_w, att_b, page_start, N, G,
                    alpha, u, beta, r, out, ldo);
    else
        COVA_LAUNCH(readout_fwd_kernel<1>, dim3(B), dim3(RO_THREADS), st, P, ldp, att_w, att_b, page_start, N, G,
                    alpha, u, beta, r, out, ldo);
    return COVA_OK;
}

COVA_API int cova_page_readout_bwd(const float *g, int ldg, const float *P, int ldp, const float *u, const float *beta,
                                   const float *r, const float *att_w, const int64_t *page_start, int B, int N, int G,
                                   float alpha, float *dP, int lddp, float *d_att_w, float *d_att_b, float *ws,
                                   void *stream)
{
    COVA_REQUIRE(G >= 1 && G <= RO_MAX_G && N >= 0 && B >= 0 && ldg >= G && ldp >= G && lddp >= G);
    if (N == 0 || B == 0) return COVA_OK;
    COVA_REQUIRE(g && P && u && beta && r && att_w && page_start && dP && d_att_w && d_att_b && ws);
    COVA_REQUIRE(cova_page_readout_workspace_floats(B, G) > 0);
    const bool v4 = G % 4 == 0 && vec4_ok(g, ldg) && vec4_ok(P, ldp) && vec4_ok(dP, lddp) && aligned16(att_w) &&
                    aligned16(r);
    hipStream_t st = (hipStream_t)stream;
    if (v4)
        COVA_LAUNCH(readout_bwd_kernel<4>, dim3(B), dim3(RO_THREADS), st, g, ldg, P, ldp, u, beta, r, att_w,
                    page_start, N, G, alpha, dP, lddp, ws);
    else
        COVA_LAUNCH(readout_bwd_kernel<1>, dim3(B), dim3(RO_THREADS), st, g, ldg, P, ldp, u, beta, r, att_w,
                    page_start, N, G, alpha, dP, lddp, ws);
    COVA_LAUNCH(readout_fold_kernel, dim3(cdiv(G + 1, RO_THREADS)), dim3(RO_THREADS), st, ws, B, G, d_att_w,
                d_att_b);
    return COVA_OK;
}
