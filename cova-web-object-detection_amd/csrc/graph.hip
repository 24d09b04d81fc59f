// Context graphs built on the device: the DOM-order window of cova_collate_boxes plus the k nearest other boxes of the page
// (include/cova_hip.h, cova_context_knn).  The graph is built AFTER background-box sampling (datasets.py:117-128 builds its
// window over the kept boxes), so it is a kernel: the kept boxes of a page are decided on the card.
//   context_knn_kernel   one wave per box, four waves per block.  The page is found by binary search of page_offsets; lanes
//                        write the window slots; then k_spatial selection rounds: lane l recomputes the packed key of the
//                        candidates l, l+64, ... and keeps the smallest (key, j) strictly above the pair emitted last; a
//                        6-step wave min-reduction picks the winner and lane 0 stores it.  The first four candidates of a
//                        lane keep their keys in registers (a page of the reference's data, 11-230 boxes, is covered);
//                        the candidates behind them are recomputed every round, with no storage: any n.
//   edge_geometry_kernel the eight relative-geometry features of every edge of a context table (cova_edge_geometry), one
//                        thread per slot.
// Integer compares of float bit patterns, every float operation rounded on its own: bit-deterministic, equal to numpy.
// knn_box and edge_features live in geometry.h: page_attn.hip forms the same feature bits for its geometry bias.
#include "geometry.h"
#include <limits.h>

namespace {

constexpr int KNN_THREADS = 256;           // four waves = four boxes per block
constexpr unsigned long long KNN_NONE = ~0ull;
constexpr int KNN_HELD = 4;                // candidate keys a lane keeps in registers: pages of up to 256 boxes

// (gap2, ctr2) of boxes a, b = x1,y1,x2,y2 as (bits(gap2) << 32) | bits(ctr2).  Both are sums of squares: non-negative (never
// -0), so for finite boxes the bit patterns order as the floats do.  No contraction: a fused multiply-add would round gap2 and
// ctr2 once instead of three times and differ from the host formulation in the last bit (__fmul_rn is a plain `*` here).
__device__ __forceinline__ unsigned long long knn_key(const float4 a, const float4 b)
{
#pragma clang fp contract(off)
    const float dx = fmaxf(0.f, fmaxf(a.x, b.x) - fminf(a.z, b.z));
    const float dy = fmaxf(0.f, fmaxf(a.y, b.y) - fminf(a.w, b.w));
    const float dx2 = dx * dx, dy2 = dy * dy;
    const float gap2 = dx2 + dy2;
    const float ex = (a.x + a.z) - (b.x + b.z);
    const float ey = (a.y + a.w) - (b.y + b.w);
    const float ex2 = ex * ex, ey2 = ey * ey;
    const float ctr2 = ex2 + ey2;
    return ((unsigned long long)__float_as_uint(gap2) << 32) | (unsigned long long)__float_as_uint(ctr2);
}

__global__ __launch_bounds__(KNN_THREADS) void context_knn_kernel(
    const float *__restrict__ bboxes, const int *__restrict__ page_offsets, int B, int N, int cs, int ks,
    long long *__restrict__ ctx)
{
    const int lane = threadIdx.x & 63;
    const int K = 2 * cs + ks;
    const long long waves = (long long)gridDim.x * (KNN_THREADS / 64);
    for (long long gw = (long long)blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6); gw < N; gw += waves) {
        const int g = (int)gw;                             // wave-uniform
        long long *row = ctx + (long long)g * K;
        int lo = 0, hi = B;                                // page of box g: page_offsets[lo] <= g < [lo+1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (page_offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const int base = page_offsets[lo], n = page_offsets[lo + 1] - base, i = g - base;
        if (base < 0 || i < 0 || i >= n || (long long)base + n > N) {      // a malformed table: pads, nothing read
            for (int s = lane; s < K; s += 64) row[s] = -1;
            continue;
        }
        // DOM window, exactly cova_collate_boxes' slots
        const int nleft = min(i, cs), nright = min(n - 1 - i, cs);
        for (int s = lane; s < 2 * cs; s += 64) {
            long long v = -1;
            if (s < nleft) v = base + (i - nleft + s);
            else if (s < nleft + nright) v = base + (i + 1 + (s - nleft));
            row[s] = v;
        }
        if (ks == 0) continue;
        const float4 me = knn_box(bboxes, g);
        // the keys of the first KNN_HELD candidates of a lane (pages of up to 256 boxes: all of them) are computed once
        unsigned long long held[KNN_HELD];
        unsigned held_ok = 0;
#pragma unroll
        for (int t = 0; t < KNN_HELD; ++t) {
            const int j = lane + 64 * t;
            const bool ok = j < n && abs(j - i) > cs;      // not the box itself, not a window member
            held[t] = ok ? knn_key(me, knn_box(bboxes, (long long)base + j)) : 0ull;
            held_ok |= (ok ? 1u : 0u) << t;
        }
        unsigned long long last_key = 0;
        int last_j = -1;                                   // (0, -1) lies below every candidate
        int r = 0;
        for (; r < ks; ++r) {
            unsigned long long best = KNN_NONE;
            int best_j = INT_MAX;
            auto consider = [&](unsigned long long key, int j) {
                const bool above = key > last_key || (key == last_key && j > last_j);
                const bool below = key < best || (key == best && j < best_j);
                if (above && below) { best = key; best_j = j; }
            };
#pragma unroll
            for (int t = 0; t < KNN_HELD; ++t)
                if ((held_ok >> t) & 1u) consider(held[t], lane + 64 * t);
            for (int j = lane + 64 * KNN_HELD; j < n; j += 64) {           // larger pages: recomputed every round, no storage
                if (abs(j - i) <= cs) continue;
                consider(knn_key(me, knn_box(bboxes, (long long)base + j)), j);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long ok = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(best_j, o, 64);
                if (ok < best || (ok == best && oj < best_j)) { best = ok; best_j = oj; }
            }
            if (best_j == INT_MAX) break;                  // the candidates are used up (wave-uniform)
            if (lane == 0) row[2 * cs + r] = (long long)base + best_j;
            last_key = best;
            last_j = best_j;
        }
        for (int s = r + lane; s < ks; s += 64) row[2 * cs + s] = -1;
    }
}

// one thread per slot (i, k), grid-stride; a pad (j < 0 or j >= N) writes eight zeros and reads no box
__global__ __launch_bounds__(256) void edge_geometry_kernel(const float *__restrict__ bboxes,
                                                            const long long *__restrict__ ctx, int N, int K, float W,
                                                            float H, float *__restrict__ phi)
{
    const long long E = (long long)N * K, step = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += step) {
        const long long i = e / K, j = ctx[e];
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j >= 0 && j < N) {
            const long long d = j - i;
            edge_features(knn_box(bboxes, i), knn_box(bboxes, j), W, H, (int)d, f);
        }
        float4 *out = reinterpret_cast<float4 *>(phi + e * 8);
        out[0] = make_float4(f[0], f[1], f[2], f[3]);
        out[1] = make_float4(f[4], f[5], f[6], f[7]);
    }
}

}  // namespace

COVA_API int cova_edge_geometry(const float *bboxes, const long long *ctx, int N, int K, float img_w, float img_h,
                                float *phi, void *stream)
{
    COVA_REQUIRE(N >= 0 && K >= 0 && K <= COVA_GAT_MAX_K);
    if (N == 0 || K == 0) return COVA_OK;
    COVA_REQUIRE(bboxes && ctx && phi && ((uintptr_t)phi & 15) == 0 && img_w > 0.f && img_h > 0.f);
    long long blocks = ((long long)N * K + 255) / 256;
    if (blocks > 64 * 1024) blocks = 64 * 1024;
    COVA_LAUNCH(edge_geometry_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, bboxes, ctx, N, K,
                img_w, img_h, phi);
    return COVA_OK;
}

COVA_API int cova_context_knn(const float *bboxes, const int *page_offsets, int B, int N, int context_size, int k_spatial,
                              long long *ctx, void *stream)
{
    COVA_REQUIRE(B >= 0 && N >= 0 && context_size >= 0 && k_spatial >= 0);
    COVA_REQUIRE(context_size <= COVA_GAT_MAX_K && k_spatial <= COVA_GAT_MAX_K &&
                 2 * context_size + k_spatial <= COVA_GAT_MAX_K);
    if (N == 0 || 2 * context_size + k_spatial == 0) return COVA_OK;
    COVA_REQUIRE(B > 0 && bboxes && page_offsets && ctx);
    long long blocks = ((long long)N + KNN_THREADS / 64 - 1) / (KNN_THREADS / 64);
    if (blocks > 256 * 1024) blocks = 256 * 1024;
    COVA_LAUNCH(context_knn_kernel, dim3((unsigned)blocks), dim3(KNN_THREADS), (hipStream_t)stream, bboxes,
                page_offsets, B, N, context_size, k_spatial, ctx);
    return COVA_OK;
}
