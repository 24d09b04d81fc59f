// GATv2 ("dynamic") scoring of the graph-attention head: cova_gat2_fwd / cova_gat2_bwd (include/cova_hip.h).
//
//   z[i,k,d] = Wh[i,d] + Wh[j,D+d]           j = ctx[i,k]; ONE f32 add, the same in all three kernels below
//   u[i,k]   = b + sum_d a[d] * lrelu(z)     lrelu(z) = z > 0 ? z : slope * z  (z == +-0 takes the slope branch)
//            (+ edge_w . phi[i,k,:], added last: OUTSIDE the non-linearity -- the static layer has it inside)
//   mask (-9e15 on pads and ids >= N), softmax over k, h'[i] = sum_k attn[i,k] * Wh[j, D:2D]   as cova_gat_fwd
//
// The score is no longer s[i] + t[j]: every edge needs a D-wide reduction in the forward and a per-channel gate in the
// backward.  All kernels are one wave per node, four nodes per 256-thread block.  Lanes run over channels: lane l owns the V
// adjacent channels (64 c + l) V .. + V - 1 of chunk c (V = 4: one float4 per row and chunk; V = 1: the scalar form for
// D % 4 != 0 or unaligned operands), NC chunks per row, a node's own row and the attention vector in registers.  The K
// scores of a node land one per lane (slot k in lane k & 63 of pass k >> 6) and wait in a per-lane LDS column between
// the passes (a lane only ever reads back what it wrote: no cross-lane traffic through LDS, no barrier).
// Neighbour rows are read twice (scores, then aggregation; dalpha, then gates): K rows of D floats do not fit a wave's
// registers, and at the DOM-window graphs the rows are L2-resident.
// No float atomics: every sum has a fixed order (channels ascending inside a lane, the wave butterfly, slots / CSR edges
// ascending, nodes in blocks of four, blocks in index order), so reruns are bit-identical, and a node's outputs depend on
// its own row and its neighbours' only.
#include "common.h"

namespace {

// slots (edges) whose rows are in flight together: fewer for wide rows (at most 64 row registers per gathered operand)
template <int NC, int V> constexpr int gat2_unroll() { return NC * V >= 32 ? 2 : NC * V >= 16 ? 4 : 8; }

template <int V>
__device__ __forceinline__ void ldv(const float *__restrict__ p, float (&r)[V])
{
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void stv(float *__restrict__ p, const float (&r)[V])
{
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else p[0] = r[0];
}

// ------------------------------------------------------------------------------------------------ forward
// DROP (all three kernels): attention dropout (common.h, GatDrop) -- attn keeps the softmax output, the aggregation and the
// destination side weigh with gat_dropped(e, attn[e]), the source side scales dattn by keep * inv before the softmax backward.
template <int NC, int V, bool EDGE, bool DROP = false>
__global__ __launch_bounds__(256) void gat2_fwd_kernel(
    const float *__restrict__ Wh, int ldw, const float *__restrict__ att_w, const float *__restrict__ att_b,
    const int64_t *__restrict__ ctx, const float *__restrict__ phi, const float *__restrict__ edge_w, int N, int K, int D,
    float slope, float *__restrict__ attn, float *__restrict__ hprime, int ldh, GatDrop dr = GatDrop{})
{
    constexpr int U = gat2_unroll<NC, V>();
    __shared__ float s_e[4][COVA_GAT_MAX_K];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, n = blockIdx.x * 4 + w;
    if (n >= N) return;
    float *se = s_e[w];
    float wi[NC][V], a[NC][V];
    int off[NC];
    bool in[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        off[c] = (64 * c + lane) * V;
        in[c] = off[c] < D;                                    // (V = 4: D % 4 == 0, the whole vector is inside)
#pragma unroll
        for (int v = 0; v < V; ++v) wi[c][v] = a[c][v] = 0.f;
        if (in[c]) {
            ldv<V>(Wh + (size_t)n * ldw + off[c], wi[c]);
            ldv<V>(att_w + off[c], a[c]);
        }
    }
    const float b = att_b[0];
    float m = -INFINITY;
    for (int p0 = 0; p0 < K; p0 += 64) {                       // scores: slot p0 + q ends in lane q
        const int cnt = min(64, K - p0);
        const int jj = lane < cnt ? gat_slot_id(ctx, (size_t)n * K + p0 + lane, N) : -1;
        float e = lane < cnt ? -9e15f : -INFINITY;             // pads keep the mask value (models.py:202-203)
        for (int q0 = 0; q0 < cnt; q0 += U) {
            int jk[U];
            float wj[U][NC][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jq = __shfl(jj, min(q0 + u, 63), 64);
                jk[u] = q0 + u < cnt ? jq : -1;
                if (jk[u] >= 0) {                              // (wave-uniform)
                    const float *row = Wh + (size_t)jk[u] * ldw + D;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (in[c]) ldv<V>(row + off[c], wj[u][c]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (jk[u] < 0) continue;
                float part = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (!in[c]) continue;
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const float z = wi[c][v] + wj[u][c][v];
                        const float lr = z > 0.f ? z : slope * z;
                        part = fmaf(a[c][v], lr, part);
                    }
                }
                float sc = wave_sum(part) + b;
                if (EDGE) sc += gat_edge_term(phi, (size_t)n * K + p0 + q0 + u, edge_w);
                if (lane == q0 + u) e = sc;
            }
        }
        se[p0 + lane] = e;
        m = fmaxf(m, e);
    }
    m = wave_max(m);
    float psum = 0.f;
    for (int p0 = 0; p0 < K; p0 += 64) {
        const float pr = p0 + lane < K ? expf(se[p0 + lane] - m) : 0.f;
        se[p0 + lane] = pr;
        psum += pr;
    }
    const float denom = wave_sum(psum);
    float acc[NC][V];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[c][v] = 0.f;
    for (int p0 = 0; p0 < K; p0 += 64) {                       // aggregation, neighbours added in slot order
        const int cnt = min(64, K - p0);
        int jj = -1;
        float aw = 0.f;
        if (lane < cnt) {
            jj = gat_slot_id(ctx, (size_t)n * K + p0 + lane, N);
            const float alpha = se[p0 + lane] / denom;
            attn[(size_t)n * K + p0 + lane] = alpha;
            aw = jj >= 0 ? alpha : 0.f;                        // pads: no weight, no row read
            if (DROP && jj >= 0) aw = gat_dropped(dr, (size_t)n * K + p0 + lane, alpha);   // (dropped slots: no row read)
        }
        for (int q0 = 0; q0 < cnt; q0 += U) {
            float au[U], wj[U][NC][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int qq = min(q0 + u, 63);
                const int jq = __shfl(jj, qq, 64);
                const float aq = __shfl(aw, qq, 64);
                au[u] = q0 + u < cnt && jq >= 0 ? aq : 0.f;
                if (au[u] != 0.f) {                            // (wave-uniform)
                    const float *row = Wh + (size_t)jq * ldw + D;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (in[c]) ldv<V>(row + off[c], wj[u][c]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (au[u] == 0.f) continue;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (!in[c]) continue;
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[c][v] = fmaf(au[u], wj[u][c][v], acc[c][v]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (in[c]) stv<V>(hprime + (size_t)n * ldh + off[c], acc[c]);
}

// ------------------------------------------------------------------------------------------------ backward, source side
// One wave per node i: dattn[k] = g_i . Wh_j, du = attn * (dattn - sum attn * dattn) (pads exactly 0) -> du [N,K];
// dWh[i, d] = a[d] * sum_k du[k] * gate(z[i,k,d]); and the node's terms of the parameter gradients:
// sum_k du[k] * lrelu(z[i,k,d]) (d_att_w), sum_k du[k] (d_att_b), sum_k du[k] * phi[i,k,:] (d_edge_w).  The four nodes of a
// block are added in wave order and written as row blockIdx.x of the workspace: [0,D) d_att_w, D d_att_b, D+1 .. D+8
// d_edge_w (row length P = D + 9); gat2_fold_kernel adds the rows.
template <int NC, int V, bool EDGE, bool DROP = false>
__global__ __launch_bounds__(256) void gat2_bwd_src_kernel(
    const float *__restrict__ g, int ldg, const float *__restrict__ Wh, int ldw, const float *__restrict__ attn,
    const int64_t *__restrict__ ctx, const float *__restrict__ att_w, const float *__restrict__ phi, int N, int K, int D,
    float slope, float *__restrict__ dWh, int lddw, float *__restrict__ du_out, float *__restrict__ ws,
    GatDrop dr = GatDrop{})
{
    constexpr int U = gat2_unroll<NC, V>();
    constexpr int ROW = NC * V * 64;                           // channels a wave covers
    __shared__ float s_k[4][COVA_GAT_MAX_K];
    __shared__ float s_x[3][ROW + 16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, n = blockIdx.x * 4 + w;
    int off[NC];
    bool in[NC];
    float accl[NC][V];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        off[c] = (64 * c + lane) * V;
        in[c] = off[c] < D;
#pragma unroll
        for (int v = 0; v < V; ++v) accl[c][v] = 0.f;
    }
    float sc[9];                                               // sum du, sum du * phi[0:8]: the wave's totals
#pragma unroll
    for (int f = 0; f < 9; ++f) sc[f] = 0.f;
    if (n < N) {                                               // (wave-uniform; the waves past N add zeros below)
        float *sk = s_k[w];
        float gi[NC][V], wi[NC][V], a[NC][V], accg[NC][V];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int v = 0; v < V; ++v) gi[c][v] = wi[c][v] = a[c][v] = accg[c][v] = 0.f;
            if (in[c]) {
                ldv<V>(g + (size_t)n * ldg + off[c], gi[c]);
                ldv<V>(Wh + (size_t)n * ldw + off[c], wi[c]);
                ldv<V>(att_w + off[c], a[c]);
            }
        }
        float ad = 0.f;
        for (int p0 = 0; p0 < K; p0 += 64) {                   // dattn of slot p0 + q ends in lane q
            const int cnt = min(64, K - p0);
            int jj = -1;
            float alpha = 0.f, dalpha = 0.f;
            if (lane < cnt) {
                jj = gat_slot_id(ctx, (size_t)n * K + p0 + lane, N);
                alpha = attn[(size_t)n * K + p0 + lane];
            }
            for (int q0 = 0; q0 < cnt; q0 += U) {
                int jk[U];
                float wj[U][NC][V];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int jq = __shfl(jj, min(q0 + u, 63), 64);
                    jk[u] = q0 + u < cnt ? jq : -1;
                    if (jk[u] >= 0) {
                        const float *row = Wh + (size_t)jk[u] * ldw + D;
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            if (in[c]) ldv<V>(row + off[c], wj[u][c]);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (jk[u] < 0) continue;
                    float part = 0.f;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (!in[c]) continue;
#pragma unroll
                        for (int v = 0; v < V; ++v) part = fmaf(gi[c][v], wj[u][c][v], part);
                    }
                    const float tot = wave_sum(part);
                    if (lane == q0 + u) dalpha = tot;
                }
            }
            if (DROP && jj >= 0) dalpha = gat_dropped(dr, (size_t)n * K + p0 + lane, dalpha);
            sk[p0 + lane] = dalpha;
            float prod = alpha * dalpha;
            ad += prod;
        }
        const float dot = wave_sum(ad);
        float dus = 0.f, dphi[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) dphi[f] = 0.f;
        for (int p0 = 0; p0 < K; p0 += 64) {                   // du, then the gated sums over the slots in slot order
            const int cnt = min(64, K - p0);
            int jj = -1;
            float du = 0.f;
            if (lane < cnt) {
                jj = gat_slot_id(ctx, (size_t)n * K + p0 + lane, N);
                if (jj >= 0) du = attn[(size_t)n * K + p0 + lane] * (sk[p0 + lane] - dot);
                du_out[(size_t)n * K + p0 + lane] = du;
                dus += du;
                if (EDGE && jj >= 0) {
                    const size_t slot = (size_t)n * K + p0 + lane;
                    const float4 f0 = *reinterpret_cast<const float4 *>(phi + slot * 8);
                    const float4 f1 = *reinterpret_cast<const float4 *>(phi + slot * 8 + 4);
                    dphi[0] = fmaf(du, f0.x, dphi[0]); dphi[1] = fmaf(du, f0.y, dphi[1]);
                    dphi[2] = fmaf(du, f0.z, dphi[2]); dphi[3] = fmaf(du, f0.w, dphi[3]);
                    dphi[4] = fmaf(du, f1.x, dphi[4]); dphi[5] = fmaf(du, f1.y, dphi[5]);
                    dphi[6] = fmaf(du, f1.z, dphi[6]); dphi[7] = fmaf(du, f1.w, dphi[7]);
                }
            }
            for (int q0 = 0; q0 < cnt; q0 += U) {
                int jk[U];
                float dk[U], wj[U][NC][V];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int qq = min(q0 + u, 63);
                    const int jq = __shfl(jj, qq, 64);
                    dk[u] = __shfl(du, qq, 64);
                    jk[u] = q0 + u < cnt ? jq : -1;
                    if (jk[u] >= 0) {
                        const float *row = Wh + (size_t)jk[u] * ldw + D;
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            if (in[c]) ldv<V>(row + off[c], wj[u][c]);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (jk[u] < 0) continue;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (!in[c]) continue;
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const float z = wi[c][v] + wj[u][c][v];          // (the forward's z, bit for bit)
                            const bool pos = z > 0.f;
                            accg[c][v] = fmaf(dk[u], pos ? 1.f : slope, accg[c][v]);
                            accl[c][v] = fmaf(dk[u], pos ? z : slope * z, accl[c][v]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (!in[c]) continue;
            float o[V];
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = a[c][v] * accg[c][v];
            stv<V>(dWh + (size_t)n * lddw + off[c], o);
        }
        sc[0] = wave_sum(dus);
        if (EDGE) {
#pragma unroll
            for (int f = 0; f < 8; ++f) sc[1 + f] = wave_sum(dphi[f]);
        }
    }
    // the block's four nodes, added in wave order
    if (w > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int v = 0; v < V; ++v) s_x[w - 1][off[c] + v] = accl[c][v];
#pragma unroll
        for (int f = 0; f < 9; ++f)
            if (lane == f) s_x[w - 1][ROW + f] = sc[f];
    }
    __syncthreads();
    if (w == 0) {
        float *out = ws + (size_t)blockIdx.x * (D + 9);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (!in[c]) continue;
#pragma unroll
            for (int v = 0; v < V; ++v)
                out[off[c] + v] = ((accl[c][v] + s_x[0][off[c] + v]) + s_x[1][off[c] + v]) + s_x[2][off[c] + v];
        }
#pragma unroll
        for (int f = 0; f < 9; ++f)
            if (lane == f) out[D + f] = ((sc[f] + s_x[0][ROW + f]) + s_x[1][ROW + f]) + s_x[2][ROW + f];
    }
}

// ------------------------------------------------------------------------------------------------ backward, destination side
// One wave per node j over row j of the transposed index (flat slots e = i*K + k naming j, ascending):
// dWh[j, D+d] = sum_e ( attn[e] * g[i_e, d] + du[e] * a[d] * gate(Wh[i_e, d] + Wh[j, D+d]) ); in-degree 0 writes zeros.
template <int NC, int V, bool DROP = false>
__global__ __launch_bounds__(256) void gat2_bwd_dst_kernel(
    const float *__restrict__ g, int ldg, const float *__restrict__ Wh, int ldw, const float *__restrict__ attn,
    const float *__restrict__ du, const int *__restrict__ row_ptr, const int *__restrict__ edges,
    const float *__restrict__ att_w, int N, int K, int D, float slope, float *__restrict__ dWh, int lddw,
    GatDrop dr = GatDrop{})
{
    constexpr int U = gat2_unroll<NC, V>();
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    const int lo = row_ptr[j], deg = row_ptr[j + 1] - lo;
    float wj[NC][V], a[NC][V], acc[NC][V];
    int off[NC];
    bool in[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        off[c] = (64 * c + lane) * V;
        in[c] = off[c] < D;
#pragma unroll
        for (int v = 0; v < V; ++v) wj[c][v] = a[c][v] = acc[c][v] = 0.f;
        if (in[c]) {
            ldv<V>(Wh + (size_t)j * ldw + D + off[c], wj[c]);
            ldv<V>(att_w + off[c], a[c]);
        }
    }
    for (int c0 = 0; c0 < deg; c0 += 64) {
        const int cnt = min(64, deg - c0);
        const int e = lane < cnt ? edges[lo + c0 + lane] : 0;
        float al = lane < cnt ? attn[e] : 0.f;
        if (DROP && lane < cnt) al = gat_dropped(dr, (size_t)e, al);
        const float de = lane < cnt ? du[e] : 0.f;
        for (int q0 = 0; q0 < cnt; q0 += U) {
            bool on[U];
            float aq[U], dq[U], gv[U][NC][V], wv[U][NC][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int qq = min(q0 + u, 63);
                const int i = __shfl(e, qq, 64) / K;
                aq[u] = __shfl(al, qq, 64);
                dq[u] = __shfl(de, qq, 64);
                on[u] = q0 + u < cnt;
                if (on[u]) {                                   // (wave-uniform)
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (!in[c]) continue;
                        ldv<V>(g + (size_t)i * ldg + off[c], gv[u][c]);
                        ldv<V>(Wh + (size_t)i * ldw + off[c], wv[u][c]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!on[u]) continue;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (!in[c]) continue;
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const float z = wv[u][c][v] + wj[c][v];              // (the forward's z, bit for bit)
                        const float t = dq[u] * (z > 0.f ? 1.f : slope);
                        acc[c][v] = fmaf(aq[u], gv[u][c][v], acc[c][v]);
                        acc[c][v] = fmaf(t, a[c][v], acc[c][v]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (in[c]) stv<V>(dWh + (size_t)j * lddw + D + off[c], acc[c]);
}

// ------------------------------------------------------------------------------------------------ parameter gradients
// Column col of the nb workspace rows (row length P), added in a fixed order: a block owns 64 columns, slice q of its 16
// takes rows q, q + 16, ... ascending, the slices are added in slice order.  cols [0,D) -> d_att_w, D -> d_att_b,
// D+1 .. D+8 -> d_edge_w (only when ncols covers them).  The bits depend on (N, D) and the data alone.
__global__ __launch_bounds__(1024) void gat2_fold_kernel(const float *__restrict__ ws, int nb, int P, int D, int ncols,
                                                         float *__restrict__ d_att_w, float *__restrict__ d_att_b,
                                                         float *__restrict__ d_edge_w)
{
    __shared__ float s_acc[16][64];
    const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + tx;
    float acc = 0.f;
    if (col < ncols)
        for (int r = q; r < nb; r += 16) acc += ws[(size_t)r * P + col];
    s_acc[q][tx] = acc;
    __syncthreads();
    if (q == 0 && col < ncols) {
        float t = 0.f;
        for (int s = 0; s < 16; ++s) t += s_acc[s][tx];
        if (col < D) d_att_w[col] = t;
        else if (col == D) d_att_b[0] = t;
        else d_edge_w[col - D - 1] = t;
    }
}

// chunks per row the kernels are instantiated for: 1, 2, 4, 8 (and 16 in the scalar form); 0 = D too large
inline int gat2_chunks(int D, int V)
{
    const int nc = cdiv(D, 64 * V);
    if (nc <= 1) return 1;
    if (nc <= 2) return 2;
    if (nc <= 4) return 4;
    if (nc <= 8) return 8;
    return V == 1 && nc <= 16 ? 16 : 0;
}

}  // namespace

// largest D: 2048 in the float4 form, 1024 in the scalar form
#define COVA_GAT2_DISPATCH(V4_, NC_, LAUNCH)                                                                        \
    do {                                                                                                            \
        if (V4_) {                                                                                                  \
            switch (NC_) {                                                                                          \
            case 1: LAUNCH(1, 4); break;                                                                            \
            case 2: LAUNCH(2, 4); break;                                                                            \
            case 4: LAUNCH(4, 4); break;                                                                            \
            default: LAUNCH(8, 4); break;                                                                           \
            }                                                                                                       \
        } else {                                                                                                    \
            switch (NC_) {                                                                                          \
            case 1: LAUNCH(1, 1); break;                                                                            \
            case 2: LAUNCH(2, 1); break;                                                                            \
            case 4: LAUNCH(4, 1); break;                                                                            \
            case 8: LAUNCH(8, 1); break;                                                                            \
            default: LAUNCH(16, 1); break;                                                                          \
            }                                                                                                       \
        }                                                                                                           \
    } while (0)

namespace {
template <bool DROP>
int gat2_fwd_launch(const float *Wh, int ldw, const float *att_w, const float *att_b, const int64_t *ctx,
                    const float *phi, const float *edge_w, int N, int K, int D, float slope, float *attn,
                    float *hprime, int ldh, void *stream, GatDrop dr = GatDrop{})
{
    COVA_REQUIRE(N >= 0 && K > 0 && K <= COVA_GAT_MAX_K && D > 0 && ldw >= 2 * D && ldh >= D);
    COVA_REQUIRE((phi == nullptr) == (edge_w == nullptr) && (phi == nullptr || aligned16(phi)));
    if (N == 0) return COVA_OK;
    COVA_REQUIRE(Wh && att_w && att_b && ctx && attn && hprime);
    const bool v4 = D % 4 == 0 && ldw % 4 == 0 && ldh % 4 == 0 && aligned16(Wh) && aligned16(att_w) && aligned16(hprime);
    const int nc = gat2_chunks(D, v4 ? 4 : 1);
    COVA_REQUIRE(nc > 0);
    const dim3 grid(cdiv(N, 4)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define COVA_GAT2_FWD(NC, V)                                                                                  \
    do {                                                                                                      \
        if (phi) COVA_LAUNCH((gat2_fwd_kernel<NC, V, true, DROP>), grid, blk, st, Wh, ldw, att_w, att_b, ctx, \
                             phi, edge_w, N, K, D, slope, attn, hprime, ldh, dr);                             \
        else COVA_LAUNCH((gat2_fwd_kernel<NC, V, false, DROP>), grid, blk, st, Wh, ldw, att_w, att_b, ctx,    \
                         phi, edge_w, N, K, D, slope, attn, hprime, ldh, dr);                                 \
    } while (0)
    COVA_GAT2_DISPATCH(v4, nc, COVA_GAT2_FWD);
#undef COVA_GAT2_FWD
    COVA_LAUNCH_CHECK();
    return COVA_OK;
}
}  // namespace

COVA_API int cova_gat2_fwd(const float *Wh, int ldw, const float *att_w, const float *att_b, const int64_t *ctx,
                           const float *phi, const float *edge_w, int N, int K, int D, float slope, float *attn,
                           float *hprime, int ldh, void *stream)
{
    return gat2_fwd_launch<false>(Wh, ldw, att_w, att_b, ctx, phi, edge_w, N, K, D, slope, attn, hprime, ldh, stream);
}

// cova_gat2_fwd with attention dropout: slot e = i*K + k is kept when hash_uniform(seed, e) >= p and
// then weighs attn * 1/(1-p) in h'; attn stays the softmax output.  p in [0, 1).
COVA_API int cova_gat2_fwd_drop(const float *Wh, int ldw, const float *att_w, const float *att_b, const int64_t *ctx,
                                const float *phi, const float *edge_w, int N, int K, int D, float slope, float p,
                                unsigned long long seed, float *attn, float *hprime, int ldh, void *stream)
{
    COVA_REQUIRE(p >= 0.f && p < 1.f);                         // (NaN fails both)
    return gat2_fwd_launch<true>(Wh, ldw, att_w, att_b, ctx, phi, edge_w, N, K, D, slope, attn, hprime, ldh, stream,
                                 gat_drop_of(p, seed));
}

// floats of cova_gat2_bwd's workspace: one row of D + 9 partial sums per block of four nodes
COVA_API int cova_gat2_workspace_floats(int N, int K, int D)
{
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    const long long n = (long long)cdiv(N, 4) * (D + 9);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

namespace {
template <bool DROP>
int gat2_bwd_launch(const float *g, int ldg, const float *Wh, int ldw, const float *attn, const int64_t *ctx,
                    const float *att_w, const float *phi, const float *edge_w, int N, int K, int D, float slope,
                    float *dWh, int lddw, float *d_att_w, float *d_att_b, float *d_edge_w, const int *csr,
                    float *du, float *workspace, void *stream, GatDrop dr = GatDrop{})
{
    COVA_REQUIRE(N >= 0 && K > 0 && K <= COVA_GAT_MAX_K && D > 0 && ldg >= D && ldw >= 2 * D && lddw >= 2 * D);
    COVA_REQUIRE((phi == nullptr) == (edge_w == nullptr) && (phi == nullptr) == (d_edge_w == nullptr) &&
                 (phi == nullptr || aligned16(phi)));
    if (N == 0) return COVA_OK;
    COVA_REQUIRE(g && Wh && attn && ctx && att_w && dWh && d_att_w && d_att_b && csr && du && workspace);
    COVA_REQUIRE(cova_gat2_workspace_floats(N, K, D) > 0);
    const bool v4 = D % 4 == 0 && ldg % 4 == 0 && ldw % 4 == 0 && lddw % 4 == 0 && aligned16(g) && aligned16(Wh) &&
                    aligned16(att_w) && aligned16(dWh);
    const int nc = gat2_chunks(D, v4 ? 4 : 1);
    COVA_REQUIRE(nc > 0);
    const dim3 grid(cdiv(N, 4)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define COVA_GAT2_BWD(NC, V)                                                                                 \
    do {                                                                                                     \
        if (phi) COVA_LAUNCH((gat2_bwd_src_kernel<NC, V, true, DROP>), grid, blk, st, g, ldg, Wh, ldw, attn, \
                             ctx, att_w, phi, N, K, D, slope, dWh, lddw, du, workspace, dr);                 \
        else COVA_LAUNCH((gat2_bwd_src_kernel<NC, V, false, DROP>), grid, blk, st, g, ldg, Wh, ldw, attn,    \
                         ctx, att_w, phi, N, K, D, slope, dWh, lddw, du, workspace, dr);                     \
        COVA_LAUNCH((gat2_bwd_dst_kernel<NC, V, DROP>), grid, blk, st, g, ldg, Wh, ldw, attn, du, csr,       \
                    csr + N + 1, att_w, N, K, D, slope, dWh, lddw, dr);                                      \
    } while (0)
    COVA_GAT2_DISPATCH(v4, nc, COVA_GAT2_BWD);
#undef COVA_GAT2_BWD
    COVA_LAUNCH_CHECK();
    const int ncols = D + 1 + (phi ? 8 : 0);
    COVA_LAUNCH(gat2_fold_kernel, dim3(cdiv(ncols, 64)), dim3(1024), st, workspace, cdiv(N, 4), D + 9, D, ncols,
                d_att_w, d_att_b, d_edge_w);
    return COVA_OK;
}
}  // namespace

COVA_API int cova_gat2_bwd(const float *g, int ldg, const float *Wh, int ldw, const float *attn, const int64_t *ctx,
                           const float *att_w, const float *phi, const float *edge_w, int N, int K, int D, float slope,
                           float *dWh, int lddw, float *d_att_w, float *d_att_b, float *d_edge_w, const int *csr,
                           float *du, float *workspace, void *stream)
{
    return gat2_bwd_launch<false>(g, ldg, Wh, ldw, attn, ctx, att_w, phi, edge_w, N, K, D, slope, dWh, lddw, d_att_w,
                                  d_att_b, d_edge_w, csr, du, workspace, stream);
}

// cova_gat2_bwd behind cova_gat2_fwd_drop: the same (p, seed) regenerate the mask on both sides
COVA_API int cova_gat2_bwd_drop(const float *g, int ldg, const float *Wh, int ldw, const float *attn, const int64_t *ctx,
                                const float *att_w, const float *phi, const float *edge_w, int N, int K, int D,
                                float slope, float p, unsigned long long seed, float *dWh, int lddw, float *d_att_w,
                                float *d_att_b, float *d_edge_w, const int *csr, float *du, float *workspace,
                                void *stream)
{
    COVA_REQUIRE(p >= 0.f && p < 1.f);
    return gat2_bwd_launch<true>(g, ldg, Wh, ldw, attn, ctx, att_w, phi, edge_w, N, K, D, slope, dWh, lddw, d_att_w,
                                 d_att_b, d_edge_w, csr, du, workspace, stream, gat_drop_of(p, seed));
}
