// Page self-attention: every box attends to all boxes of its page, per head a of dh = E / Hh columns,
//   s_ij = (Q_i . K_j) * rs,  rs = 1 / sqrt(dh),  A_ij = softmax_j s_ij over ALL rows j of the page,  O_i = sum_j A_ij V_j,
// and its hand-written backward.  [Q | K | V] are the columns [0, E), [E, 2E), [2E, 3E) of the dense qkv rows.  Pages come
// from page_rows() (rows.h: both ends clamped into [0, N]); an empty page writes nothing.
//
// Both products of every kernel run on the f32 matrix pipe (mfma16x4, mma.h).  One tile shape serves all three kernels:
// a block of four waves owns 64 OWN rows of one (page, head), a wave 16 of them, held in registers as the B operand; it
// walks the OTHER rows of the page in ascending tiles of KT rows (64; 32 when dh > 96) staged in LDS as the A operand.
//   forward, backward query side   own = queries (Q_i, g_i),  other = keys (K, V tiles)
//   backward key side              own = keys (K_j, V_j),     other = queries (Q, g tiles, their lse and delta)
// Lane l = 16 grp + l16 of a wave holds, of its own row l16, the dims 16 c + 4 grp + r (c < ceil(dh / 16), r < 4).  A 16 x 16
// score tile S^T[other][own] is up to four short chains of MFMAs per wave; lane l receives the other rows 4 grp + r of the
// sub-tile for its own row l16, which is exactly the B operand of the second product, so nothing is transposed or exchanged.
//
// The forward is TWO PASSES over the key tiles: pass 1 the row maximum m_i, pass 2 p_ij = expf(s_ij - m_i), their sum l_i and
// sum_j p_ij V_j; O_i = (sum_j p_ij V_j) / l_i and lse_i = m_i + logf(l_i).  No probability is stored; the backward recomputes
// A_ij = expf(s_ij - lse_i).  LDS holds two tiles whatever the page's length: a page of any size runs.
//
// Summation orders (all f32, every one a function of the page's own row count, E and Hh alone; no atomics, no host read):
//   Q_i . K_j, g_i . V_j   NA = min(ceil(dh / 16), 4) independent MFMA chains from +0: chain t takes the blocks c = t, t + NA,
//                          ... in turn, r ascending inside a block; inside an MFMA the four k slots grp = 0..3 (dims 16 c + r,
//                          16 c + 4 + r, 16 c + 8 + r, 16 c + 12 + r) as the pipe's own fma chain; the chains are added as
//                          (t0 + t1) + (t2 + t3); then ONE rounded multiply by rs.  (Independent chains issue back to back
//                          where one chain waits out the pipe's latency, and partial sums a quarter as long round less.)
//   m_i                    f32 compares per lane over its other rows, then fmaxf over lanes xor 16, xor 32 (a maximum: exact)
//   l_i                    lane (l16, grp) adds its p in turn (tiles ascending, sub-tiles of 16 ascending, r ascending: other
//                          rows 16 sub + 4 grp + r), then (l_grp + l_grp^1) + (l_grp^2 + l_grp^3) by shuffles xor 16, xor 32
//   sum_j p_ij V_j, dQ_i, dK_j, dV_j   per output dim one MFMA chain from +0: tiles ascending, sub-tiles ascending, r
//                          ascending, the k slots grp = 0..3 (other rows 16 sub + 4 grp + r) inside an MFMA; dQ and dK then
//                          ONE rounded multiply by rs
//   delta_i = g_i . O_i    part_j (j < 4) = fma chain from +0 over the dims 16 c + 4 j + r (c, then r ascending), then
//                          (part_0 + part_1) + (part_2 + part_3) by shuffles (pa_delta_part: both sides call it)
// A row's own tile-mates never enter its sums, so O, lse and dqkv rows keep their bits whatever other pages share the batch,
// and reruns are bit-identical.
//
// The GEO instantiations (cova_page_attn_fwd_geo / cova_page_attn_bwd_geo) add a relative-geometry
// bias to every score, formed on the fly from the two boxes of the pair, per head a with eight weights w[a][0..7]:
//   phi_ij = edge_features(box of the QUERY i, box of the KEY j, W, H, dj = j - i)    geometry.h: cova_edge_geometry's bits
//   b_ij   = fma chain from +0 over e = 0..7 of w[a][e] * phi_ij[e]
//   s_ij   = (Q_i . K_j) * rs + b_ij                  one rounded multiply, then one rounded add
// A lane keeps the box of its own row in four registers; the boxes of the staged other rows lie in LDS beside the tile
// (KT x 4 floats, staged in the same phase); the head's eight weights are block-uniform.  On the key side own = key and
// other = query, and the call is still edge_features(query box, key box, key index - query index): five of the eight
// features are antisymmetric.  Everything GEO sits behind `if constexpr`: the plain instantiations are what they were.
//   d w[a][e] = sum over pages, i, j of ds_ij * phi_ij[e], on the QUERY side:
//     lane (l16, grp)   eight partials, fmaf(ds, phi[e], partial) in turn: tiles ascending, sub-tiles ascending, r
//                       ascending (own row l16, other rows 16 sub + 4 grp + r); a masked pair enters with ds = +0
//     wave              v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1
//     block             ((w0 + w1) + w2) + w3 over its four waves through LDS, written to workspace[block][e]; a block whose
//                       own tile lies behind its page's end writes eight zeros
//     fold launch       per (a, e) one thread, from +0: pages ascending, inside a page its own tiles ascending (the blocks
//                       behind the page's end hold zeros and are passed over: the sum's bits are the same)
// No atomics, no host read: d w is bit-identical between reruns.  phi has no gradient (the boxes are data).
//
// The DROP instantiations (cova_page_attn_fwd_drop / cova_page_attn_bwd_drop and their _geo_ forms)
// drop attention probabilities, torch's inverted dropout on A: rate p, inv = 1.f / (1.f - p), stream seed.  No mask is
// stored.  The score of (query batch row i, head a, key batch row j) is kept when
//   hash_uniform(seed, ((uint64)(i * Hh + a) << 32) | (uint64)j) >= p          (f32 compare; N * Hh < 2**32)
// and all three kernels form that index from the same integers and call pa_dropped(): ONE rounded multiply v * inv on a
// kept score, 0.f on a dropped one.  What DROP adds, every sum in its order above:
//   forward, pass 2        l_i += p_ij as before (pass 1, m_i, l_i and lse_i keep the plain forward's bits); the V product
//                          takes pa_dropped(p_ij): O_i = (sum_j D_ij inv p_ij V_j) / l_i
//   both backward sides    dA_ij = pa_dropped(g_i . V_j) (the rounded product of the plain form, then the helper);
//                          ds_ij = A_ij * (dA_ij - delta_i) with the undropped A_ij: a dropped score still takes
//                          -A_ij delta_i through the softmax; delta_i = g_i . O_i holds with the dropped O
//   key side               dV_j takes pa_dropped(A_ij)
// A dropped score enters its sums as +0.  A row whose keys are all dropped has O = 0, delta = 0 and zero dqkv rows.
// Everything DROP sits behind `if constexpr`: the other instantiations are what they were.
#include "geometry.h"
#include "mma.h"
#include "rows.h"

// the orders above count one rounding per written operation: only the fmaf calls and the MFMAs fuse
#pragma clang fp contract(off)

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_OWN = 64;                 // own rows of a block: 16 per wave
constexpr int PA_MAX_E = 512;
constexpr int PA_MAX_DH = 128;

template <int DHB>                         // DHB = blocks of 16 head dims the kernel is built for (1, 2, 4, 6, 8): dh <= 16 DHB
struct PaCfg {
    static constexpr int DHP = 16 * DHB;   // staged width: dims dh .. DHP - 1 hold zeros
    static constexpr int LD = DHP + 4;     // LDS row stride in floats: 16-byte rows; a score read's sixteen rows and an
                                           // accumulate read's four row groups fall on distinct banks
    static constexpr int KT = DHB == 8 ? 32 : 64;      // other rows per staged tile: two tiles stay below 52 KB
};

__device__ __forceinline__ f32x4 pa_ld4(const float *__restrict__ p, bool vec)
{
    if (vec) return *reinterpret_cast<const f32x4 *>(p);
    return f32x4{p[0], p[1], p[2], p[3]};
}

__device__ __forceinline__ void pa_st4(float *__restrict__ p, f32x4 v, bool vec)
{
    if (vec) {
        *reinterpret_cast<f32x4 *>(p) = v;
    } else {
        p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
    }
}

// this lane's fragment of its own row's head slice `row` (nullptr: an absent row, zeros): dims 16 c + 4 grp + r
template <int DHB>
__device__ __forceinline__ void pa_frag(const float *__restrict__ row, int dh, int grp, bool vec, f32x4 (&f)[DHB])
{
#pragma unroll
    for (int c = 0; c < DHB; ++c) {
        const int d = 16 * c + 4 * grp;
        f[c] = (row != nullptr && d < dh) ? pa_ld4(row + d, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// rows [0, KT) x dims [0, DHP) of a tile into LDS; rows >= rows_valid and dims >= dh are zeros.  src = head slice of row 0.
template <int DHB>
__device__ __forceinline__ void pa_stage(float *__restrict__ lds, const float *__restrict__ src, size_t ld, int rows_valid,
                                         int dh, bool vec, int tid)
{
    using C = PaCfg<DHB>;
    constexpr int C4 = C::DHP / 4;
    for (int idx = tid; idx < C::KT * C4; idx += PA_THREADS) {
        const int row = idx / C4, c = (idx - row * C4) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < rows_valid && c < dh) v = pa_ld4(src + (size_t)row * ld + c, vec);
        *reinterpret_cast<f32x4 *>(lds + row * C::LD + c) = v;
    }
}

// S^T[other 16 sub + 4 grp + r'][own l16] = X_other . x_own over the head dims, register r' of the result
template <int DHB>
__device__ __forceinline__ f32x4 pa_dot(const float *__restrict__ lds, int sub, const f32x4 (&f)[DHB], int l16, int grp)
{
    using C = PaCfg<DHB>;
    constexpr int NA = DHB < 4 ? DHB : 4;
    const float *row = lds + (sub * 16 + l16) * C::LD + 4 * grp;
    f32x4 acc[NA];
#pragma unroll
    for (int t = 0; t < NA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DHB; ++c) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(row + 16 * c);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[c % NA] = mfma16x4(a[r], f[c][r], acc[c % NA]);
    }
    if constexpr (NA == 1) return acc[0];
    else if constexpr (NA == 2) return acc[0] + acc[1];
    else return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// acc[db][r'] (dim 16 db + 4 grp + r' of own row l16) += sum over the sub-tile's other rows of X_other[dim] * w
template <int DHB>
__device__ __forceinline__ void pa_acc(const float *__restrict__ lds, int sub, f32x4 w, f32x4 (&acc)[DHB], int l16, int grp)
{
    using C = PaCfg<DHB>;
    const float *base = lds + (sub * 16 + 4 * grp) * C::LD + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int db = 0; db < DHB; ++db) acc[db] = mfma16x4(base[r * C::LD + 16 * db], w[r], acc[db]);
}

// quarter j of g_i . O_i over one head slice: the dims 16 c + 4 j + r, c then r ascending, one fma chain
__device__ __forceinline__ float pa_delta_part(const float *__restrict__ g, const float *__restrict__ o, int dh, int j,
                                               bool vg, bool vo)
{
    float d = 0.f;
    for (int c = 4 * j; c < dh; c += 16) {
        const f32x4 a = pa_ld4(g + c, vg), b = pa_ld4(o + c, vo);
#pragma unroll
        for (int r = 0; r < 4; ++r) d = fmaf(a[r], b[r], d);
    }
    return d;
}

// a value per grp of the same l16 -> (v_grp + v_grp^1) + (v_grp^2 + v_grp^3): the same bits in all four lanes
__device__ __forceinline__ float pa_grp_sum(float v)
{
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

struct PaBlock {
    int own_tile, head, base, n;
};

// block -> (page, head, tile of own rows); n == 0 where the block has nothing to do (block-uniform)
__device__ __forceinline__ PaBlock pa_block(const int64_t *__restrict__ page_start, int N, int Hh, int tiles)
{
    const int bid = blockIdx.x;
    const int t = bid % tiles, a = (bid / tiles) % Hh, p = bid / (tiles * Hh);
    const PageRows pr = page_rows(page_start, p, N);
    const int n = pr.end - pr.base;
    return PaBlock{t, a, pr.base, t * PA_OWN < n ? n : 0};
}

// operands of the geometry bias; the plain instantiations carry the empty form
template <bool GEO>
struct PaGeo {};

template <>
struct PaGeo<true> {
    const float *bboxes;                   // [N, 5] = page, x1, y1, x2, y2
    const float *w;                        // [Hh, 8]
    float W, H;                            // page width and height in pixels
    float *ws;                             // query side of the backward: [blocks][8] partial sums of d w
};

// the boxes of a tile's rows [0, KT) into LDS; rows >= rows_valid are zeros.  row0 = batch row of the tile's row 0.
template <int DHB>
__device__ __forceinline__ void pa_stage_boxes(float4 *__restrict__ lds, const float *__restrict__ bboxes, int row0,
                                               int rows_valid, int tid)
{
    if (tid < PaCfg<DHB>::KT)
        lds[tid] = tid < rows_valid ? knn_box(bboxes, (long long)row0 + tid) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void pa_geo_weights(const float *__restrict__ w, int head, float (&wt)[8])
{
#pragma unroll
    for (int e = 0; e < 8; ++e) wt[e] = w[head * 8 + e];
}

// phi of (query box, key box, dj = key index - query index) and the bias w . phi as one fma chain from +0
__device__ __forceinline__ float pa_bias(const float4 qbox, const float4 kbox, float W, float H, int dj, const float (&wt)[8],
                                         float (&phi)[8])
{
    edge_features(qbox, kbox, W, H, dj, phi);
    float b = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) b = fmaf(wt[e], phi[e], b);
    return b;
}

// operands of the attention dropout; the other instantiations carry the empty form
template <bool DROP>
struct PaDrop {};

template <>
struct PaDrop<true> {
    float p, inv;                          // rate, 1.f / (1.f - p)
    unsigned long long seed;
};

// the mask word of (query batch row i, head a, key batch row j): the three kernels call this with the same integers
__device__ __forceinline__ unsigned long long pa_drop_idx(int i, int Hh, int a, int j)
{
    return ((unsigned long long)((unsigned)i * (unsigned)Hh + (unsigned)a) << 32) | (unsigned long long)(unsigned)j;
}

// v * inv on a kept score, 0 on a dropped one: ONE rounded f32 multiply (never contracted into a neighbouring add), so the
// forward and both sides of the backward form the same dropped value bit for bit (common.h: gat_dropped's statement)
__device__ __forceinline__ float pa_dropped(const PaDrop<true> &dr, unsigned long long idx, float v)
{
    return hash_uniform(dr.seed, idx) >= dr.p ? __fmul_rn(v, dr.inv) : 0.f;
}

template <int DHB, bool GEO, bool DROP>
__global__ __launch_bounds__(PA_THREADS) void pa_fwd_kernel(const float *__restrict__ qkv, int ldq,
                                                            const int64_t *__restrict__ page_start, int N, int E, int Hh,
                                                            int tiles, float *__restrict__ out, int ldo,
                                                            float *__restrict__ lse, int vo, PaGeo<GEO> geo,
                                                            PaDrop<DROP> dr)
{
    using C = PaCfg<DHB>;
    __shared__ __attribute__((aligned(16))) float Ks[C::KT * C::LD];
    __shared__ __attribute__((aligned(16))) float Vs[C::KT * C::LD];
    __shared__ float4 Bs[GEO ? C::KT : 1];                               // boxes of the staged keys (GEO)
    const PaBlock b = pa_block(page_start, N, Hh, tiles);
    const int n = b.n;
    if (n == 0) return;
    const int dh = E / Hh, tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, grp = lane >> 4;
    const float rs = 1.f / sqrtf((float)dh);
    const int q = b.own_tile * PA_OWN + (tid >> 6) * 16 + l16;
    const bool qok = q < n;
    const float *qh = qkv + (size_t)b.base * ldq + b.head * dh;          // Q head slice of the page's row 0

    f32x4 Qf[DHB];
    pa_frag<DHB>(qok ? qh + (size_t)q * ldq : nullptr, dh, grp, true, Qf);
    const int nkt = (n + C::KT - 1) / C::KT;
    float4 qbox = make_float4(0.f, 0.f, 0.f, 0.f);
    [[maybe_unused]] float wt[8], phi[8];
    if constexpr (GEO) {
        if (qok) qbox = knn_box(geo.bboxes, (long long)b.base + q);
        pa_geo_weights(geo.w, b.head, wt);
    }

    // pass 1: the row maximum
    float m = -INFINITY;
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * C::KT;
        __syncthreads();
        pa_stage<DHB>(Ks, qh + E + (size_t)k0 * ldq, ldq, n - k0, dh, true, tid);
        if constexpr (GEO) pa_stage_boxes<DHB>(Bs, geo.bboxes, b.base + k0, n - k0, tid);
        __syncthreads();
        for (int sub = 0; sub < C::KT / 16 && k0 + sub * 16 < n; ++sub) {
            const f32x4 s = pa_dot<DHB>(Ks, sub, Qf, l16, grp);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = s[r] * rs;
                if constexpr (GEO) {
                    const int o = sub * 16 + 4 * grp + r;
                    v = v + pa_bias(qbox, Bs[o], geo.W, geo.H, k0 + o - q, wt, phi);
                }
                if (k0 + sub * 16 + 4 * grp + r < n && v > m) m = v;
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));

    // pass 2: the probabilities, their sum and the weighted V rows
    float l = 0.f;
    f32x4 acc[DHB];
#pragma unroll
    for (int c = 0; c < DHB; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * C::KT;
        __syncthreads();
        pa_stage<DHB>(Ks, qh + E + (size_t)k0 * ldq, ldq, n - k0, dh, true, tid);
        pa_stage<DHB>(Vs, qh + 2 * E + (size_t)k0 * ldq, ldq, n - k0, dh, true, tid);
        if constexpr (GEO) pa_stage_boxes<DHB>(Bs, geo.bboxes, b.base + k0, n - k0, tid);
        __syncthreads();
        for (int sub = 0; sub < C::KT / 16 && k0 + sub * 16 < n; ++sub) {
            const f32x4 s = pa_dot<DHB>(Ks, sub, Qf, l16, grp);
            f32x4 pw;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = s[r] * rs;
                if constexpr (GEO) {
                    const int o = sub * 16 + 4 * grp + r;
                    v = v + pa_bias(qbox, Bs[o], geo.W, geo.H, k0 + o - q, wt, phi);
                }
                const bool kin = k0 + sub * 16 + 4 * grp + r < n;
                pw[r] = kin ? expf(v - m) : 0.f;
                l += pw[r];
                if constexpr (DROP) {       // l keeps every key; the V product takes the dropped weight (a pair in range only)
                    if (qok && kin)
                        pw[r] = pa_dropped(dr, pa_drop_idx(b.base + q, Hh, b.head, b.base + k0 + sub * 16 + 4 * grp + r), pw[r]);
                }
            }
            pa_acc<DHB>(Vs, sub, pw, acc, l16, grp);
        }
    }
    l = pa_grp_sum(l);

    if (!qok) return;
    float *orow = out + (size_t)(b.base + q) * ldo + b.head * dh;
#pragma unroll
    for (int c = 0; c < DHB; ++c) {
        const int d = 16 * c + 4 * grp;
        if (d < dh) pa_st4(orow + d, acc[c] / l, vo != 0);
    }
    if (grp == 0) lse[(size_t)(b.base + q) * Hh + b.head] = m + logf(l);
}

// query side of the backward: dQ_i = rs * sum_j ds_ij K_j, keys in ascending tiles
template <int DHB, bool GEO, bool DROP>
__global__ __launch_bounds__(PA_THREADS) void pa_bwd_q_kernel(const float *__restrict__ g, int ldg,
                                                              const float *__restrict__ qkv, int ldq,
                                                              const float *__restrict__ out, int ldo,
                                                              const float *__restrict__ lse,
                                                              const int64_t *__restrict__ page_start, int N, int E, int Hh,
                                                              int tiles, float *__restrict__ dqkv, int lddq, int vg, int vo,
                                                              int vd, PaGeo<GEO> geo, PaDrop<DROP> dr)
{
    using C = PaCfg<DHB>;
    __shared__ __attribute__((aligned(16))) float Ks[C::KT * C::LD];
    __shared__ __attribute__((aligned(16))) float Vs[C::KT * C::LD];
    __shared__ float4 Bs[GEO ? C::KT : 1];                               // boxes of the staged keys (GEO)
    __shared__ float wred[GEO ? PA_THREADS / 64 * 8 : 1];                // the waves' partial sums of d w (GEO)
    const PaBlock b = pa_block(page_start, N, Hh, tiles);
    const int n = b.n;
    if (n == 0) {
        if constexpr (GEO)
            if (threadIdx.x < 8) geo.ws[(size_t)blockIdx.x * 8 + threadIdx.x] = 0.f;
        return;
    }
    const int dh = E / Hh, tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, grp = lane >> 4;
    const float rs = 1.f / sqrtf((float)dh);
    const int q = b.own_tile * PA_OWN + (tid >> 6) * 16 + l16;
    const bool qok = q < n;
    const float *qh = qkv + (size_t)b.base * ldq + b.head * dh;
    const float *grow = g + (size_t)(b.base + q) * ldg + b.head * dh;     // (read only where qok)
    const float *orow = out + (size_t)(b.base + q) * ldo + b.head * dh;

    f32x4 Qf[DHB], Gf[DHB];
    pa_frag<DHB>(qok ? qh + (size_t)q * ldq : nullptr, dh, grp, true, Qf);
    pa_frag<DHB>(qok ? grow : nullptr, dh, grp, vg != 0, Gf);
    const float lse_q = qok ? lse[(size_t)(b.base + q) * Hh + b.head] : 0.f;
    const float delta = pa_grp_sum(qok ? pa_delta_part(grow, orow, dh, grp, vg != 0, vo != 0) : 0.f);
    float4 qbox = make_float4(0.f, 0.f, 0.f, 0.f);
    [[maybe_unused]] float wt[8], phi[8], dw[8];
    if constexpr (GEO) {
        if (qok) qbox = knn_box(geo.bboxes, (long long)b.base + q);
        pa_geo_weights(geo.w, b.head, wt);
#pragma unroll
        for (int e = 0; e < 8; ++e) dw[e] = 0.f;
    }

    f32x4 acc[DHB];
#pragma unroll
    for (int c = 0; c < DHB; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkt = (n + C::KT - 1) / C::KT;
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * C::KT;
        __syncthreads();
        pa_stage<DHB>(Ks, qh + E + (size_t)k0 * ldq, ldq, n - k0, dh, true, tid);
        pa_stage<DHB>(Vs, qh + 2 * E + (size_t)k0 * ldq, ldq, n - k0, dh, true, tid);
        if constexpr (GEO) pa_stage_boxes<DHB>(Bs, geo.bboxes, b.base + k0, n - k0, tid);
        __syncthreads();
        for (int sub = 0; sub < C::KT / 16 && k0 + sub * 16 < n; ++sub) {
            const f32x4 s = pa_dot<DHB>(Ks, sub, Qf, l16, grp);
            const f32x4 dA = pa_dot<DHB>(Vs, sub, Gf, l16, grp);
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = s[r] * rs;
                if constexpr (GEO) {
                    const int o = sub * 16 + 4 * grp + r;
                    v = v + pa_bias(qbox, Bs[o], geo.W, geo.H, k0 + o - q, wt, phi);
                }
                const bool ok = qok && k0 + sub * 16 + 4 * grp + r < n;
                float da = dA[r];
                if constexpr (DROP) {       // (a pair in range only: ds is +0 elsewhere whatever da holds)
                    if (ok) da = pa_dropped(dr, pa_drop_idx(b.base + q, Hh, b.head, b.base + k0 + sub * 16 + 4 * grp + r), da);
                }
                ds[r] = ok ? expf(v - lse_q) * (da - delta) : 0.f;
                if constexpr (GEO) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) dw[e] = fmaf(ds[r], phi[e], dw[e]);
                }
            }
            pa_acc<DHB>(Ks, sub, ds, acc, l16, grp);
        }
    }

    if constexpr (GEO) {                   // lane partials -> wave (fixed butterfly) -> block (wave order) -> workspace
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = dw[e];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) wred[(tid >> 6) * 8 + e] = v;
        }
        __syncthreads();
        if (tid < 8) {
            float v = wred[tid];
            for (int w = 1; w < PA_THREADS / 64; ++w) v += wred[w * 8 + tid];
            geo.ws[(size_t)blockIdx.x * 8 + tid] = v;
        }
    }

    if (!qok) return;
    float *drow = dqkv + (size_t)(b.base + q) * lddq + b.head * dh;
#pragma unroll
    for (int c = 0; c < DHB; ++c) {
        const int d = 16 * c + 4 * grp;
        if (d < dh) pa_st4(drow + d, acc[c] * rs, vd != 0);
    }
}

// key side of the backward: dK_j = rs * sum_i ds_ij Q_i, dV_j = sum_i A_ij g_i, queries in ascending tiles
template <int DHB, bool GEO, bool DROP>
__global__ __launch_bounds__(PA_THREADS) void pa_bwd_k_kernel(const float *__restrict__ g, int ldg,
                                                              const float *__restrict__ qkv, int ldq,
                                                              const float *__restrict__ out, int ldo,
                                                              const float *__restrict__ lse,
                                                              const int64_t *__restrict__ page_start, int N, int E, int Hh,
                                                              int tiles, float *__restrict__ dqkv, int lddq, int vg, int vo,
                                                              int vd, PaGeo<GEO> geo, PaDrop<DROP> dr)
{
    using C = PaCfg<DHB>;
    __shared__ __attribute__((aligned(16))) float Qs[C::KT * C::LD];
    __shared__ __attribute__((aligned(16))) float Gs[C::KT * C::LD];
    __shared__ float lse_s[C::KT], del_s[C::KT];
    __shared__ float4 Bs[GEO ? C::KT : 1];                               // boxes of the staged queries (GEO)
    const PaBlock b = pa_block(page_start, N, Hh, tiles);
    const int n = b.n;
    if (n == 0) return;
    const int dh = E / Hh, tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, grp = lane >> 4;
    const float rs = 1.f / sqrtf((float)dh);
    const int k = b.own_tile * PA_OWN + (tid >> 6) * 16 + l16;
    const bool kok = k < n;
    const float *qh = qkv + (size_t)b.base * ldq + b.head * dh;
    const float *gh = g + (size_t)b.base * ldg + b.head * dh;
    const float *oh = out + (size_t)b.base * ldo + b.head * dh;

    f32x4 Kf[DHB], Vf[DHB];
    pa_frag<DHB>(kok ? qh + E + (size_t)k * ldq : nullptr, dh, grp, true, Kf);
    pa_frag<DHB>(kok ? qh + 2 * E + (size_t)k * ldq : nullptr, dh, grp, true, Vf);

    float4 kbox = make_float4(0.f, 0.f, 0.f, 0.f);
    [[maybe_unused]] float wt[8], phi[8];
    if constexpr (GEO) {
        if (kok) kbox = knn_box(geo.bboxes, (long long)b.base + k);
        pa_geo_weights(geo.w, b.head, wt);
    }

    f32x4 dK[DHB], dV[DHB];
#pragma unroll
    for (int c = 0; c < DHB; ++c) dK[c] = dV[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nqt = (n + C::KT - 1) / C::KT;
    for (int qt = 0; qt < nqt; ++qt) {
        const int q0 = qt * C::KT;
        __syncthreads();
        pa_stage<DHB>(Qs, qh + (size_t)q0 * ldq, ldq, n - q0, dh, true, tid);
        pa_stage<DHB>(Gs, gh + (size_t)q0 * ldg, ldg, n - q0, dh, vg != 0, tid);
        if constexpr (GEO) pa_stage_boxes<DHB>(Bs, geo.bboxes, b.base + q0, n - q0, tid);
        {   // four threads per query: its delta (the query side's bits) and its lse
            const int qq = tid >> 2, j = tid & 3;
            const bool ok = qq < C::KT && q0 + qq < n;
            float part = ok ? pa_delta_part(gh + (size_t)(q0 + qq) * ldg, oh + (size_t)(q0 + qq) * ldo, dh, j, vg != 0,
                                            vo != 0)
                            : 0.f;
            part += __shfl_xor(part, 1, 64);
            part += __shfl_xor(part, 2, 64);
            if (ok && j == 0) {
                del_s[qq] = part;
                lse_s[qq] = lse[(size_t)(b.base + q0 + qq) * Hh + b.head];
            }
        }
        __syncthreads();
        for (int sub = 0; sub < C::KT / 16 && q0 + sub * 16 < n; ++sub) {
            const f32x4 s = pa_dot<DHB>(Qs, sub, Kf, l16, grp);
            const f32x4 dA = pa_dot<DHB>(Gs, sub, Vf, l16, grp);
            f32x4 pw, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = sub * 16 + 4 * grp + r;
                float v = s[r] * rs;
                if constexpr (GEO)          // own = key, other = query: still (query box, key box, key - query)
                    v = v + pa_bias(Bs[qi], kbox, geo.W, geo.H, k - (q0 + qi), wt, phi);
                if (kok && q0 + qi < n) {
                    pw[r] = expf(v - lse_s[qi]);
                    if constexpr (DROP) {   // ds from the undropped A and the dropped dA; dV weighs with the dropped A
                        const unsigned long long idx = pa_drop_idx(b.base + q0 + qi, Hh, b.head, b.base + k);
                        ds[r] = pw[r] * (pa_dropped(dr, idx, dA[r]) - del_s[qi]);
                        pw[r] = pa_dropped(dr, idx, pw[r]);
                    } else {
                        ds[r] = pw[r] * (dA[r] - del_s[qi]);
                    }
                } else {
                    pw[r] = ds[r] = 0.f;
                }
            }
            pa_acc<DHB>(Gs, sub, pw, dV, l16, grp);
            pa_acc<DHB>(Qs, sub, ds, dK, l16, grp);
        }
    }

    if (!kok) return;
    float *drow = dqkv + (size_t)(b.base + k) * lddq + b.head * dh;
#pragma unroll
    for (int c = 0; c < DHB; ++c) {
        const int d = 16 * c + 4 * grp;
        if (d < dh) {
            pa_st4(drow + E + d, dK[c] * rs, vd != 0);
            pa_st4(drow + 2 * E + d, dV[c], vd != 0);
        }
    }
}

// E, Hh and the derived head width; the grid of (page, head, own tile) blocks must fit an int
static bool pa_shape_ok(int B, int N, int E, int Hh)
{
    if (E < 4 || E > PA_MAX_E || Hh < 1 || E % Hh != 0 || N < 0 || B < 0) return false;
    const int dh = E / Hh;
    if (dh % 4 != 0 || dh < 4 || dh > PA_MAX_DH) return false;
    return (long long)B * Hh * cdiv(N > 0 ? N : 1, PA_OWN) <= 0x7fffffffLL;
}

// d w[a][e] from the query side's block partials: one thread per (a, e), pages ascending, a page's own tiles ascending
__global__ __launch_bounds__(64) void pa_geo_fold_kernel(const float *__restrict__ ws, const int64_t *__restrict__ page_start,
                                                         int B, int N, int Hh, int tiles, float *__restrict__ d_w)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Hh * 8) return;
    const int a = i >> 3, e = i & 7;
    float v = 0.f;
    for (int p = 0; p < B; ++p) {
        const PageRows pr = page_rows(page_start, p, N);
        const int nt = (pr.end - pr.base + PA_OWN - 1) / PA_OWN;
        const float *src = ws + ((size_t)p * Hh + a) * tiles * 8 + e;
        for (int t = 0; t < nt; ++t) v += src[(size_t)t * 8];
    }
    d_w[i] = v;
}

}  // namespace

#define PA_DISPATCH(KERNEL, GEO, DROP, ...)                                                                                     \
    do {                                                                                                                        \
        if (dh <= 16) COVA_LAUNCH(HIP_KERNEL_NAME(KERNEL<1, GEO, DROP>), dim3(blocks), dim3(PA_THREADS), st, __VA_ARGS__);      \
        else if (dh <= 32) COVA_LAUNCH(HIP_KERNEL_NAME(KERNEL<2, GEO, DROP>), dim3(blocks), dim3(PA_THREADS), st, __VA_ARGS__); \
        else if (dh <= 64) COVA_LAUNCH(HIP_KERNEL_NAME(KERNEL<4, GEO, DROP>), dim3(blocks), dim3(PA_THREADS), st, __VA_ARGS__); \
        else if (dh <= 96) COVA_LAUNCH(HIP_KERNEL_NAME(KERNEL<6, GEO, DROP>), dim3(blocks), dim3(PA_THREADS), st, __VA_ARGS__); \
        else COVA_LAUNCH(HIP_KERNEL_NAME(KERNEL<8, GEO, DROP>), dim3(blocks), dim3(PA_THREADS), st, __VA_ARGS__);               \
    } while (0)

// 0 < p < 1 (a NaN fails both compares) and every mask index within its 32 + 32 bits
static bool pa_drop_ok(float p, int N, int Hh) { return p > 0.f && p < 1.f && (long long)N * Hh < (1LL << 32); }

static PaDrop<true> pa_drop_of(float p, unsigned long long seed) { return PaDrop<true>{p, 1.f / (1.f - p), seed}; }

// the checks and launches every form shares; the GEO and DROP entry points check their own operands first
template <bool GEO, bool DROP>
static int pa_fwd(const float *qkv, int ldq, const int64_t *page_start, int B, int N, int E, int Hh, float *out, int ldo,
                  float *lse, PaGeo<GEO> geo, PaDrop<DROP> dr, void *stream)
{
    COVA_REQUIRE(pa_shape_ok(B, N, E, Hh) && ldq >= 3 * E && ldo >= E);
    if (N == 0 || B == 0) return COVA_OK;
    COVA_REQUIRE(qkv && page_start && out && lse);
    COVA_REQUIRE(vec4_ok(qkv, ldq));                     // the engine's own dense buffer: no scalar form
    const int dh = E / Hh, tiles = cdiv(N, PA_OWN), blocks = B * Hh * tiles;
    const int vo = vec4_ok(out, ldo);
    hipStream_t st = (hipStream_t)stream;
    PA_DISPATCH(pa_fwd_kernel, GEO, DROP, qkv, ldq, page_start, N, E, Hh, tiles, out, ldo, lse, vo, geo, dr);
    return COVA_OK;
}

template <bool GEO, bool DROP>
static int pa_bwd(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo, const float *lse,
                  const int64_t *page_start, int B, int N, int E, int Hh, float *dqkv, int lddq, PaGeo<GEO> geo,
                  PaDrop<DROP> dr, void *stream)
{
    COVA_REQUIRE(pa_shape_ok(B, N, E, Hh) && ldg >= E && ldq >= 3 * E && ldo >= E && lddq >= 3 * E);
    if (N == 0 || B == 0) return COVA_OK;
    COVA_REQUIRE(g && qkv && out && lse && page_start && dqkv);
    COVA_REQUIRE(vec4_ok(qkv, ldq));
    const int dh = E / Hh, tiles = cdiv(N, PA_OWN), blocks = B * Hh * tiles;
    const int vg = vec4_ok(g, ldg), vo = vec4_ok(out, ldo), vd = vec4_ok(dqkv, lddq);
    hipStream_t st = (hipStream_t)stream;
    PA_DISPATCH(pa_bwd_q_kernel, GEO, DROP, g, ldg, qkv, ldq, out, ldo, lse, page_start, N, E, Hh, tiles, dqkv, lddq, vg, vo,
                vd, geo, dr);
    PA_DISPATCH(pa_bwd_k_kernel, GEO, DROP, g, ldg, qkv, ldq, out, ldo, lse, page_start, N, E, Hh, tiles, dqkv, lddq, vg, vo,
                vd, geo, dr);
    return COVA_OK;
}

COVA_API int cova_page_attn_fwd(const float *qkv, int ldq, const int64_t *page_start, int B, int N, int E, int Hh, float *out,
                                int ldo, float *lse, void *stream)
{
    return pa_fwd<false, false>(qkv, ldq, page_start, B, N, E, Hh, out, ldo, lse, PaGeo<false>{}, PaDrop<false>{}, stream);
}

COVA_API int cova_page_attn_bwd(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                                const float *lse, const int64_t *page_start, int B, int N, int E, int Hh, float *dqkv,
                                int lddq, void *stream)
{
    return pa_bwd<false, false>(g, ldg, qkv, ldq, out, ldo, lse, page_start, B, N, E, Hh, dqkv, lddq, PaGeo<false>{},
                                PaDrop<false>{}, stream);
}

COVA_API int cova_page_attn_geo_workspace_floats(int B, int N, int Hh)
{
    if (B <= 0 || N <= 0 || Hh < 1) return 0;
    const long long v = 8LL * B * Hh * cdiv(N, PA_OWN);
    return v <= 0x7fffffffLL ? (int)v : 0;
}

// the GEO entry points' own checks and launches, with and without DROP
template <bool DROP>
static int pa_fwd_geo(const float *qkv, int ldq, const int64_t *page_start, const float *bboxes, const float *geo_w,
                      float img_w, float img_h, int B, int N, int E, int Hh, float *out, int ldo, float *lse, PaDrop<DROP> dr,
                      void *stream)
{
    COVA_REQUIRE(img_w > 0.f && img_h > 0.f);
    if (N > 0 && B > 0) {
        COVA_REQUIRE(bboxes && geo_w);
    }
    return pa_fwd<true, DROP>(qkv, ldq, page_start, B, N, E, Hh, out, ldo, lse,
                              PaGeo<true>{bboxes, geo_w, img_w, img_h, nullptr}, dr, stream);
}

template <bool DROP>
static int pa_bwd_geo(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo, const float *lse,
                      const int64_t *page_start, const float *bboxes, const float *geo_w, float img_w, float img_h, int B,
                      int N, int E, int Hh, float *dqkv, int lddq, float *d_geo_w, float *workspace, PaDrop<DROP> dr,
                      void *stream)
{
    COVA_REQUIRE(img_w > 0.f && img_h > 0.f);
    if (N > 0 && B > 0) {
        COVA_REQUIRE(bboxes && geo_w && d_geo_w && workspace);
        COVA_REQUIRE(Hh < 1 || cova_page_attn_geo_workspace_floats(B, N, Hh) > 0);      // the workspace's size fits an int
    }
    const int rc = pa_bwd<true, DROP>(g, ldg, qkv, ldq, out, ldo, lse, page_start, B, N, E, Hh, dqkv, lddq,
                                      PaGeo<true>{bboxes, geo_w, img_w, img_h, workspace}, dr, stream);
    if (rc != COVA_OK || N == 0 || B == 0) return rc;
    COVA_LAUNCH(pa_geo_fold_kernel, dim3(cdiv(Hh * 8, 64)), dim3(64), (hipStream_t)stream, workspace, page_start, B,
                N, Hh, cdiv(N, PA_OWN), d_geo_w);
    return COVA_OK;
}

COVA_API int cova_page_attn_fwd_geo(const float *qkv, int ldq, const int64_t *page_start, const float *bboxes,
                                    const float *geo_w, float img_w, float img_h, int B, int N, int E, int Hh, float *out,
                                    int ldo, float *lse, void *stream)
{
    return pa_fwd_geo<false>(qkv, ldq, page_start, bboxes, geo_w, img_w, img_h, B, N, E, Hh, out, ldo, lse, PaDrop<false>{},
                             stream);
}

COVA_API int cova_page_attn_bwd_geo(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                                    const float *lse, const int64_t *page_start, const float *bboxes, const float *geo_w,
                                    float img_w, float img_h, int B, int N, int E, int Hh, float *dqkv, int lddq,
                                    float *d_geo_w, float *workspace, void *stream)
{
    return pa_bwd_geo<false>(g, ldg, qkv, ldq, out, ldo, lse, page_start, bboxes, geo_w, img_w, img_h, B, N, E, Hh, dqkv, lddq,
                             d_geo_w, workspace, PaDrop<false>{}, stream);
}

// ---- attention dropout: the pairs above on the DROP instantiations, 0 < p < 1
COVA_API int cova_page_attn_fwd_drop(const float *qkv, int ldq, const int64_t *page_start, int B, int N, int E, int Hh,
                                     float *out, int ldo, float *lse, float p, unsigned long long seed, void *stream)
{
    COVA_REQUIRE(pa_drop_ok(p, N, Hh));
    return pa_fwd<false, true>(qkv, ldq, page_start, B, N, E, Hh, out, ldo, lse, PaGeo<false>{}, pa_drop_of(p, seed), stream);
}

COVA_API int cova_page_attn_bwd_drop(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                                     const float *lse, const int64_t *page_start, int B, int N, int E, int Hh, float *dqkv,
                                     int lddq, float p, unsigned long long seed, void *stream)
{
    COVA_REQUIRE(pa_drop_ok(p, N, Hh));
    return pa_bwd<false, true>(g, ldg, qkv, ldq, out, ldo, lse, page_start, B, N, E, Hh, dqkv, lddq, PaGeo<false>{},
                               pa_drop_of(p, seed), stream);
}

COVA_API int cova_page_attn_fwd_geo_drop(const float *qkv, int ldq, const int64_t *page_start, const float *bboxes,
                                         const float *geo_w, float img_w, float img_h, int B, int N, int E, int Hh,
                                         float *out, int ldo, float *lse, float p, unsigned long long seed, void *stream)
{
    COVA_REQUIRE(pa_drop_ok(p, N, Hh));
    return pa_fwd_geo<true>(qkv, ldq, page_start, bboxes, geo_w, img_w, img_h, B, N, E, Hh, out, ldo, lse,
                            pa_drop_of(p, seed), stream);
}

COVA_API int cova_page_attn_bwd_geo_drop(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                                         const float *lse, const int64_t *page_start, const float *bboxes,
                                         const float *geo_w, float img_w, float img_h, int B, int N, int E, int Hh,
                                         float *dqkv, int lddq, float *d_geo_w, float *workspace, float p,
                                         unsigned long long seed, void *stream)
{
    COVA_REQUIRE(pa_drop_ok(p, N, Hh));
    return pa_bwd_geo<true>(g, ldg, qkv, ldq, out, ldo, lse, page_start, bboxes, geo_w, img_w, img_h, B, N, E, Hh, dqkv, lddq,
                            d_geo_w, workspace, pa_drop_of(p, seed), stream);
}
