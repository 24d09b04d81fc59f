// Joint page decoding (the decision side of "exactly one box of each non-background class per page"): instead of the
// arg-max of every class column on its own (cova_page_class_topk, cova_eval_page_ranks' top1), the choice of pairwise
// DISTINCT boxes i_1..i_C, C = NC - 1, that maximises sum_c score[i_c, c] -- with score = logit[., c] - logit[., 0] the most
// probable labelling of the page under the model's per-box softmax.  Solved exactly by enumeration over the C + 1 best boxes
// of every class: in any assignment the other classes hold at most C - 1 of them, so a class that sits on a box outside its
// list can move to either of two free listed boxes without lowering the (monotonically rounded) total, and one of the two
// moves is not the optimum itself.  The m^C rank tuples over the lists, m = min(n, C + 1) <= 7, therefore hold the best and
// the second-best assignment.  The contract is in include/cova_hip.h, the numpy statement in tests/decode_oracle.py.
#include "common.h"

namespace {

constexpr int NONE = 0x7fffffff;

// additions and compares only, every one rounded on its own
#pragma clang fp contract(off)

__device__ __forceinline__ float score_of(const float *__restrict__ row, int c, int score_mode)
{
    float v = row[c];
    if (score_mode) v = __fsub_rn(v, row[0]);
    return v != v ? -INFINITY : v;                          // a NaN score counts as -inf
}

// What a lane, a wave, the block knows of the assignments it has seen: how many, the greatest total with its tuple id (the
// lowest id among equal totals) and the greatest total of the others.  best / second are order statistics of a multiset,
// so the result of a merge tree does not depend on its shape.
struct Best {
    double best, second;
    int id, cnt;
};

__device__ __forceinline__ void best_merge(Best &a, const Best &b)
{
    if (b.cnt == 0) return;
    if (a.cnt == 0) { a = b; return; }
    const bool a_wins = a.best > b.best || (a.best == b.best && a.id < b.id);
    const Best w = a_wins ? a : b, l = a_wins ? b : a;
    double sec = l.best;                                    // l.second <= l.best: it cannot be the runner-up
    if (w.cnt > 1 && w.second > sec) sec = w.second;
    a.best = w.best, a.second = sec, a.id = w.id, a.cnt = a.cnt + b.cnt;
}

// One block per page: 4 waves, 16 from five classes on (6^5 and 7^6 tuples).  Phase 1, a wave per class column: the m best
// boxes in cova_page_class_topk's order, one pass over the page per selection (selection j takes the best box that comes
// strictly after selection j - 1 in that order);
// the column is strided by NC floats, a page is a few hundred boxes, every pass after the first hits L2.  Phase 2: the m^C
// rank tuples in contiguous runs over the block's lanes (a lane walks its run as an odometer, class 1 the most significant
// digit, so ascending tuple id is the lexicographic order and "first seen wins a tie" is the tie rule), then the xor
// butterfly and a fold of one entry per wave in LDS.
template <int C>
constexpr int decode_threads() { return C >= 5 ? 1024 : 256; }

template <int C>
__global__ __launch_bounds__(decode_threads<C>()) void page_joint_decode_kernel(const float *__restrict__ logits,
                                                                const int64_t *__restrict__ labels,
                                                                const int64_t *__restrict__ page_start,
                                                                const int *__restrict__ page_ids, int P, int score_mode,
                                                                int *__restrict__ choice, int *__restrict__ hit,
                                                                double *__restrict__ gap)
{
    constexpr int NC = C + 1, M = C + 1, THREADS = decode_threads<C>(), WAVES = THREADS / 64;
    __shared__ int s_idx[C][M];
    __shared__ float s_val[C][M];
    __shared__ int s_has[C];
    __shared__ Best s_red[WAVES];
    const int page = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = page_ids ? page_ids[page] : page;
    if (row < 0 || row >= P) return;                        // block-uniform: no barrier is skipped by a part of the block
    int64_t lo = page_start[page], hi = page_start[page + 1];
    if (lo < 0) lo = 0;
    if (hi < lo) hi = lo;
    const int n = (int)(hi - lo < (int64_t)NONE - 64 ? hi - lo : (int64_t)NONE - 64);
    const int m = n < M ? n : M;
    const float *__restrict__ rows = logits + (size_t)lo * NC;

    for (int k = wave; k < C; k += WAVES) {
        const int c = k + 1;
        if (hit) {
            int has = 0;
            for (int i = lane; i < n; i += 64) has |= labels[lo + i] == (int64_t)c ? 1 : 0;
            has = __ballot(has) != 0ull;
            if (lane == 0) s_has[k] = has;
        }
        float pv = 0.f;
        int pi = -1;
        for (int j = 0; j < m; ++j) {
            float bv = -INFINITY;
            int bi = NONE;
            for (int i = lane; i < n; i += 64) {
                const float v = score_of(rows + (size_t)i * NC, c, score_mode);
                const bool after = j == 0 || v < pv || (v == pv && i > pi);   // ranks_before(pv, pi, v, i) of rows.h
                if (after && (bi == NONE || v > bv)) { bv = v; bi = i; }   // ascending i per lane: a tie keeps the lower index
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {              // wave_ranked_first (rows.h), written out: these statements must match it
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi != NONE && (bi == NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (lane == 0) { s_idx[k][j] = bi; s_val[k][j] = bv; }          // j < m <= n: a box is always found
            pv = bv, pi = bi;
        }
    }
    __syncthreads();

    Best b;
    b.best = b.second = 0.0, b.id = 0, b.cnt = 0;
    if (n >= C) {
        int T = 1;
#pragma unroll
        for (int k = 0; k < C; ++k) T *= m;                 // <= 7^6 = 117649
        const int run = (T + THREADS - 1) / THREADS, t0 = tid * run, t1 = t0 + run < T ? t0 + run : T;
        int r[C];
        {
            int x = t0;
#pragma unroll
            for (int k = C - 1; k >= 0; --k) { r[k] = x % m; x /= m; }
        }
        for (int t = t0; t < t1; ++t) {
            int box[C];
#pragma unroll
            for (int k = 0; k < C; ++k) box[k] = s_idx[k][r[k]];
            bool distinct = true;
#pragma unroll
            for (int k = 0; k < C; ++k)
#pragma unroll
                for (int l = k + 1; l < C; ++l) distinct = distinct && box[k] != box[l];
            if (distinct) {
                double tot = (double)s_val[0][r[0]];
#pragma unroll
                for (int k = 1; k < C; ++k) tot = __dadd_rn(tot, (double)s_val[k][r[k]]);
                if (tot != tot) tot = -(double)INFINITY;    // +inf + -inf: a NaN total counts as -inf
                if (b.cnt == 0) {
                    b.best = tot, b.id = t;
                } else if (tot > b.best) {                  // strictly: among equal totals the lowest id stays
                    b.second = b.best, b.best = tot, b.id = t;
                } else if (b.cnt == 1 || tot > b.second) {
                    b.second = tot;
                }
                ++b.cnt;
            }
            int carry = 1;
#pragma unroll
            for (int k = C - 1; k >= 0; --k) {
                r[k] += carry;
                carry = r[k] == m ? 1 : 0;
                if (carry) r[k] = 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            Best ob;
            ob.best = __shfl_xor(b.best, o, 64);
            ob.second = __shfl_xor(b.second, o, 64);
            ob.id = __shfl_xor(b.id, o, 64);
            ob.cnt = __shfl_xor(b.cnt, o, 64);
            best_merge(b, ob);
        }
        if (lane == 0) s_red[wave] = b;
    }
    __syncthreads();
    if (tid != 0) return;

    int ch[C];
    double g = (double)INFINITY;
    if (n >= C) {
        b = s_red[0];
        for (int w = 1; w < WAVES; ++w) best_merge(b, s_red[w]);
        int x = b.id;                                       // m >= C: class k always has a candidate the k - 1 before it left
#pragma unroll
        for (int k = C - 1; k >= 0; --k) { ch[k] = s_idx[k][x % m]; x /= m; }
        if (b.cnt > 1) g = b.best == b.second ? 0.0 : b.best - b.second;
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) ch[k] = n > 0 ? s_idx[k][0] : -1;       // too few boxes: the column decision
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const size_t at = (size_t)row * C + k;
        choice[at] = ch[k];
        if (hit) hit[at] = !s_has[k] ? -1 : (labels[lo + ch[k]] == (int64_t)(k + 1) ? 1 : 0);
    }
    if (gap) gap[row] = g;
}

}  // namespace

COVA_API int cova_page_joint_decode(const float *logits, const int64_t *labels, const int64_t *page_start,
                                    const int *page_ids, int B, int NC, int P, int score_mode, int *choice, int *hit,
                                    double *gap, void *stream)
{
    COVA_REQUIRE(logits && page_start && choice && B > 0 && NC >= 2 && NC <= 7 && P > 0);
    COVA_REQUIRE((score_mode == 0 || score_mode == 1) && (!hit || labels));
#define COVA_DECODE_CASE(C)                                                                               \
    case C + 1:                                                                                           \
        COVA_LAUNCH(page_joint_decode_kernel<C>, dim3(B), dim3(decode_threads<C>()), (hipStream_t)stream, \
                    logits, labels, page_start, page_ids, P, score_mode, choice, hit, gap);               \
        break;
    switch (NC) {
        COVA_DECODE_CASE(1)
        COVA_DECODE_CASE(2)
        COVA_DECODE_CASE(3)
        COVA_DECODE_CASE(4)
        COVA_DECODE_CASE(5)
        COVA_DECODE_CASE(6)
    }
#undef COVA_DECODE_CASE
    COVA_LAUNCH_CHECK();
    return COVA_OK;
}
