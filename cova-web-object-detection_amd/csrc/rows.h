// What the row and page kernels (head.hip, loss.hip, rank.hip, mine.hip, eval.hip, decode.hip, readout.hip, page_attn.hip,
// page_encoder.hip) promise each other bit for bit: the class limit, the logsumexp of a row, the label predicate, the rows of
// a page, the chunk access of a row whose lanes sit over channels and the ranking order.  One definition each; none of them
// holds a product that feeds a sum, so a file-level fp-contract pragma of the including file has nothing to reach here.
#pragma once
#include "common.h"

// logits rows of at most this many classes (decode.hip enumerates and stops at 7); engine.LOSS_MAX_CLASSES restates it
constexpr int COVA_MAX_CLASSES = 16;

// "no box": the index of an empty selection in the ranking order below
constexpr int RANK_NONE = 0x7fffffff;

// max / first argmax / logsumexp of one row: f32, expf / logf, the first maximum wins.  ce_sum_kernel (head.hip) writes
// the same statement out (the call changes its register allocation) and must match this one.
__device__ __forceinline__ float row_lse(const float *__restrict__ l, int NC, int *am_out)
{
    float m = l[0];
    int am = 0;
    for (int k = 1; k < NC; ++k)
        if (l[k] > m) { m = l[k]; am = k; }
    float se = 0.f;
    for (int k = 0; k < NC; ++k) se += expf(l[k] - m);
    *am_out = am;
    return m + logf(se);
}

// a row's label under the criterion's options -- 0: kept (a term of the criterion, a candidate of the ranking loss),
// 1: ignored, 2: outside [0, NC) and not the ignore label
__device__ __forceinline__ int label_state(long long lab, int NC, long long ignore_index, int has_ignore)
{
    if (has_ignore && lab == ignore_index) return 1;
    return (lab < 0 || lab >= NC) ? 2 : 0;
}

// The rows [base, end) of page p in a flat batch of N rows, from page_start [B + 1].  Who does what with a malformed table:
//   mine_select_kernel, rank_lists_kernel, readout_fwd_kernel, readout_bwd_kernel (readout.hip), the kernels of
//   page_attn.hip (pa_block)
//                                              page_rows(): both ends clamped into [0, N], end >= base
//   page_joint_decode_kernel                   its own clamp without N: lo >= 0, hi >= lo
//   eval_page_ranks_kernel, page_class_topk_kernel, rank_bwd_kernel's page search    page_start as it is
__device__ __forceinline__ int page_clamp(long long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }

struct PageRows {
    int base, end;
};

__device__ __forceinline__ PageRows page_rows(const int64_t *__restrict__ page_start, int p, int N)
{
    const int base = page_clamp(page_start[p], 0, N);
    return PageRows{base, page_clamp(page_start[p + 1], base, N)};
}

// One chunk of a row whose lanes sit over channels (readout.hip, page_encoder.hip): V = 4 is a 16-byte access (the caller has
// checked C % 4 == 0 and the alignment of every base and leading dimension), V = 1 a scalar one.
template <int V>
__device__ __forceinline__ void ro_load(const float *__restrict__ p, float (&v)[V])
{
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void ro_store(float *__restrict__ p, const float (&v)[V])
{
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// The ranking order of a class column: score descending, ties to the lower page-local index.  "a comes before b":
__device__ __forceinline__ bool ranks_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// The first (value, index) pair of the wave in that order; a lane without a pair holds index RANK_NONE and never wins, a
// lane's own pair stays unless another comes before it (so a NaN value survives only where no other lane has a pair).
// eval_page_ranks_kernel calls it; page_joint_decode_kernel writes the same statements out (with the call its 7-class
// launch measured 0.8 % slower, outside the parent's own spread) and must match them.  page_class_topk_kernel's butterfly
// is ranks_before() alone, without the RANK_NONE tests: its lanes never select a NaN and its empty lanes hold
// (-inf, RANK_NONE), which loses every compare.
__device__ __forceinline__ void wave_ranked_first(float &bv, int &bi)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != RANK_NONE && (bi == RANK_NONE || ranks_before(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
}
