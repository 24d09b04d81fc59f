// Per-page listwise ranking loss: the training term over the lists the evaluation ranks.  A list
// is (page p, class c >= 1) with the scores v_n = logits[n, c] of the page's candidate rows (label in [0, NC), not the
// ignore label); its targets are the rows labelled c, and a list with a target is scored:
//   L_pc = lse_candidates(v) - lse_targets(v),   dL_pc/dv_n = softmax_cand(v)_n - [n is a target] softmax_tgt(v)_n.
//   rank_lists_kernel  one wave per list, as eval.hip: f32 maxima, expf(v - m) terms in f32 summed in float64 (lane-
//                      strided over the page's rows, then the xor butterfly wave_sum_f64), lse = (double)m + log(sum) -> lists.
//   rank_fold_kernel   one wave folds the table into acc = {sum w_c L_pc, sum w_c, scored lists} in a fixed order.
//   rank_bwd_kernel    one thread per row: finds the row's page, reads the lists' lse values, writes or accumulates
//                      dlogits[n, 1..NC-1]; thread 0 writes or accumulates the loss.
// No atomics, no workspace beyond the table, no host read; a list's result is a function of its page's rows alone.
#include "rows.h"

// the contract counts one rounding per operation (accumulate = pre-fill + the accumulate == 0 result, in f32): no fused
// multiply-adds in this file
#pragma clang fp contract(off)

namespace {

constexpr int RANK_THREADS = 256;
constexpr int RANK_LIST = 4;              // doubles per list: lse of the candidates, lse of the targets, the two counts

__global__ __launch_bounds__(RANK_THREADS) void rank_lists_kernel(const float *__restrict__ logits,
                                                                  const int64_t *__restrict__ labels,
                                                                  const int64_t *__restrict__ page_start, int B, int N,
                                                                  int NC, long long ignore_index, int has_ignore,
                                                                  double *__restrict__ lists)
{
    const int task = blockIdx.x * (RANK_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (task >= B * (NC - 1)) return;                     // wave-uniform
    const int p = task / (NC - 1), c = 1 + task - p * (NC - 1);
    const PageRows pr = page_rows(page_start, p, N);
    const int base = pr.base, end = pr.end;
    float mA = -INFINITY, mT = -INFINITY;
    int nA = 0, nT = 0;
    for (int n = base + lane; n < end; n += 64) {
        const long long lab = labels[n];
        if (label_state(lab, NC, ignore_index, has_ignore) != 0) continue;
        const float v = logits[(size_t)n * NC + c];
        ++nA;
        if (v > mA) mA = v;
        if (lab == c) {
            ++nT;
            if (v > mT) mT = v;
        }
    }
    nA = wave_sum_i(nA);
    nT = wave_sum_i(nT);
    double *out = lists + (size_t)task * RANK_LIST;
    if (nT == 0) {                                        // unscored: counts only
        if (lane == 0) {
            out[0] = 0.0;
            out[1] = 0.0;
            out[2] = (double)nA;
            out[3] = 0.0;
        }
        return;
    }
    mA = wave_max_gt(mA);
    mT = wave_max_gt(mT);
    double sA = 0.0, sT = 0.0;
    for (int n = base + lane; n < end; n += 64) {
        const long long lab = labels[n];
        if (label_state(lab, NC, ignore_index, has_ignore) != 0) continue;
        const float v = logits[(size_t)n * NC + c];
        sA += (double)expf(v - mA);
        if (lab == c) sT += (double)expf(v - mT);
    }
    sA = wave_sum_f64(sA);
    sT = wave_sum_f64(sT);
    if (lane == 0) {
        out[0] = (double)mA + log(sA);
        out[1] = (double)mT + log(sT);
        out[2] = (double)nA;
        out[3] = (double)nT;
    }
}

// lane i: lists i, i + 64, ... in turn; then the butterfly
__global__ __launch_bounds__(64) void rank_fold_kernel(const double *__restrict__ lists, int n_lists, int NC,
                                                       const float *__restrict__ weight, double *__restrict__ acc)
{
    double num = 0.0, den = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < n_lists; i += 64) {
        const double *l = lists + (size_t)i * RANK_LIST;
        if (l[3] > 0.0) {
            const double w = weight ? (double)weight[1 + i % (NC - 1)] : 1.0;
            num += w * (l[0] - l[1]);
            den += w;
            cnt += 1.0;
        }
    }
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    cnt = wave_sum_f64(cnt);
    if (threadIdx.x == 0) {
        acc[0] = num;
        acc[1] = den;
        acc[2] = cnt;
    }
}

__global__ __launch_bounds__(RANK_THREADS) void rank_bwd_kernel(
    const float *__restrict__ logits, const int64_t *__restrict__ labels, const int64_t *__restrict__ page_start, int B,
    int N, int NC, const float *__restrict__ weight, long long ignore_index, int has_ignore,
    const double *__restrict__ lists, const double *__restrict__ acc, double rank_weight, int mean,
    const float *__restrict__ grad_scale, float *__restrict__ loss, float *__restrict__ dlogits, int accumulate)
{
    const double num = acc[0], den = acc[1];
    if (loss && blockIdx.x == 0 && threadIdx.x == 0) {
        const double R = mean ? (den > 0.0 ? num / den : 0.0) : num;
        const float term = (float)(rank_weight * R);
        loss[0] = accumulate ? loss[0] + term : term;
    }
    if (!dlogits) return;
    const int n = blockIdx.x * RANK_THREADS + threadIdx.x;
    if (n >= N) return;
    float *d = dlogits + (size_t)n * NC;
    // the row's page: the first p with page_start[p + 1] > n, when page_start[p] <= n (0 <= n < N: the clamps of the
    // contract change neither comparison); p stays in [0, B) whatever page_start holds
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (page_start[mid + 1] > (int64_t)n) hi = mid;
        else lo = mid + 1;
    }
    const long long lab = labels[n];
    const bool live = lo < B && page_start[lo] <= (int64_t)n && label_state(lab, NC, ignore_index, has_ignore) == 0;
    if (!live) {
        if (!accumulate)
            for (int k = 0; k < NC; ++k) d[k] = 0.f;
        return;
    }
    const double s = mean ? (den > 0.0 ? 1.0 / den : 0.0) : 1.0;
    const float *l = logits + (size_t)n * NC;
    const double *pl = lists + (size_t)lo * (NC - 1) * RANK_LIST;
    if (!accumulate) d[0] = 0.f;
    for (int c = 1; c < NC; ++c) {
        const double *e = pl + (size_t)(c - 1) * RANK_LIST;
        if (!(e[3] > 0.0)) {                              // unscored list
            if (!accumulate) d[c] = 0.f;
            continue;
        }
        float g = (float)(rank_weight * s * (weight ? (double)weight[c] : 1.0));
        if (grad_scale) g *= grad_scale[0];
        const double v = (double)l[c];
        const float x = (float)(v - e[0]);
        float t = 0.f;
        if (lab == c) t = expf((float)(v - e[1]));
        const float dv = g * (expf(x) - t);
        d[c] = accumulate ? d[c] + dv : dv;
    }
}

}  // namespace

COVA_API int cova_page_rank_loss_fwd(const float *logits, const int64_t *labels, const int64_t *page_start, int B, int N,
                                     int NC, const float *class_weight, long long ignore_index, int has_ignore_index,
                                     double *lists, double *acc, void *stream)
{
    COVA_REQUIRE(logits && labels && page_start && lists && acc && B >= 1 && N >= 1);
    COVA_REQUIRE(NC >= 2 && NC <= COVA_MAX_CLASSES);
    const long long n_lists = (long long)B * (NC - 1);
    COVA_REQUIRE(n_lists <= INT32_MAX);
    hipStream_t s = (hipStream_t)stream;
    COVA_LAUNCH(rank_lists_kernel, dim3(cdiv((int)n_lists, RANK_THREADS / 64)), dim3(RANK_THREADS), s, logits,
                labels, page_start, B, N, NC, ignore_index, has_ignore_index != 0, lists);
    COVA_LAUNCH(rank_fold_kernel, dim3(1), dim3(64), s, lists, (int)n_lists, NC, class_weight, acc);
    return COVA_OK;
}

COVA_API int cova_page_rank_loss_bwd(const float *logits, const int64_t *labels, const int64_t *page_start, int B, int N,
                                     int NC, const float *class_weight, long long ignore_index, int has_ignore_index,
                                     const double *lists, const double *acc_total, double rank_weight, int reduction_mean,
                                     const float *grad_scale, float *loss_inout, float *dlogits, int accumulate,
                                     void *stream)
{
    COVA_REQUIRE(logits && labels && page_start && lists && acc_total && (loss_inout || dlogits) && B >= 1 && N >= 1);
    COVA_REQUIRE(NC >= 2 && NC <= COVA_MAX_CLASSES);
    COVA_REQUIRE((long long)B * (NC - 1) <= INT32_MAX);
    COVA_REQUIRE(rank_weight >= 0.0 && rank_weight <= DBL_MAX);
    const int grid = dlogits ? cdiv(N, RANK_THREADS) : 1;
    COVA_LAUNCH(rank_bwd_kernel, dim3(grid), dim3(RANK_THREADS), (hipStream_t)stream, logits, labels,
                page_start, B, N, NC, class_weight, ignore_index, has_ignore_index != 0, lists, acc_total,
                rank_weight, reduction_mean != 0, grad_scale, loss_inout, dlogits, accumulate != 0);
    return COVA_OK;
}
