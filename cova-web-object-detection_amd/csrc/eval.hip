// Evaluation of a whole split on the device (train.py:131-154 over every batch of a loader): the rank of the labelled box.
//   cova_eval_page_ranks: per page of the batch and class c >= 1, the position of the FIRST box labelled c in the order
//   cova_page_class_topk uses (ranks_before in rows.h: score descending, ties to the lower page-local index), scattered
//   into a split-resident table by page id.  "Among the top k" is then 0 <= rank < k for every k, and the per-batch host
//   fold of HotPathTrainer.evaluate's booleans becomes one device-to-host copy per split.
#include "rows.h"

namespace {

// One wave per (page of the batch, class 1..NC-1); a wave owns its table entries, so there is no atomic and no workspace.
// Pass 1 finds the first labelled box (lowest index) and the best box of the column; pass 2 counts the boxes that come
// before the labelled one.  The column is strided by NC floats: a page is a few hundred boxes, the second pass hits L2.
__global__ __launch_bounds__(256) void eval_page_ranks_kernel(const float *__restrict__ logits,
                                                              const int64_t *__restrict__ labels,
                                                              const int64_t *__restrict__ page_start,
                                                              const int *__restrict__ page_ids, int B, int NC, int P,
                                                              int *__restrict__ rank, int *__restrict__ top1)
{
    const int task = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (task >= B * (NC - 1)) return;
    const int page = task / (NC - 1), c = 1 + task - page * (NC - 1);
    const int row = page_ids ? page_ids[page] : page;
    if (row < 0 || row >= P) return;                       // the host validates ids; an id outside the table is skipped
    const int64_t lo = page_start[page], hi = page_start[page + 1];
    int t = RANK_NONE, bi = RANK_NONE;
    float bv = -INFINITY;
    for (int64_t n = lo + lane; n < hi; n += 64) {
        const int i = (int)(n - lo);
        if (labels[n] == (int64_t)c) t = min(t, i);
        const float v = logits[(size_t)n * NC + c];
        if (bi == RANK_NONE || v > bv) { bv = v; bi = i; }   // ascending i per lane: a tie keeps the lower index
    }
    t = wave_min_i(t);
    wave_ranked_first(bv, bi);
    int r = -1;
    if (t != RANK_NONE) {
        const float vt = logits[(size_t)(lo + t) * NC + c];
        int before = 0;
        for (int64_t n = lo + lane; n < hi; n += 64) {
            const float v = logits[(size_t)n * NC + c];
            const int i = (int)(n - lo);
            before += ranks_before(v, i, vt, t) ? 1 : 0;
        }
        r = wave_sum_i(before);
    }
    if (lane == 0) {
        const size_t at = (size_t)row * (NC - 1) + (c - 1);
        rank[at] = r;
        if (top1) top1[at] = (bi == RANK_NONE) ? -1 : bi;
    }
}

}  // namespace

COVA_API int cova_eval_page_ranks(const float *logits, const int64_t *labels, const int64_t *page_start,
                                  const int *page_ids, int B, int NC, int P, int *rank, int *top1, void *stream)
{
    COVA_REQUIRE(logits && labels && page_start && rank && B > 0 && NC >= 2 && NC <= COVA_MAX_CLASSES && P > 0);
    COVA_LAUNCH(eval_page_ranks_kernel, dim3(cdiv(B * (NC - 1), 4)), dim3(256), (hipStream_t)stream, logits,
                labels, page_start, page_ids, B, NC, P, rank, top1);
    return COVA_OK;
}
