// Per-page hard-negative mining for the criterion: after the forward every page keeps its
// positives and the k hardest background boxes, k = max(min_keep, floor(ratio * positives)); the other background boxes
// get the criterion's ignore label and stay graph context.  The score is the plain cross-entropy against background,
// lse - l[0], with row_lse (rows.h); it becomes an integer key and the rank is a count, as in eval.hip and
// sample.hip: no atomics, no host read, one launch, a function of the inputs alone.
//   mine_select_kernel  one block per page: scores and keys of the page's rows (keys in an LDS tile), the page's counts
//                       and quota, then one thread per background row counts the rows that rank before it with broadcast
//                       reads of the tile.  A page of more than MINE_TILE rows walks its keys tile by tile, recomputing
//                       them from the logits (n / MINE_THREADS passes: the counting itself stays the larger cost).
#include "rows.h"

namespace {

constexpr int MINE_THREADS = 256;
constexpr int MINE_TILE = 2048;           // keys per LDS tile (8 KiB); a page of the reference's data (11-230 boxes) is one tile
constexpr unsigned MINE_NAN_KEY = 0x7FC00000u;

__device__ __forceinline__ float mine_score(const float *__restrict__ logits, int row, int NC)
{
    const float *l = logits + (size_t)row * NC;
    int am;
    return row_lse(l, NC, &am) - l[0];
}

// NaN ranks above +inf (a broken forward stays in the loss), s <= 0 (rounding, -0) is the easiest
__device__ __forceinline__ unsigned mine_key(float s)
{
    return s != s ? MINE_NAN_KEY : s > 0.f ? __float_as_uint(s) : 0u;
}

// the tile's word of a row: key + 1 for a background row, 0 for every other row and for the padding, so that a word of 0
// never ranks before a background row
__device__ __forceinline__ unsigned mine_word(float s, long long lab) { return lab == 0 ? mine_key(s) + 1u : 0u; }

// how many of the four words w of rows j .. j + 3 rank before row i with word wi >= 1: w > wi, or w == wi at a lower row
// (w >= wi is w > wi - 1).  One address for the whole wave: the caller's read of w is a broadcast read.
__device__ __forceinline__ int mine_before(uint4 w, unsigned wi, int j, int i)
{
    return (w.x > (j < i ? wi - 1u : wi) ? 1 : 0) + (w.y > (j + 1 < i ? wi - 1u : wi) ? 1 : 0) +
           (w.z > (j + 2 < i ? wi - 1u : wi) ? 1 : 0) + (w.w > (j + 3 < i ? wi - 1u : wi) ? 1 : 0);
}

// rows outside every page: label and score pass through
__device__ __forceinline__ void mine_pass_through(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                  int lo, int hi, int NC, int64_t *__restrict__ labels_out,
                                                  float *__restrict__ score_out)
{
    for (int n = lo + (int)threadIdx.x; n < hi; n += MINE_THREADS) {
        labels_out[n] = labels[n];
        if (score_out) score_out[n] = mine_score(logits, n, NC);
    }
}

__global__ __launch_bounds__(MINE_THREADS) void mine_select_kernel(
    const float *__restrict__ logits, const int64_t *__restrict__ labels, const int64_t *__restrict__ page_start, int B,
    int N, int NC, double ratio, int min_keep, long long drop_label, int64_t *__restrict__ labels_out,
    float *__restrict__ score_out, int *__restrict__ counts)
{
    __shared__ __attribute__((aligned(16))) unsigned tile[MINE_TILE];
    __shared__ int wave_cnt[MINE_THREADS / 64][2];
    const int p = blockIdx.x, tid = threadIdx.x;
    const PageRows pr = page_rows(page_start, p, N);
    const int base = pr.base, end = pr.end, n = end - base;
    if (p == 0) mine_pass_through(logits, labels, 0, base, NC, labels_out, score_out);
    if (p == B - 1) mine_pass_through(logits, labels, end, N, NC, labels_out, score_out);
    const bool one_tile = n <= MINE_TILE;

    // scores, the default of labels_out (kept), the page's counts; a one-tile page also fills its tile
    int n_pos = 0, n_bg = 0;
    for (int i = tid; i < n; i += MINE_THREADS) {
        const float s = mine_score(logits, base + i, NC);
        const long long lab = labels[base + i];
        if (score_out) score_out[base + i] = s;
        labels_out[base + i] = lab;
        n_pos += (lab >= 1 && lab < NC) ? 1 : 0;
        n_bg += lab == 0 ? 1 : 0;
        if (one_tile) tile[i] = mine_word(s, lab);
    }
    if (one_tile && tid < 4 && n + tid < ((n + 3) & ~3)) tile[n + tid] = 0u;           // pad to whole uint4 reads
    n_pos = wave_sum_i(n_pos);
    n_bg = wave_sum_i(n_bg);
    if ((tid & 63) == 0) {
        wave_cnt[tid >> 6][0] = n_pos;
        wave_cnt[tid >> 6][1] = n_bg;
    }
    __syncthreads();
    n_pos = n_bg = 0;
#pragma unroll
    for (int w = 0; w < MINE_THREADS / 64; ++w) {
        n_pos += wave_cnt[w][0];
        n_bg += wave_cnt[w][1];
    }
    const double q = fmax((double)min_keep, floor(ratio * (double)n_pos));
    const int k_p = q >= (double)n_bg ? n_bg : (int)q;
    if (counts && tid == 0) {
        counts[p * 3 + 0] = n_pos;
        counts[p * 3 + 1] = n_bg;
        counts[p * 3 + 2] = k_p;
    }
    if (k_p >= n_bg) return;                         // every background row is kept (block-uniform)

    // thread tid ranks rows tid, tid + MINE_THREADS, ...: the rows whose labels_out it wrote above
    const uint4 *tile4 = reinterpret_cast<const uint4 *>(tile);
    for (int i0 = 0; i0 < n; i0 += MINE_THREADS) {
        const int i = i0 + tid;
        const bool live = i < n;
        const unsigned wi = !live ? 0u : one_tile ? tile[i] : mine_word(mine_score(logits, base + i, NC), labels[base + i]);
        int rank = 0;
        if (k_p > 0)
            for (int j0 = 0; j0 < n; j0 += MINE_TILE) {
                const int tn = min(MINE_TILE, n - j0), tn4 = (tn + 3) >> 2;
                if (!one_tile) {
                    __syncthreads();                 // the previous tile has been read by everyone
                    for (int t = tid; t < 4 * tn4; t += MINE_THREADS)
                        tile[t] = t < tn ? mine_word(mine_score(logits, base + j0 + t, NC), labels[base + j0 + t]) : 0u;
                    __syncthreads();
                }
                if (wi != 0u) {                      // four waves a block: four tile reads in flight per round
                    int t = 0;
                    for (; t + 4 <= tn4; t += 4) {
                        const uint4 a = tile4[t], b = tile4[t + 1], c = tile4[t + 2], d = tile4[t + 3];
                        const int j = j0 + 4 * t;
                        rank += mine_before(a, wi, j, i) + mine_before(b, wi, j + 4, i) + mine_before(c, wi, j + 8, i) +
                                mine_before(d, wi, j + 12, i);
                    }
                    for (; t < tn4; ++t) rank += mine_before(tile4[t], wi, j0 + 4 * t, i);
                }
            }
        if (wi != 0u && rank >= k_p) labels_out[base + i] = drop_label;
    }
}

}  // namespace

COVA_API int cova_hard_negative_select(const float *logits, const int64_t *labels, const int64_t *page_start, int B, int N,
                                       int NC, double ratio, int min_keep, long long drop_label, int64_t *labels_out,
                                       float *score_out, int *counts, void *stream)
{
    COVA_REQUIRE(logits && labels && page_start && labels_out && B >= 1 && N >= 1);
    COVA_REQUIRE(NC >= 2 && NC <= COVA_MAX_CLASSES);
    COVA_REQUIRE(ratio >= 0.0 && ratio <= DBL_MAX && min_keep >= 0);
    COVA_LAUNCH(mine_select_kernel, dim3(B), dim3(MINE_THREADS), (hipStream_t)stream, logits, labels, page_start,
                B, N, NC, ratio, min_keep, drop_label, labels_out, score_out, counts);
    return COVA_OK;
}
