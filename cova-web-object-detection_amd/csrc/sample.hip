// Background-box sampling of WebDataset.__getitem__ (datasets.py:101-110) and the collation of the surviving boxes
// (datasets.py:112-128,159-178), on the device.  The reference draws np.random.permutation(n)[:int(sf*n)], adds every
// labelled box and sorts; here each box gets an integer key, the m = int(sf*n) smallest (key, index) pairs are the draw,
// and the kept boxes are compacted in ascending order.  Integer and byte work only, no atomics: bit-deterministic.
//   sample_mark_kernel    one block per page: keys in LDS tiles, rank by counting, block-wide exclusive scan of the keep
//                         flags; kept source row ids, page-locally compacted, and the page's kept count go to the workspace
//   sample_compact_kernel one block per page: sums the counts of the pages before it (cross-page offsets) and moves the
//                         page's list to its final place
//   collate_selected_kernel  cova_collate_boxes' thread-per-(box, slot) layout over the kept boxes
#include "common.h"

namespace {

constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_TILE = 2048;          // keys per LDS tile (16 KiB); a page of the reference's data (11-230 boxes) is one tile

// key of box i of dataset page `pid` in the stream `stream_seed`: 63 bits of the counter hash (include/cova_hip.h)
__device__ __forceinline__ long long sample_key(unsigned long long stream_seed, unsigned long long pid, int i)
{
    return (long long)(hash_mix64(hash_mix64(stream_seed, pid), (unsigned long long)i) >> 1);
}

// exclusive scan of one 0/1 flag per thread over the block (4 waves of 64); *total = number of flags set
__device__ __forceinline__ int block_excl_scan_flag(bool flag, int *wave_tot, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();                       // wave_tot of the previous call has been read by everyone
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_THREADS / 64; ++w) {
        const int t = wave_tot[w];
        if (w < wave) base += t;
        tot += t;
    }
    *total = tot;
    return base + before;
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_mark_kernel(
    const float *__restrict__ rows, const int *__restrict__ page_offsets, const int *__restrict__ row_starts,
    const int *__restrict__ page_ids, const int *__restrict__ keep_counts, int N,
    const long long *__restrict__ keys, unsigned long long stream_seed, int *__restrict__ local_sel,
    int *__restrict__ counts)
{
    __shared__ long long tile[SAMPLE_TILE];
    __shared__ int wave_tot[SAMPLE_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int base = page_offsets[p], n = page_offsets[p + 1] - base, m = keep_counts[p];
    const int src0 = row_starts ? row_starts[p] : base;
    const unsigned long long pid = page_ids ? (unsigned long long)page_ids[p] : (unsigned long long)p;
    if (n <= 0 || base < 0 || base + n > N) {          // an empty page; a malformed table writes nothing
        if (tid == 0) counts[p] = 0;
        return;
    }
    const bool one_tile = n <= SAMPLE_TILE;
    int kept_before = 0;
    for (int i0 = 0; i0 < n; i0 += SAMPLE_THREADS) {
        const int i = i0 + tid;
        const bool live = i < n;
        const long long ki = !live ? 0 : keys ? keys[base + i] : sample_key(stream_seed, pid, i);
        int rank = 0;
        for (int j0 = 0; j0 < n; j0 += SAMPLE_TILE) {
            const int tn = min(SAMPLE_TILE, n - j0);
            if (!one_tile || i0 == 0) {
                __syncthreads();
                for (int t = tid; t < tn; t += SAMPLE_THREADS)
                    tile[t] = keys ? keys[base + j0 + t] : sample_key(stream_seed, pid, j0 + t);
                __syncthreads();
            }
            if (live)
                for (int t = 0; t < tn; ++t) {
                    const long long kj = tile[t];
                    rank += (kj < ki || (kj == ki && j0 + t < i)) ? 1 : 0;
                }
        }
        const bool keep = live && (rank < m || rows[(long long)(src0 + i) * 5 + 4] != 0.f);     // datasets.py:106
        int tot;
        const int pos = block_excl_scan_flag(keep, wave_tot, &tot);
        if (keep) local_sel[base + kept_before + pos] = src0 + i;
        kept_before += tot;
    }
    if (tid == 0) counts[p] = kept_before;
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_compact_kernel(
    const int *__restrict__ page_offsets, const int *__restrict__ local_sel, const int *__restrict__ counts, int B, int N,
    int *__restrict__ sel, int *__restrict__ out_offsets)
{
    __shared__ int wave_tot[SAMPLE_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    int s = 0;
    for (int q = tid; q < p; q += SAMPLE_THREADS) s += counts[q];
    s = wave_sum_i(s);
    if ((tid & 63) == 0) wave_tot[tid >> 6] = s;
    __syncthreads();
    int start = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_THREADS / 64; ++w) start += wave_tot[w];
    const int cnt = counts[p], base = page_offsets[p];
    if (tid == 0) {
        if (p == 0) out_offsets[0] = 0;
        out_offsets[p + 1] = start + cnt;
    }
    if (base < 0 || base + cnt > N || start + cnt > N) return;
    for (int k = tid; k < cnt; k += SAMPLE_THREADS) sel[start + k] = local_sel[base + k];
}

// one thread per (kept box, slot): slot < K writes a neighbour id, slot == K the box row, label and additional features
__global__ __launch_bounds__(256) void collate_selected_kernel(
    const float *__restrict__ rows, const int *__restrict__ sel, const int *__restrict__ out_offsets, int B, int cs,
    float *__restrict__ bboxes, long long *__restrict__ labels, long long *__restrict__ ctx,
    const float *__restrict__ addl_in, int A, float *__restrict__ addl_out, int N_out)
{
    const int K = 2 * cs;
    const long long total = (long long)N_out * (K + 1);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(t / (K + 1)), slot = (int)(t - (long long)g * (K + 1));
        int lo = 0, hi = B;                        // page of kept box g: out_offsets[lo] <= g < [lo+1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (out_offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const int base = out_offsets[lo], n = out_offsets[lo + 1] - base, i = g - base;
        if (slot == K) {
            const float *r = rows + (long long)sel[g] * 5;
            const float x = r[0], y = r[1];
            bboxes[g * 5 + 0] = (float)lo;
            bboxes[g * 5 + 1] = x;
            bboxes[g * 5 + 2] = y;
            bboxes[g * 5 + 3] = x + r[2];                      // datasets.py:115, float32 add
            bboxes[g * 5 + 4] = y + r[3];
            labels[g] = (long long)r[4];                       // torch.LongTensor(float) truncates
            for (int a = 0; a < A; ++a) addl_out[(long long)g * A + a] = addl_in[(long long)sel[g] * A + a];
        } else {
            // neighbours among the KEPT boxes (datasets.py:117-128 runs after the sampling)
            const int nleft = min(i, cs), nright = min(n - 1 - i, cs);
            long long v = -1;
            if (slot < nleft) v = base + (i - nleft + slot);
            else if (slot < nleft + nright) v = base + (i + 1 + (slot - nleft));
            ctx[(long long)g * K + slot] = v;
        }
    }
}

}  // namespace

COVA_API int cova_sample_boxes_workspace_ints(int B, int N) { return (B > 0 ? B : 0) + (N > 0 ? N : 0); }

COVA_API int cova_sample_boxes(const float *rows, const int *page_offsets, const int *row_starts, const int *page_ids,
                               const int *keep_counts, int B, int N, const long long *keys,
                               unsigned long long stream_seed, int *workspace, int *sel, int *out_offsets, void *stream)
{
    COVA_REQUIRE(page_offsets && keep_counts && workspace && out_offsets && B > 0 && N >= 0);
    COVA_REQUIRE(N == 0 || (rows && sel));
    hipStream_t st = (hipStream_t)stream;
    int *local_sel = workspace, *counts = workspace + N;
    COVA_LAUNCH(sample_mark_kernel, dim3(B), dim3(SAMPLE_THREADS), st, rows, page_offsets, row_starts, page_ids,
                keep_counts, N, keys, stream_seed, local_sel, counts);
    COVA_LAUNCH(sample_compact_kernel, dim3(B), dim3(SAMPLE_THREADS), st, page_offsets, local_sel, counts, B, N,
                sel, out_offsets);
    return COVA_OK;
}

COVA_API int cova_collate_selected(const float *rows, const int *sel, const int *out_offsets, int B, int N_out,
                                   int context_size, float *bboxes, long long *labels, long long *ctx, const float *addl_in,
                                   int A, float *addl_out, void *stream)
{
    COVA_REQUIRE(out_offsets && B > 0 && N_out >= 0 && context_size >= 0 && A >= 0);
    if (N_out == 0) return COVA_OK;
    COVA_REQUIRE(rows && sel && bboxes && labels);
    COVA_REQUIRE(context_size == 0 || ctx);
    COVA_REQUIRE(A == 0 || (addl_in && addl_out));
    COVA_LAUNCH(collate_selected_kernel, dim3(grid_for((long long)N_out * (2 * context_size + 1))), dim3(256),
                (hipStream_t)stream, rows, sel, out_offsets, B, context_size, bboxes, labels, ctx, addl_in, A,
                addl_out, N_out);
    return COVA_OK;
}
