// Configurable criterion of the trainer and of models.CrossEntropyLoss: cross-entropy with class
// weights, label smoothing, an ignore label and sum / mean reduction, or the focal loss, plus per-class counters kept on
// the device.  Two phases with the denominator in device memory between them (data parallelism all-reduces it there):
//   cova_ce_loss_fwd: per-row loss terms -> acc = {numerator, denominator, kept rows} in float64, pred, metrics;
//   cova_ce_loss_bwd: acc -> scalar loss and dlogits.
// Per-row arithmetic is ce_sum_kernel's (f32, expf / logf, first maximum wins); sums over rows are float64 over fixed
// slices of LOSS_SLICE rows folded in a fixed order, so the results depend on N alone: no float atomics, no host read.
// With no option set the rows' terms are ce_sum_kernel's bits (1.0f factors and +0 terms only).
#include "rows.h"

namespace {

constexpr int LOSS_THREADS = 1024;
constexpr int LOSS_ROWS = 2;          // rows per thread of the forward: a slice is one block's rows
constexpr int LOSS_SLICE = LOSS_THREADS * LOSS_ROWS;
constexpr int LOSS_BWD_THREADS = 256;
constexpr int N_ACC = 4;              // numerator, denominator, kept, bad labels

struct LossOpt {
    float c1;        // 1 - label_smoothing
    float eps_c;     // label_smoothing / NC
    float gamma;     // focal exponent (0: cross-entropy)
    long long ignore_index;
    int has_ignore;
};

// 1 - p_y as the sum of the other classes' probabilities: a saturated row gives 0, never a negative or a NaN
__device__ __forceinline__ float others_prob(const float *__restrict__ l, int NC, int y, float lse)
{
    float q = 0.f;
    for (int k = 0; k < NC; ++k)
        if (k != y) q += expf(l[k] - lse);
    return q;
}

// q^(gamma-1) of the focal term (q^gamma = that times q): gamma 1 and 2, the usual values, need no powf; powf(0, 0) = 1
// keeps gamma = 1 exact at a saturated row
__device__ __forceinline__ float focal_pow_m1(float q, float gamma)
{
    return gamma == 1.f ? 1.f : gamma == 2.f ? q : powf(q, gamma - 1.f);
}

// metrics (int64 words, M = NC*NC): [0, M) confusion[label][pred], [M] kept, [M+1] bad labels, [M+2], [M+3] the float64
// running sums of numerator and denominator.  One finisher per launch, launches are stream-ordered: plain updates.
__device__ __forceinline__ void finish(const double *t, double *__restrict__ acc, int64_t *__restrict__ metrics, int NC)
{
    acc[0] = t[0];
    acc[1] = t[1];
    acc[2] = t[2];
    if (metrics) {
        const int M = NC * NC;
        metrics[M] += (int64_t)t[2];
        metrics[M + 1] += (int64_t)t[3];
        double *f = reinterpret_cast<double *>(metrics + M + 2);
        f[0] += t[0];
        f[1] += t[1];
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void ce_loss_fwd_kernel(const float *__restrict__ logits,
                                                                   const int64_t *__restrict__ labels, int N, int NC,
                                                                   const float *__restrict__ weight, LossOpt o,
                                                                   double *__restrict__ partial, int n_part,
                                                                   double *__restrict__ acc, int64_t *__restrict__ pred,
                                                                   int64_t *__restrict__ metrics)
{
    __shared__ float s_w[COVA_MAX_CLASSES];
    __shared__ int s_conf[COVA_MAX_CLASSES * COVA_MAX_CLASSES];
    __shared__ double s_part[LOSS_THREADS / 64][N_ACC];
    if (threadIdx.x < NC) s_w[threadIdx.x] = weight ? weight[threadIdx.x] : 1.f;
    if (threadIdx.x < NC * NC) s_conf[threadIdx.x] = 0;
    __syncthreads();
    double t[N_ACC] = {0.0, 0.0, 0.0, 0.0};
    const int r0 = blockIdx.x * LOSS_SLICE;
#pragma unroll
    for (int j = 0; j < LOSS_ROWS; ++j) {
        const int n = r0 + j * LOSS_THREADS + threadIdx.x;
        if (n >= N) break;
        const float *l = logits + (size_t)n * NC;
        int am;
        const float lse = row_lse(l, NC, &am);
        if (pred) pred[n] = am;
        const long long lab = labels[n];
        const int state = label_state(lab, NC, o.ignore_index, o.has_ignore);
        if (state == 2) t[3] += 1.0;
        if (state != 0) continue;
        const int y = (int)lab;
        const float wy = s_w[y];
        float li;
        if (o.gamma == 0.f) {
            li = (o.c1 * wy) * (lse - l[y]);
            if (o.eps_c != 0.f) {
                float sm = 0.f;
                for (int k = 0; k < NC; ++k) sm += s_w[k] * (lse - l[k]);
                li += o.eps_c * sm;
            }
        } else {
            const float q = others_prob(l, NC, y, lse);
            li = wy * (focal_pow_m1(q, o.gamma) * q) * (lse - l[y]);
        }
        t[0] += (double)li;
        t[1] += (double)wy;
        t[2] += 1.0;
        if (metrics) atomicAdd(&s_conf[y * NC + am], 1);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < N_ACC; ++j) {
        const double s = wave_sum_f64(t[j]);
        if (lane == 0) s_part[wave][j] = s;
    }
    __syncthreads();
    if (metrics && threadIdx.x < NC * NC && s_conf[threadIdx.x] != 0)     // integer adds: any order, same result
        atomicAdd(reinterpret_cast<unsigned long long *>(metrics) + threadIdx.x,
                  (unsigned long long)s_conf[threadIdx.x]);
    if (threadIdx.x == 0) {
        double s[N_ACC];
        for (int j = 0; j < N_ACC; ++j) {
            s[j] = 0.0;
            for (int w = 0; w < LOSS_THREADS / 64; ++w) s[j] += s_part[w][j];
        }
        if (n_part == 1) finish(s, acc, metrics, NC);
        else
            for (int j = 0; j < N_ACC; ++j) partial[(size_t)blockIdx.x * N_ACC + j] = s[j];
    }
}

// more than one slice: one wave folds the slices' partials (lane i: slices i, i + 64, ... in turn; then the butterfly)
__global__ __launch_bounds__(64) void ce_loss_fold_kernel(const double *__restrict__ partial, int n_part,
                                                          double *__restrict__ acc, int64_t *__restrict__ metrics,
                                                          int NC)
{
    double s[N_ACC];
#pragma unroll
    for (int j = 0; j < N_ACC; ++j) {
        double a = 0.0;
        for (int i = threadIdx.x; i < n_part; i += 64) a += partial[(size_t)i * N_ACC + j];
        s[j] = wave_sum_f64(a);
    }
    if (threadIdx.x == 0) finish(s, acc, metrics, NC);
}

// one row per thread; block 0 also writes the scalar loss.  mean: a zero denominator gives loss 0 and dlogits 0.
__global__ __launch_bounds__(LOSS_BWD_THREADS) void ce_loss_bwd_kernel(const float *__restrict__ logits,
                                                                       const int64_t *__restrict__ labels, int N,
                                                                       int NC, const float *__restrict__ weight,
                                                                       LossOpt o, const double *__restrict__ acc,
                                                                       int mean, const float *__restrict__ grad_scale,
                                                                       float *__restrict__ loss,
                                                                       float *__restrict__ dlogits)
{
    __shared__ float s_w[COVA_MAX_CLASSES];
    if (threadIdx.x < NC) s_w[threadIdx.x] = weight ? weight[threadIdx.x] : 1.f;
    __syncthreads();
    const double num = acc[0], den = acc[1];
    if (loss && blockIdx.x == 0 && threadIdx.x == 0) loss[0] = mean ? (den > 0.0 ? (float)(num / den) : 0.f) : (float)num;
    if (!dlogits) return;
    const int n = blockIdx.x * LOSS_BWD_THREADS + threadIdx.x;
    if (n >= N) return;
    float s = mean ? (den > 0.0 ? (float)(1.0 / den) : 0.f) : 1.f;
    if (grad_scale) s *= grad_scale[0];
    const float *l = logits + (size_t)n * NC;
    float *d = dlogits + (size_t)n * NC;
    const long long lab = labels[n];
    if (label_state(lab, NC, o.ignore_index, o.has_ignore) != 0) {
        for (int k = 0; k < NC; ++k) d[k] = 0.f;
        return;
    }
    int am;
    const float lse = row_lse(l, NC, &am);
    const int y = (int)lab;
    const float wy = s_w[y];
    if (o.gamma == 0.f) {
        // d/dl_k of (1-eps) w_y (lse - l_y) + (eps/C) sum_j w_j (lse - l_j) = A p_k - t_k
        const float hit = o.c1 * wy;
        float A = hit;
        if (o.eps_c != 0.f) {
            float sw = 0.f;
            for (int k = 0; k < NC; ++k) sw += s_w[k];
            A += o.eps_c * sw;
        }
        for (int k = 0; k < NC; ++k) {
            float tk = k == y ? hit : 0.f;
            if (o.eps_c != 0.f) tk += o.eps_c * s_w[k];
            d[k] = s * (A * expf(l[k] - lse) - tk);
        }
    } else {
        // w_y (p_k - [k == y]) (1-p_y)^(g-1) ((1-p_y) - g p_y log p_y), with p_y - 1 taken as -(1 - p_y)
        const float q = others_prob(l, NC, y, lse);
        const float logp = l[y] - lse;
        const float f = wy * focal_pow_m1(q, o.gamma) * (q - o.gamma * expf(logp) * logp);
        for (int k = 0; k < NC; ++k) d[k] = s * (f * (k == y ? -q : expf(l[k] - lse)));
    }
}

inline bool loss_options(int NC, double label_smoothing, double focal_gamma, long long ignore_index,
                         int has_ignore_index, LossOpt *o)
{
    if (!(NC > 0 && NC <= COVA_MAX_CLASSES)) return false;
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0)) return false;
    if (!(focal_gamma == 0.0 || focal_gamma >= 1.0)) return false;
    if (focal_gamma != 0.0 && label_smoothing != 0.0) return false;
    o->c1 = (float)(1.0 - label_smoothing);
    o->eps_c = (float)(label_smoothing / NC);
    o->gamma = (float)focal_gamma;
    o->ignore_index = ignore_index;
    o->has_ignore = has_ignore_index != 0;
    return true;
}

}  // namespace

// doubles of cova_ce_loss_fwd's workspace for N rows (four per slice of its first launch)
COVA_API int cova_ce_loss_workspace_doubles(int N)
{
    return N_ACC * (N > 0 ? cdiv(N, LOSS_SLICE) : 1);
}

COVA_API int cova_ce_loss_fwd(const float *logits, const int64_t *labels, int N, int NC, const float *class_weight,
                              double label_smoothing, double focal_gamma, long long ignore_index, int has_ignore_index,
                              double *acc, int64_t *pred, int64_t *metrics, double *workspace, void *stream)
{
    LossOpt o;
    COVA_REQUIRE(logits && labels && acc && workspace && N > 0);
    COVA_REQUIRE(loss_options(NC, label_smoothing, focal_gamma, ignore_index, has_ignore_index, &o));
    const int n_part = cdiv(N, LOSS_SLICE);
    hipStream_t s = (hipStream_t)stream;
    COVA_LAUNCH(ce_loss_fwd_kernel, dim3(n_part), dim3(LOSS_THREADS), s, logits, labels, N, NC, class_weight,
                o, workspace, n_part, acc, pred, metrics);
    if (n_part > 1) {
        COVA_LAUNCH(ce_loss_fold_kernel, dim3(1), dim3(64), s, workspace, n_part, acc, metrics, NC);
    }
    return COVA_OK;
}

COVA_API int cova_ce_loss_bwd(const float *logits, const int64_t *labels, int N, int NC, const float *class_weight,
                              double label_smoothing, double focal_gamma, long long ignore_index, int has_ignore_index,
                              const double *acc_total, int reduction_mean, const float *grad_scale, float *loss_out,
                              float *dlogits, void *stream)
{
    LossOpt o;
    COVA_REQUIRE(logits && labels && acc_total && (loss_out || dlogits) && N > 0);
    COVA_REQUIRE(loss_options(NC, label_smoothing, focal_gamma, ignore_index, has_ignore_index, &o));
    const int grid = dlogits ? cdiv(N, LOSS_BWD_THREADS) : 1;
    COVA_LAUNCH(ce_loss_bwd_kernel, dim3(grid), dim3(LOSS_BWD_THREADS), (hipStream_t)stream, logits, labels,
                N, NC, class_weight, o, acc_total, reduction_mean, grad_scale, loss_out, dlogits);
    return COVA_OK;
}
