// Parameter-group optimizers and the global gradient norm of HotPathTrainer (trainer.py): torch.optim.Adam (L2 added to the
// gradient), AdamW and SGD (momentum, dampening, nesterov) over a table of flat-buffer segments with per-group
// hyper-parameters, and torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) as two deterministic launches.
// Also the averaged copy of the weights (EMA / equal-weight running mean, HotPathTrainer(average=)) and the accumulation of
// the gradient bucket over micro-batches (HotPathTrainer(accumulate_steps=)) over the same table.
//
// Segment table: int64 rows {lo, hi, group, start}.  Row r covers flat elements [lo, hi) of every buffer; `start` is the
// sum of the lengths of the rows before it, so the rows tile one concatenated index space [0, total).  A block owns a
// fixed slice of that space, finds the row its slice begins in with one parallel pass over the table and walks on from
// there.  Frozen tensors are simply not in the table.
//
// Every kernel over the table is the one walk (for_each_piece) around the one element loop (for_each_element) around an
// operation struct with a four(i) and a one(i) body: a new flat-bucket kernel is a new operation, not a new walk.
#include "common.h"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_SLICE = 2048;      // concatenated elements per optimizer block: two float4 per thread
constexpr int NORM_SLICE = 4096;     // concatenated elements per norm partial: four float4 per thread
constexpr int MAX_GROUPS = 16;

enum { ALGO_ADAM = 0, ALGO_ADAMW = 1, ALGO_SGD = 2 };

// one parameter group in the form the update uses; converted from the host's doubles exactly as cova_adam_step does
struct OptGroup {
    float lr, wd, beta1, beta2, eps;
    float bc1, bc2_sqrt;             // 1 - beta1^step, sqrt(1 - beta2^step), in double on the host
    float decay;                     // adamw: 1 - lr * wd, in double on the host (torch: param.mul_(1 - lr * wd))
    float momentum, damp1;           // sgd: damp1 = 1 - dampening, in double on the host (torch: add_(g, alpha=1 - d))
    int nesterov, has_buf;           // sgd: has_buf = 0 on a group's first momentum step (buf = clone(g))
};

struct OptGroups {                   // by value: read from the kernel arguments, no copy to the device
    OptGroup g[MAX_GROUPS];
};

__device__ __forceinline__ const long long *seg_row(const long long *seg, int r) { return seg + 4 * (long long)r; }

struct FirstRow {
    int r;
    long long row[4];
};

// the row whose concatenated range holds v (exactly one row does in a valid table; r = n_seg if none), with its entries:
// the block starts on it without a second dependent load
__device__ __forceinline__ int find_first_row(const long long *__restrict__ seg, int n_seg, long long v, FirstRow *s)
{
    if (threadIdx.x == 0) s->r = n_seg;
    __syncthreads();
    for (int r = threadIdx.x; r < n_seg; r += blockDim.x) {
        const long long *row = seg_row(seg, r);
        const long long lo = row[0], hi = row[1], g = row[2], st = row[3];
        if (hi > lo && st <= v && v < st + (hi - lo)) {
            s->r = r;
            s->row[0] = lo; s->row[1] = hi; s->row[2] = g; s->row[3] = st;
        }
    }
    __syncthreads();
    return s->r;
}

__device__ __forceinline__ const long long *row_at(const long long *seg, int r, int first, const FirstRow &s)
{
    return r == first ? s.row : seg_row(seg, r);
}

// The Adam moments and step, rounding for rounding as adam_kernel (head.hip) compiles: the L2 term and the final step
// are fused multiply-adds, the moment updates and `+ eps` round every product and sum.  No contraction here (HIP's
// __fmul_rn / __fadd_rn are plain operators the backend may fuse), the fused ones are explicit fmaf: one group of
// ALGO_ADAM gives the bits of cova_adam_step.
__device__ __forceinline__ void adam_moments_and_step(float &pv, float gv, float &mv, float &vv, const OptGroup &q)
{
#pragma clang fp contract(off)
    const float mn = q.beta1 * mv + (1.f - q.beta1) * gv;
    const float vn = q.beta2 * vv + (1.f - q.beta2) * gv * gv;
    mv = mn;
    vv = vn;
    const float denom = sqrtf(vn) / q.bc2_sqrt + q.eps;
    pv = fmaf(-(q.lr / q.bc1), mn / denom, pv);
}

template <int ALGO>
__device__ __forceinline__ void update(float &pv, float gv, float &mv, float &vv, const OptGroup &q)
{
#pragma clang fp contract(off)
    if (ALGO == ALGO_ADAM) {
        adam_moments_and_step(pv, fmaf(q.wd, pv, gv), mv, vv, q);
    } else if (ALGO == ALGO_ADAMW) {
        pv = pv * q.decay;                     // its own rounding, as torch's separate mul_
        adam_moments_and_step(pv, gv, mv, vv, q);
    } else {
        if (q.wd != 0.f) gv = gv + q.wd * pv;
        if (q.momentum != 0.f) {
            const float b = q.has_buf ? q.momentum * mv + q.damp1 * gv : gv;
            mv = b;
            gv = q.nesterov ? gv + q.momentum * b : b;
        }
        pv = pv - q.lr * gv;
    }
}

// The walk of a block over its slice of SLICE concatenated elements: start() behind the table scan, then f(a, b, group) per
// valid flat piece [a, b) of a row, in table order.  A malformed row (outside [0, n), or behind the position reached) is skipped.
template <int SLICE, class Start, class Piece>
__device__ __forceinline__ void for_each_piece(const long long *__restrict__ seg, int n_seg, long long total, long long n,
                                               FirstRow *s_first, Start start, Piece f)
{
    const long long v0 = (long long)blockIdx.x * SLICE;
    const long long v1 = v0 + SLICE < total ? v0 + SLICE : total;
    const int first = find_first_row(seg, n_seg, v0, s_first);
    start();
    for (long long pos = v0, r = first; pos < v1 && r < n_seg; ++r) {
        const long long *row = row_at(seg, (int)r, first, *s_first);
        const long long lo = row[0], hi = row[1], st = row[3];
        const long long end = st + (hi - lo) < v1 ? st + (hi - lo) : v1;
        if (lo >= 0 && hi <= n && pos >= st) f(lo + (pos - st), lo + (end - st), (int)row[2]);
        pos = end;
    }
}

// Flat elements [a, b) of one piece: op.four(i) on float4s when the buffers are 16-byte aligned (vec4) and the piece begins
// and ends on a multiple of four, else op.one(i); a thread's elements and their order are the same for every operation.
template <class Op>
__device__ __forceinline__ void for_each_element(long long a, long long b, bool vec4, Op &op)
{
    if (vec4 && ((a | b) & 3) == 0) {
        for (long long i = a + 4 * (long long)threadIdx.x; i < b; i += 4 * OPT_THREADS) op.four(i);
        return;
    }
    for (long long i = a + threadIdx.x; i < b; i += OPT_THREADS) op.one(i);
}

// update<ALGO> of one group over (p, g, m, v); gscale (nullable) is the clip coefficient, multiplied into g on load
template <int ALGO>
struct UpdateOp {
    float *p, *m, *v;
    const float *g;
    const OptGroup &q;
    bool has_m, scaled;              // has_m: every algorithm but sgd without momentum keeps a first moment / buffer
    float gs;
    static constexpr bool has_v = ALGO != ALGO_SGD;

    __device__ __forceinline__ void four(long long i) const
    {
#pragma clang fp contract(off)
        float4 pv = *reinterpret_cast<const float4 *>(p + i);
        float4 gv = *reinterpret_cast<const float4 *>(g + i);
        float4 mv = has_m ? *reinterpret_cast<const float4 *>(m + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 vv = has_v ? *reinterpret_cast<const float4 *>(v + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (scaled) {
            gv.x = gv.x * gs; gv.y = gv.y * gs;
            gv.z = gv.z * gs; gv.w = gv.w * gs;
        }
        update<ALGO>(pv.x, gv.x, mv.x, vv.x, q);
        update<ALGO>(pv.y, gv.y, mv.y, vv.y, q);
        update<ALGO>(pv.z, gv.z, mv.z, vv.z, q);
        update<ALGO>(pv.w, gv.w, mv.w, vv.w, q);
        *reinterpret_cast<float4 *>(p + i) = pv;
        if (has_m) *reinterpret_cast<float4 *>(m + i) = mv;
        if (has_v) *reinterpret_cast<float4 *>(v + i) = vv;
    }

    __device__ __forceinline__ void one(long long i) const
    {
#pragma clang fp contract(off)
        float pv = p[i], gv = g[i];
        float mv = has_m ? m[i] : 0.f, vv = has_v ? v[i] : 0.f;
        if (scaled) gv = gv * gs;
        update<ALGO>(pv, gv, mv, vv, q);
        p[i] = pv;
        if (has_m) m[i] = mv;
        if (has_v) v[i] = vv;
    }
};

// (the buffers as __restrict__ parameters: as struct members alone the qualifier is lost and the sgd loops compile longer)
template <int ALGO>
__device__ __forceinline__ void update_range(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                             float *__restrict__ v, long long a, long long b, const OptGroup &q,
                                             bool scaled, float gs, bool vec4)
{
    UpdateOp<ALGO> op = {p, m, v, g, q, ALGO != ALGO_SGD || q.momentum != 0.f, scaled, gs};
    for_each_element(a, b, vec4, op);
}

template <int ALGO>
__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                                float *__restrict__ m, float *__restrict__ v,
                                                                long long n, const long long *__restrict__ seg,
                                                                int n_seg, long long total, OptGroups G, int n_groups,
                                                                const float *__restrict__ gscale, int vec4)
{
    __shared__ FirstRow s_first;
    float gs;     // read behind the table scan: ahead of it the load and its null test stand alone, +0.2 us on a 6 us launch
    for_each_piece<OPT_SLICE>(seg, n_seg, total, n, &s_first, [&] { gs = gscale ? *gscale : 1.f; },
                              [&](long long a, long long b, int grp) {
        grp = grp < 0 ? 0 : (grp >= n_groups ? n_groups - 1 : grp);
        update_range<ALGO>(p, g, m, v, a, b, G.g[grp], gscale != nullptr, gs, vec4 != 0);
    });
}

// double-precision sum over the block in a fixed order (wave butterflies, then the waves in index order)
__device__ __forceinline__ double block_sum(double x, double *s_wave)
{
    x = wave_sum_f64(x);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < OPT_THREADS / 64; ++w) t += s_wave[w];
    return t;
}

// this thread's sum of g^2 in double, in the order for_each_element hands the elements out
struct SumSqOp {
    const float *g;
    double acc;

    __device__ __forceinline__ void four(long long i)
    {
        const float4 x = *reinterpret_cast<const float4 *>(g + i);
        acc += (double)x.x * x.x;
        acc += (double)x.y * x.y;
        acc += (double)x.z * x.z;
        acc += (double)x.w * x.w;
    }

    __device__ __forceinline__ void one(long long i)
    {
        const double x = g[i];
        acc += x * x;
    }
};

// stage 1: partial[b] = sum of g^2 (in double) over concatenated elements [b * NORM_SLICE, (b + 1) * NORM_SLICE)
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(const float *__restrict__ g, long long n,
                                                                const long long *__restrict__ seg, int n_seg,
                                                                long long total, int vec4, double *__restrict__ partial)
{
    __shared__ FirstRow s_first;
    __shared__ double s_wave[OPT_THREADS / 64];
    SumSqOp op = {g, 0.0};
    for_each_piece<NORM_SLICE>(seg, n_seg, total, n, &s_first, [] {},
                               [&](long long a, long long b, int) { for_each_element(a, b, vec4 != 0, op); });
    const double t = block_sum(op.acc, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// stage 2: fold the partials in a fixed order (thread t: partials t, t + 256, ... in turn; then block_sum) and write
// out[0] = sqrt(sum) (torch's total_norm) and out[1] = clamp(max_norm / (norm + 1e-6), max=1) in f32 as clip_grad_norm_
// computes it (a python float over a tensor is reciprocal() * max_norm: two roundings) -- a NaN norm gives a NaN
// coefficient (torch.clamp propagates it), an infinite one 0.  (A last-block fold inside stage 1 measured slower: its
// agent-scope loads of the partials are serial.)
__global__ __launch_bounds__(OPT_THREADS) void grad_norm_finish_kernel(const double *__restrict__ partial, int n_part,
                                                                      float max_norm, float *__restrict__ out)
{
    __shared__ double s_wave[OPT_THREADS / 64];
    double acc = 0.0;
    for (int j = threadIdx.x; j < n_part; j += OPT_THREADS) acc += partial[j];
    const double t = block_sum(acc, s_wave);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(t);
        const float c = (1.f / (norm + 1e-6f)) * max_norm;   // (no contraction possible)
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;
    }
}

// avg += w * (p - avg): the difference, the product and the sum each round to f32 on their own (no contraction), so the
// update is a numpy float32 statement bit for bit and p == avg is a fixed point
__device__ __forceinline__ float average(float av, float pv, float w)
{
#pragma clang fp contract(off)
    const float d = pv - av;
    const float t = w * d;
    return av + t;
}

struct AverageOp {
    float *avg;
    const float *p;
    float w;

    __device__ __forceinline__ void four(long long i) const
    {
        float4 av = *reinterpret_cast<const float4 *>(avg + i);
        const float4 pv = *reinterpret_cast<const float4 *>(p + i);
        av.x = average(av.x, pv.x, w);
        av.y = average(av.y, pv.y, w);
        av.z = average(av.z, pv.z, w);
        av.w = average(av.w, pv.w, w);
        *reinterpret_cast<float4 *>(avg + i) = av;
    }

    __device__ __forceinline__ void one(long long i) const { avg[i] = average(avg[i], p[i], w); }
};

__global__ __launch_bounds__(OPT_THREADS) void weight_average_kernel(float *__restrict__ avg, const float *__restrict__ p,
                                                                    long long n, const long long *__restrict__ seg,
                                                                    int n_seg, long long total, float w, int vec4)
{
    __shared__ FirstRow s_first;
    AverageOp op = {avg, p, w};
    for_each_piece<OPT_SLICE>(seg, n_seg, total, n, &s_first, [] {},
                              [&](long long a, long long b, int) { for_each_element(a, b, vec4 != 0, op); });
}

enum { ACC_OPEN = 0, ACC_ADD = 1, ACC_CLOSE = 2, ACC_ADD_CLOSE = 3 };

// one element of cova_grad_accumulate: the sum and the product each round to f32 on their own (no contraction), so every
// mode is a numpy float32 statement bit for bit and a scale of 1 leaves the sum's bits
template <int MODE>
__device__ __forceinline__ float accumulate(float av, float gv, float s)
{
#pragma clang fp contract(off)
    if (MODE == ACC_OPEN) return gv;
    if (MODE == ACC_ADD) return av + gv;
    if (MODE == ACC_CLOSE) return av * s;
    const float t = av + gv;
    return t * s;
}

// open and add write acc and only read g, close and add-close write g and only read acc (open does not read acc at all,
// close does not read g)
template <int MODE>
struct AccumulateOp {
    float *acc, *g;
    float s;
    static constexpr bool reads_acc = MODE != ACC_OPEN, reads_g = MODE != ACC_CLOSE;

    __device__ __forceinline__ float *dst() const { return MODE == ACC_OPEN || MODE == ACC_ADD ? acc : g; }

    __device__ __forceinline__ void four(long long i) const
    {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 av = reads_acc ? *reinterpret_cast<const float4 *>(acc + i) : z;
        const float4 gv = reads_g ? *reinterpret_cast<const float4 *>(g + i) : z;
        float4 o;
        o.x = accumulate<MODE>(av.x, gv.x, s);
        o.y = accumulate<MODE>(av.y, gv.y, s);
        o.z = accumulate<MODE>(av.z, gv.z, s);
        o.w = accumulate<MODE>(av.w, gv.w, s);
        *reinterpret_cast<float4 *>(dst() + i) = o;
    }

    __device__ __forceinline__ void one(long long i) const
    {
        dst()[i] = accumulate<MODE>(reads_acc ? acc[i] : 0.f, reads_g ? g[i] : 0.f, s);
    }
};

// every piece is cut to the clip range [c0, c1) of flat elements before it is touched
template <int MODE>
__global__ __launch_bounds__(OPT_THREADS) void grad_accumulate_kernel(float *__restrict__ acc, float *__restrict__ g,
                                                                     long long n, const long long *__restrict__ seg,
                                                                     int n_seg, long long total, long long c0,
                                                                     long long c1, float s, int vec4)
{
    __shared__ FirstRow s_first;
    AccumulateOp<MODE> op = {acc, g, s};
    for_each_piece<OPT_SLICE>(seg, n_seg, total, n, &s_first, [] {}, [&](long long a, long long b, int) {
        a = a > c0 ? a : c0;
        b = b < c1 ? b : c1;
        if (a < b) for_each_element(a, b, vec4 != 0, op);
    });
}

}  // namespace

COVA_API int cova_optim_step(int algo, float *p, const float *g, float *m, float *v, long long n, const long long *segs,
                             int n_seg, long long total, const double *groups, int n_groups, int step,
                             const float *gscale, void *stream)
{
    COVA_REQUIRE(algo >= ALGO_ADAM && algo <= ALGO_SGD);
    COVA_REQUIRE(p && g && segs && groups && n > 0 && n_seg > 0 && total > 0 && total <= n);
    COVA_REQUIRE(n_groups > 0 && n_groups <= MAX_GROUPS);
    COVA_REQUIRE(algo == ALGO_SGD || (m && v && step >= 1));
    OptGroups G = {};
    for (int k = 0; k < n_groups; ++k) {
        const double *h = groups + 9 * k;
        const double lr = h[0], wd = h[1], beta1 = h[2], beta2 = h[3], eps = h[4], mom = h[5], damp = h[6];
        OptGroup &q = G.g[k];
        q.lr = (float)lr;
        q.wd = (float)wd;
        q.beta1 = (float)beta1;
        q.beta2 = (float)beta2;
        q.eps = (float)eps;
        if (algo != ALGO_SGD) {
            q.bc1 = (float)(1.0 - pow(beta1, (double)step));
            q.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
        }
        q.decay = (float)(1.0 - lr * wd);
        q.momentum = (float)mom;
        q.damp1 = (float)(1.0 - damp);
        q.nesterov = h[7] != 0.0;
        q.has_buf = h[8] != 0.0;
        if (algo == ALGO_SGD && mom != 0.0) COVA_REQUIRE(m);
    }
    const int vec4 = aligned16(p) && aligned16(g) && (!m || aligned16(m)) && (!v || aligned16(v));
    const dim3 grid((unsigned)cdivll(total, OPT_SLICE)), block(OPT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    static constexpr decltype(&optim_step_kernel<ALGO_ADAM>) kernels[] = {
        optim_step_kernel<ALGO_ADAM>, optim_step_kernel<ALGO_ADAMW>, optim_step_kernel<ALGO_SGD>};   // by algorithm code
    COVA_LAUNCH(kernels[algo], grid, block, s, p, g, m, v, n, segs, n_seg, total, G, n_groups, gscale,
                vec4);
    return COVA_OK;
}

// doubles of cova_grad_norm's workspace: one partial per block of the first launch
COVA_API int cova_grad_norm_workspace_doubles(long long total)
{
    return total > 0 ? (int)cdivll(total, NORM_SLICE) : 1;
}

COVA_API int cova_grad_norm(const float *g, long long n, const long long *segs, int n_seg, long long total,
                            double max_norm, double *workspace, float *out, void *stream)
{
    COVA_REQUIRE(g && workspace && out && n > 0 && total >= 0 && total <= n && n_seg >= 0);
    COVA_REQUIRE(total == 0 || (segs && n_seg > 0));
    const int n_part = cova_grad_norm_workspace_doubles(total);
    hipStream_t s = (hipStream_t)stream;
    COVA_LAUNCH(grad_sumsq_kernel, dim3(n_part), dim3(OPT_THREADS), s, g, n, segs, total ? n_seg : 0, total,
                (int)aligned16(g), workspace);                    // (no element: no row is read, segs may be null)
    COVA_LAUNCH(grad_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), s, workspace, n_part, (float)max_norm,
                out);
    return COVA_OK;
}

COVA_API int cova_weight_average(float *avg, const float *p, long long n, const long long *segs, int n_seg,
                                 long long total, double one_minus_decay, void *stream)
{
    COVA_REQUIRE(n_seg >= 0 && total >= 0);
    if (n_seg == 0 || total == 0) return COVA_OK;
    COVA_REQUIRE(avg && p && segs && n > 0 && total <= n);
    const float w = (float)one_minus_decay;                  // converted once: the kernel multiplies by this f32
    const dim3 grid((unsigned)cdivll(total, OPT_SLICE)), block(OPT_THREADS);
    COVA_LAUNCH(weight_average_kernel, grid, block, (hipStream_t)stream, avg, p, n, segs, n_seg, total, w,
                (int)(aligned16(avg) && aligned16(p)));
    return COVA_OK;
}

COVA_API int cova_grad_accumulate(int mode, float *acc, float *g, long long n, const long long *segs, int n_seg,
                                  long long total, long long clip_lo, long long clip_hi, double scale, void *stream)
{
    COVA_REQUIRE(mode >= ACC_OPEN && mode <= ACC_ADD_CLOSE);
    COVA_REQUIRE(n_seg >= 0 && total >= 0);
    if (n_seg == 0 || total == 0) return COVA_OK;
    COVA_REQUIRE(acc && g && segs && n > 0 && total <= n);
    const long long c0 = clip_lo > 0 ? clip_lo : 0, c1 = clip_hi < n ? clip_hi : n;
    if (c0 >= c1) return COVA_OK;                            // an empty clip touches nothing: no launch
    const float s = (float)scale;                            // converted once: the kernel multiplies by this f32
    const int vec4 = aligned16(acc) && aligned16(g);
    const dim3 grid((unsigned)cdivll(total, OPT_SLICE)), block(OPT_THREADS);
    static constexpr decltype(&grad_accumulate_kernel<ACC_OPEN>) kernels[] = {                       // by mode
        grad_accumulate_kernel<ACC_OPEN>, grad_accumulate_kernel<ACC_ADD>, grad_accumulate_kernel<ACC_CLOSE>,
        grad_accumulate_kernel<ACC_ADD_CLOSE>};
    COVA_LAUNCH(kernels[mode], grid, block, (hipStream_t)stream, acc, g, n, segs, n_seg, total, c0, c1, s, vec4);
    return COVA_OK;
}
