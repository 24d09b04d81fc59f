// Cached RoI visual features (features.FeatureCache): with a frozen, eval-mode conv stack the RoI-pooled row of a box is a
// constant of its page and coordinates, kept in a split-resident table [R, C].  A head-only step or evaluation batch takes
// its rows from the table by the sampler's SOURCE row ids and lands them in comb[:, :n_vis] (leading dimension T), where
// RoIPool would have written them.
// HBM-bound copy: one pass, 16 bytes per lane when the shapes allow, no atomics, no workspace, bit-exact.
#include "common.h"

namespace {

// VEC floats per thread (4: float4 load and store, 1: scalar).  Flat over N * (C / VEC) elements; IDX is the type of the flat
// index (32-bit when N * C / VEC fits: no 64-bit division in the usual case).  Offsets into the table and the output are
// formed in 64 bits -- a resnet50 table passes 4 GiB at 466 000 boxes.  A row id outside [0, R) yields a row of zeros.
template <int VEC, typename IDX>
__global__ __launch_bounds__(256) void feat_rows_gather_kernel(const float *__restrict__ table, long long R, int C,
                                                               const int *__restrict__ row_ids, IDX total, IDX per_row,
                                                               float *__restrict__ out, int ld_out)
{
    for (IDX i = (IDX)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (IDX)gridDim.x * blockDim.x) {
        const IDX g = i / per_row;
        const int c = (int)(i - g * per_row) * VEC;
        const int r = row_ids[g];
        const bool ok = r >= 0 && (long long)r < R;
        float *d = out + (long long)g * ld_out + c;
        if (VEC == 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = *reinterpret_cast<const float4 *>(table + (long long)r * C + c);
            *reinterpret_cast<float4 *>(d) = v;
        } else {
            *d = ok ? table[(long long)r * C + c] : 0.f;
        }
    }
}

template <int VEC>
int launch_gather(const float *table, long long R, int C, const int *row_ids, int N, float *out, int ld_out,
                   hipStream_t st)
{
    const long long per_row = C / VEC, total = per_row * N;
    long long grid = (total + 255) / 256;
    if (grid > 2048) grid = 2048;                       // 256 CUs x 8 blocks; the rest by grid stride
    if (total < (1ll << 31))
        COVA_LAUNCH((feat_rows_gather_kernel<VEC, unsigned int>), dim3((unsigned)grid), dim3(256), st, table, R,
                    C, row_ids, (unsigned int)total, (unsigned int)per_row, out, ld_out);
    else
        COVA_LAUNCH((feat_rows_gather_kernel<VEC, unsigned long long>), dim3((unsigned)grid), dim3(256), st,
                    table, R, C, row_ids, (unsigned long long)total, (unsigned long long)per_row, out, ld_out);
    return COVA_OK;
}

}  // namespace

// out[g*ld_out + c] = table[row_ids[g]*C + c], c < C; columns C..ld_out of out are not touched
COVA_API int cova_feat_rows_gather(const float *table, long long R, int C, const int *row_ids, int N, float *out,
                                   int ld_out, void *stream)
{
    COVA_REQUIRE(R >= 0 && C > 0 && N >= 0 && ld_out >= C);
    if (N == 0) return COVA_OK;
    COVA_REQUIRE(table && row_ids && out);
    hipStream_t st = (hipStream_t)stream;
    // the table is dense and C % 4 == 0, so its rows are 16-byte aligned whenever its base is
    if (C % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 15) == 0)
        return launch_gather<4>(table, R, C, row_ids, N, out, ld_out, st);
    return launch_gather<1>(table, R, C, row_ids, N, out, ld_out, st);
}
