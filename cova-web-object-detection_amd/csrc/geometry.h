// What the kernels that read box geometry (graph.hip: cova_context_knn, cova_edge_geometry; page_attn.hip: the GEO
// instantiations) promise each other bit for bit: how a box is read from a [N, 5] row and the eight relative-geometry
// features of an ordered pair of boxes.  One definition each; edge_features carries its own fp-contract pragma, so the
// including file's setting does not reach it.
#pragma once
#include "common.h"

// x1, y1, x2, y2 of box g of a [N, 5] table (column 0 is the page)
__device__ __forceinline__ float4 knn_box(const float *__restrict__ bboxes, long long g)
{
    const float *r = bboxes + g * 5;
    return make_float4(r[1], r[2], r[3], r[4]);
}

// Relative geometry of one edge (include/cova_hip.h, cova_edge_geometry): box a = the node i, box b = its neighbour j, both
// x1,y1,x2,y2; dj = j - i.  Every operation is rounded on its own (no contraction: tests/edge_oracle.py states the same
// expressions in numpy float32, parenthesis for parenthesis) and `/` is the correctly rounded division.
__device__ __forceinline__ void edge_features(const float4 a, const float4 b, float W, float H, int dj, float *f)
{
#pragma clang fp contract(off)
    const float wi = a.z - a.x, hi = a.w - a.y, wj = b.z - b.x, hj = b.w - b.y;
    f[0] = ((b.x + b.z) - (a.x + a.z)) / (2.f * W);
    f[1] = ((b.y + b.w) - (a.y + a.w)) / (2.f * H);
    f[2] = (wj - wi) / ((wj + wi) + 1.f);
    f[3] = (hj - hi) / ((hj + hi) + 1.f);
    f[4] = fmaxf(0.f, fmaxf(a.x, b.x) - fminf(a.z, b.z)) / W;      // the gap of knn_key
    f[5] = fmaxf(0.f, fmaxf(a.y, b.y) - fminf(a.w, b.w)) / H;
    const float iw = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
    const float ih = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
    const float inter = iw * ih;
    const float ai = wi * hi, aj = wj * hj;
    const float uni = (ai + aj) - inter;
    f[6] = uni > 0.f ? inter / uni : 0.f;
    f[7] = (float)max(-64, min(64, dj)) / 64.f;
}
