/*
 * cova_hip.h -- C ABI of libcova_hip.so: the MI355X (gfx950) implementation of the CoVA
 * forward/backward hot path.
 *
 * The reference (kevalmorabia97/CoVA-Web-Object-Detection) is pure Python: its hot path is
 * `models.CoVA.forward` + autograd backward (models.py:94-122, train.py:47-60) and every kernel
 * it runs comes from torch / torchvision.  It has no FFI of its own, so this boundary is what a
 * native replacement of those torch/torchvision operator calls has to export (SURVEY.md
 * section 8b): one entry point per fused stage of the path, each citing the reference call it
 * replaces.  The reference-side binding is a ctypes stub; the host mirror of
 * the reference's nn.Module surface lives in cova-web-object-detection_amd/models.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated; the library never allocates:
 *     outputs and workspaces are caller-provided, sizes via the *_num_* / *_workspace_* queries;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all work is
 *     asynchronous on it, nothing synchronises, so calls are hipGraph-capturable;
 *   - return value: 0 on success, a hipError_t value, or COVA_ERR_BAD_ARG (10001);
 *   - all floating point data is IEEE fp32 (the reference computes in fp32), indices int64
 *     as in the reference, RoIPool argmax int32;
 *   - activations of the conv stack are NHWC ([B,H,W,64]; channel = fastest); the image is the
 *     reference's NCHW [B,3,H,W]; dense matrices are row-major with a leading dimension `ld*`
 *     counted in floats.
 */
#ifndef COVA_HIP_H
#define COVA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVA_ERR_BAD_ARG 10001

/* largest K (neighbour slots per node) the cova_gat_* entry points take: sixteen 64-lane passes of the wave-per-node kernels
 * (-cs <= 512: far beyond the boxes of a page -- slots past a page's size are pads; models.py:171-177 itself takes any
 * n_context) */
#define COVA_GAT_MAX_K 1024

/* BatchNorm finalize as the TAIL of the launch that produced the statistics partials (cova_conv1_fwd_tail,
 * cova_conv3x3_wino4_full_tail): the last block to finish folds the partial rows and writes what
 * cova_bn_finalize_fwd (mode 1) or cova_bn_finalize_bwd_abc (mode 2) would write in a launch of its own -- same
 * fp64 arithmetic.  A HOST struct of device pointers, read at launch time.  `counter`: one device int, zero before the
 * first launch; the kernel leaves it zero.  64 channels. */
typedef struct cova_bn_tail {
    int mode;                                   /* 0 none | 1 forward statistics | 2 backward sums */
    int *counter;
    double count;                               /* elements per channel */
    const float *gamma, *beta;                  /* mode 1 */
    float *running_mean, *running_var;          /* mode 1, nullable: momentum update */
    long long *num_batches_tracked;             /* mode 1, nullable: += 1 */
    float momentum, eps;
    float *scale, *shift, *mean, *invstd;       /* mode 1: outputs | mode 2: inputs (mean, invstd, scale) */
    float *dgamma, *dbeta, *abc;                /* mode 2 outputs: dgamma / dbeta (nullable), abc [3][64] */
} cova_bn_tail;

/* ------------------------------------------------------------------ conv stack (models.py:49-51)
 * replaces: torchvision resnet18 children()[:-5] = nn.Conv2d(3,64,7,2,3), nn.BatchNorm2d(64),
 * nn.ReLU, nn.MaxPool2d(3,2,1), 2 x BasicBlock(64) as called at models.py:125 `self.convnet(images)`
 */
int cova_conv_out_size(int in_size, int kernel, int stride, int pad);
/* Test / A-B hooks, not part of the path's contract (six keys; everything else is refused):
 *   2  = cap on the persistent grids (tests force many tiles per block); 0 = none,
 *   7  = conv1 forward and weight gradient on the f32-MFMA kernels (1) instead of the bf16-split ones (0, default): bench.py's `ab` leg,
 *   9  = F(4x4,3x3) forward / data-gradient launches on the f32-MFMA main loop (1) instead of the bf16-split one (0, default): `ab` leg,
 *   14 = cova_bn1d_fwd / _bwd in the float4 form (1, default: taken when the operands are 16-byte aligned) or the 128-slice form (0),
 *   16 = cova_gat_fwd / _bwd with every 64-channel chunk of a neighbour row in flight (1, default; K <= 64, D <= 512) or chunk by chunk (0).
 *   22 = cova_sgemm with the operand tiles brought in by global -> LDS copies (1, default: taken when both operands allow 16-byte
 *        pieces) or staged through registers (0: the kernel every other shape takes).
 * 14, 16 and 22 select between two kernels that both run by default (by alignment / by shape): the tests use them to compare the forms.
 * The option state is a PER-PROCESS CONSTANT: it may be set until the first size query or launch that depends on ANY of the six
 * options (every persistent-grid launch and *_num_partials / *_workspace_floats query reads the grid cap; cova_sgemm, cova_bn1d_*
 * and cova_gat_* read theirs) and is fixed from then on, all six keys together -- launches captured into a hipGraph, workspace
 * sizes already queried and a trainer's buffers all depend on it.  A later
 * cova_set_option that would CHANGE a value returns COVA_ERR_BAD_ARG (10001).  A process that sets COVA_ALLOW_OPTION_CHANGES=1
 * in its environment before the library is loaded keeps them mutable (the test suite and bench.py's `ab` legs, which re-query
 * every workspace size per step, do); options 7 and 9 change the result of the matching *_num_partials queries. */
int cova_set_option(int key, int value);

/* weight layout transforms (OIHW -> kernel layouts); run once per optimizer step */
int cova_conv1_prep_weights(const float *w_oihw /*[64,3,7,7]*/, float *w_k /*[154,64]*/, void *stream);

/* nn.Conv2d(3,64,7,stride 2,pad 3,bias=False): img NCHW -> out NHWC [B,H1,W1,64].
 * stat_part (nullable) [cova_conv1_num_partials][2][64]: per-block channel sum / sum of squares of
 * the output (feeds cova_bn_finalize_fwd: train-mode BatchNorm2d statistics).
 * Arithmetic (forward and cova_conv1_wgrad*): f32 in, f32 out, f32 accumulation; the products run on the bf16 matrix
 * pipe with every f32 operand taken as three bf16 pieces (x = x0 + x1 + x2 up to 2^-26 |x|) and the six products of
 * order <= 2 -- the error against a float64 convolution is that of the f32-MFMA kernels (cova_set_option 7 selects
 * those; tests/test_kernels_gpu.py::test_conv1_bf16_split_error_class), gfx950 having no faster f32 matrix path. */
int cova_conv1_num_tiles(int B, int H, int W);
/* rows of the statistics partials written by cova_conv1_fwd (per tile, or per persistent block) */
int cova_conv1_num_partials(int B, int H, int W);
int cova_conv1_fwd(const float *img, const float *w_k, float *out, float *stat_part, int B, int H,
                   int W, void *stream);
/* ... reading the [64,3,7,7] OIHW weight directly (no cova_conv1_prep_weights launch), and with the BatchNorm finalize
 * of its statistics as the launch's tail (tail: host pointer, mode 1; nullable) */
int cova_conv1_fwd_tail(const float *img, const float *w_oihw, float *out, float *stat_part, int B, int H, int W,
                        const cova_bn_tail *tail, void *stream);
/* gradient of conv1's weight (the image needs no gradient): dw OIHW [64,3,7,7] */
int cova_conv1_wgrad_workspace_floats(int B, int H, int W);
int cova_conv1_wgrad(const float *img, const float *dy /*NHWC*/, float *dw, float *ws, int B, int H,
                     int W, void *stream);
/* gradient w.r.t. the image -- what autograd gives the reference when `images.requires_grad` (models.py:94-122 through
 * nn.Conv2d(3,64,7,2,3)); not on the training hot path (train.py never asks for it): plain kernels.
 * cova_pool_bwd_dy1 writes out dy1 = abc[0]*route(dp, idx) + abc[1]*y1 + abc[2] (NHWC [B,H1,W1,64]), the operand
 * cova_conv1_wgrad_poolbwd forms on load; cova_conv1_dgrad: dimg NCHW [B,3,H,W] from dy1 and the OIHW weight */
int cova_pool_bwd_dy1(const float *dp, const uint8_t *idx, const float *y1, const float *abc, float *dy1, int B, int H1,
                      int W1, void *stream);
int cova_conv1_dgrad(const float *dy1, const float *w_oihw, float *dimg, int B, int H, int W, void *stream);
/* same with the BatchNorm+ReLU+MaxPool backward apply folded into the gradient operand:
 * dy1 = abc[0]*route(dp, idx) + abc[1]*y1 + abc[2]; dp [B,H2,W2,64] already ReLU-masked */
int cova_conv1_wgrad_poolbwd(const float *img, const float *y1, const float *dp, const uint8_t *idx,
                             const float *abc, float *dw, float *ws, int B, int H, int W,
                             void *stream);

/* nn.Conv2d(64,64,3,1,1,bias=False) on NHWC [B,H,W,64] (torchvision BasicBlock / Bottleneck conv2; models.py:49-51) runs as
 * Winograd F(4x4,3x3) convolutions in f32-class arithmetic (below).  The F(2x2,3x3) kernels of rounds 1-3 (forward, data
 * gradient, weight gradient) left the product library in round 6: tools/csrc/conv_wino_f2x2.hip + tools/include/cova_wino_f2x2.h,
 * built as a test-support library (the F(4x4) kernel tests cross-check against them); the direct implicit-GEMM kernels of
 * round 1 live in tools/csrc as well. */
/* Weight gradient in Winograd F(4x4,3x3) form (csrc/conv_wgrad4.hip; 1.78x fewer MFMAs than the F(2x2,3x3) form,
 * fp32 error 3.7e-6 of the gradient's scale): replaces autograd's conv2d weight gradient of the four layer1 3x3
 * convolutions (torchvision BasicBlock conv1 / conv2, models.py:49-51; loss.backward() at train.py:59).  Two steps:
 * activation = relu?(A*act + C) on load (act_abc nullable), gradient = A*dz + B*dz2 + C on load (dz_abc, dz2 nullable;
 * the [3][64] = A | B | C coefficient layout of cova_conv3x3_wino4_full's prologue), per-block partials into ws
 * (cova_conv3x3_wgrad4_workspace_floats; each block applies G^T . G to its own sums in fp64 and writes [9][64][64]),
 * then the fp64 fold of up to four convolutions in one launch. */
int cova_conv3x3_wgrad4_num_partials(int B, int H, int W);
int cova_conv3x3_wgrad4_workspace_floats(int B, int H, int W);
int cova_conv3x3_wgrad4_partial(const float *act, const float *act_abc /*nullable*/, int act_relu, const float *dz,
                                const float *dz2 /*nullable*/, const float *dz_abc /*nullable*/,
                                float *dz_out /*nullable: also writes A*dz + B*dz2 + C, NHWC [B,H,W,64]*/, float *ws, int B,
                                int H, int W, void *stream);
/* finish: every (ws_i, dw_i) pair is nullable as a pair -- a (NULL, NULL) slot is skipped (a frozen weight whose partial
 * launch was not issued); the given pairs are folded exactly as when all four are present; all four NULL issues no launch. */
int cova_conv3x3_wgrad4_finish(const float *ws0, float *dw0, const float *ws1, float *dw1, const float *ws2,
                               float *dw2, const float *ws3, float *dw3, int B, int H, int W, void *stream);
int cova_conv3x3_wgrad4(const float *act, const float *dz, float *dw /*OIHW*/, float *ws, int B, int H, int W,
                        void *stream);

/* F(4x4,3x3) form of the same convolution (csrc/conv_wino4.hip; 1.78x fewer MFMAs than F(2x2,3x3), fp32 error 2.9e-6 of
 * the output scale): u_fwd / u_dgrad cova_conv3x3_wino4_u_floats() floats each per convolution (the per-wave register
 * images written by the prep kernel: the f32 image, its three-bf16-piece image, and the piece image of -U -- the tiles of odd
 * tile row ty (rows of 8-pixel-high block tiles, counted per page) are multiplied with the negated weights and un-negated in the
 * epilogue, so that the bf16 MFMA's sign-asymmetric accumulation (7e-8 of the mean magnitude toward -inf on every output,
 * tools/w4s_bias.py) cancels in sums over a map; a map of one tile row (tiles_y == 1) has no negated tiles at all);
 * stat_part (nullable) [cova_conv3x3_wino4_num_partials][2][64] = (sum y, sum y^2).
 * Arithmetic: f32 in, f32 out, f32 transforms and accumulation; the transform-domain products run on the bf16 matrix pipe
 * with both f32 operands taken as three round-to-nearest bf16 pieces and the six products of order <= 2 (as conv1, see
 * above): f32-class error (tests/test_kernels_gpu.py::test_conv3x3_winograd_f4x4_split_error_class; piece by piece:
 * tests/test_wino4_probe_gpu.py).  The launches with a
 * SECOND input tensor (in2) and cova_set_option(9, 1) run the products on v_mfma_f32_16x16x4_f32. */
int cova_conv3x3_wino4_u_floats(void);
int cova_conv3x3_wino4_num_tiles(int B, int H, int W);
int cova_conv3x3_wino4_num_partials(int B, int H, int W);
int cova_conv3x3_wino4_prep(const float *w_oihw, float *u_fwd, float *u_dgrad, void *stream);
/* ... of up to four convolutions in ONE call (w1..w3 nullable): u_fwd / u_dgrad hold n x cova_conv3x3_wino4_u_floats() floats */
int cova_conv3x3_wino4_prep_multi(const float *w0, const float *w1, const float *w2, const float *w3, float *u_fwd,
                                  float *u_dgrad, void *stream);
int cova_conv3x3_wino4(const float *in, const float *u, float *out, float *stat_part /*nullable*/, int B, int H,
                       int W, void *stream);
/* ... on relu?(A[c]*in + C[c]) formed on load (pro_abc [3][64] = A | unused | C), zero padding stays zero */
int cova_conv3x3_wino4_pro(const float *in, const float *pro_abc, int pro_relu, const float *u, float *out,
                           float *stat_part /*nullable*/, int B, int H, int W, void *stream);
/* ... full form.  The prologue / epilogue contract (cova_conv1x1 and the wgrad4 operands follow it):
 *   on load   x = f(A[c]*in + B[c]*in2 + C[c]), pro_abc [3][C] = A | B | C per input channel, f = ReLU if pro_relu; in2 NULL drops
 *             the B term, pro_abc NULL takes in as it is; zero padding stays zero.
 *   epilogue  g = (acc + addend) x ReLU mask; addend (nullable) has the output's shape; the mask is act > 0, or
 *             fma(mask_scale[c], z, mask_shift[c]) > 0 when act is NULL, and absent when neither is given.
 *   stat_part z given: the BatchNorm-backward sums (sum g, sum g*xhat(z)), xhat(z) = (z - mean[c]) * invstd[c];
 *             z NULL: the plain statistics (sum y, sum y^2) of the output. */
int cova_conv3x3_wino4_full(const float *in, const float *in2 /*nullable*/, const float *pro_abc /*nullable*/,
                            int pro_relu, const float *u, const float *addend /*nullable*/,
                            const float *act /*nullable*/, const float *mask_scale /*nullable*/,
                            const float *mask_shift /*nullable*/, const float *z /*nullable*/,
                            const float *mean /*nullable*/, const float *invstd /*nullable*/, float *out,
                            float *stat_part /*nullable*/, int B, int H, int W, void *stream);
/* ... with the BatchNorm finalize of stat_part as the launch's tail (tail: host pointer; mode 1 for plain statistics,
 * mode 2 for the BatchNorm-backward sums of the z epilogue).  act_bits (nullable, instead of act): the mask source as
 * one bit per element, [B*H*W][2] words as cova_bn_act_fwd_bits writes them */
int cova_conv3x3_wino4_full_tail(const float *in, const float *in2 /*nullable*/, const float *pro_abc /*nullable*/,
                                 int pro_relu, const float *u, const float *addend /*nullable*/,
                                 const float *act /*nullable*/, const uint32_t *act_bits /*nullable*/,
                                 const float *mask_scale /*nullable*/,
                                 const float *mask_shift /*nullable*/, const float *z /*nullable*/,
                                 const float *mean /*nullable*/, const float *invstd /*nullable*/, float *out,
                                 float *stat_part, int B, int H, int W, const cova_bn_tail *tail, void *stream);
/* ... inference form (replaces conv -> eval-mode BatchNorm -> (+ identity) -> ReLU of torchvision's BasicBlock.forward in
 * train.evaluate_model's no-grad forward, train.py:99-129; models.py:49-51):
 * out = f(scale[c]*conv(g(in)) + shift[c] + addend), f = ReLU if relu; g = relu?(A[c]*in + C[c]) on load when pro_abc
 * ([3][64] = A | unused | C) is given.  Same expression and operation order as cova_bn_act_fwd; no statistics */
int cova_conv3x3_wino4_bnact(const float *in, const float *pro_abc /*nullable*/, int pro_relu, const float *u,
                             const float *addend /*nullable*/, const float *scale, const float *shift, int relu,
                             float *out, int B, int H, int W, void *stream);

/* ---- ResNet-50-stem extension (BASELINE.json configs[2], [4]; the reference wires resnet18 only,
 * models.py:49): 1x1 convolutions of torchvision's Bottleneck (conv1, conv3, downsample[0]) on NHWC rows.
 * out[r,co] = sum_ci f(A[ci]*in[r,ci] + B[ci]*in2[r,ci] + C[ci]) * w[co,ci], (Cin,Cout) in {(64,64),(64,256),
 * (256,64)}; w [Cout,Cin] row-major (= OIHW), or with w_trans [Cin,Cout] (data gradient of the conv whose
 * weight it is).  Prologue / epilogue arguments as cova_conv3x3_wino4_full; stat_part
 * [cova_conv1x1_num_partials][2][Cout] = (sum y, sum y^2) when z == NULL, else (sum dy, sum dy*xhat);
 * z2/mean2/invstd2 + stat_part2: a second BatchNorm (the downsample branch) fed by the same dy.
 * z == NULL with act != NULL (Cout = 256): (acc + addend) * [act > 0] without sums (taken by cova_conv1x1_vprod);
 * the same with act_bits [R][8] words instead of act: bit (c & 31) of word c >> 5 = the decision for channel c, as
 * written by cova_conv1x1_materialize (1/32 of the mask source's bytes). */
int cova_conv1x1_num_partials(long long R, int Cin, int Cout);
int cova_conv1x1(const float *in, const float *in2 /*nullable*/, const float *pro_abc /*nullable [3,Cin]*/,
                 int pro_relu, const float *w, int w_trans, const float *addend /*nullable*/,
                 const float *act /*nullable*/, const uint32_t *act_bits /*nullable*/,
                 const float *mask_scale /*nullable*/,
                 const float *mask_shift /*nullable*/, const float *z /*nullable*/,
                 const float *mean /*nullable*/, const float *invstd /*nullable*/,
                 const float *z2 /*nullable*/, const float *mean2 /*nullable*/,
                 const float *invstd2 /*nullable*/, float *out, float *stat_part /*nullable*/,
                 float *stat_part2 /*nullable*/, long long R, int Cin, int Cout, void *stream);
/* cova_conv1x1 (256 -> 64, forward; stat_part as there, nullable) on relu(A*in + B*in2 + C), which is also
 * written to side [R,256]: the first consumer of a Bottleneck output materialises it -- and (side_bits nullable,
 * [R][8] words) its ReLU decisions as one bit per element */
int cova_conv1x1_materialize(const float *in, const float *in2, const float *pro_abc /*[3,256]*/, const float *w,
                             float *side, uint32_t *side_bits, float *out, float *stat_part /*nullable*/, long long R,
                             void *stream);
/* dw [Co,Ci] = sum_r (dz_abc[0]*dz + dz_abc[1]*dz2 + dz_abc[2])[r,co] * relu?(act_abc[0]*act + act_abc[2])[r,ci];
 * (Co,Ci) in {(64,64),(256,64),(64,256)}; ws >= cova_conv1x1_wgrad_workspace_floats */
int cova_conv1x1_wgrad_workspace_floats(long long R, int Co, int Ci);
int cova_conv1x1_wgrad(const float *dz, const float *dz2 /*nullable*/, const float *dz_abc /*nullable [3,Co]*/,
                       const float *act, const float *act_abc /*nullable [3,Ci]*/, int act_relu, float *dw,
                       float *ws, long long R, int Co, int Ci, void *stream);

/* Linear form of the backward of (1x1 conv 64->256, train-mode BatchNorm) -- Bottleneck conv3+bn3 and
 * downsample[0]+[1]: with z = a W^T, the BatchNorm sums, dW and dz*W are functions of P = v^T a, G = a^T a,
 * S = sum a, SU = sum v, so the 256-channel z is never read in the backward (csrc/conv1x1_lin.hip).
 *   cova_conv1x1_vprod      v [R,256], act [R,64] (a = relu?(act_abc[0]*act + act_abc[2]), act_abc nullable)
 *                           -> lin [cova_conv1x1_lin_floats] = P | G | S | SU
 *   cova_conv1x1_lin_bnsums lin, w [256,64], mean, invstd -> part [2][256] = (sum v, sum v*xhat(z)): one row of
 *                           partials for cova_bn_finalize_bwd_abc
 *   cova_conv1x1_lin_finish lin, abc [3][256] (dz = A*v + B*z + C), w -> dw [256,64], m [64,64] = W^T diag(B) W,
 *                           cvec [64] = C^T W, avec [3][256] = A | 0 | 0
 *   cova_conv1x1_lin_dgrad  out [R,64] = ((avec.v) W + a m + cvec (+ addend)) * [fma(mask_scale, z, mask_shift) > 0]
 *                           and (sum, sum*xhat(z)) partials [cova_conv1x1_lin_dgrad_num_partials][2][64] of the
 *                           64-channel BatchNorm in front (z, mean, invstd: that layer's) */
int cova_conv1x1_lin_floats(void);
int cova_conv1x1_vprod_workspace_floats(long long R);
int cova_conv1x1_vprod(const float *v, const float *act, const float *act_abc /*nullable [3,64]*/, int act_relu,
                       float *lin, float *ws, long long R, void *stream);
int cova_conv1x1_lin_bnsums(const float *lin, const float *w, const float *mean, const float *invstd,
                            float *part, void *stream);
int cova_conv1x1_lin_finish(const float *lin, const float *abc, const float *w, float *dw, float *m,
                            float *cvec, float *avec, void *stream);
int cova_conv1x1_lin_dgrad_num_partials(long long R);
int cova_conv1x1_lin_dgrad(const float *v, const float *avec, const float *w, const float *act,
                           const float *act_abc, int act_relu, const float *m, const float *cvec,
                           const float *addend /*nullable [R,64]*/, const float *mask_scale,
                           const float *mask_shift, const float *z, const float *mean, const float *invstd,
                           float *out, float *stat_part, long long R, void *stream);

/* ---- optional layer2 stage (CoVA(backbone_layers=2): torchvision resnet18 children()[:-4], one stage more than
 * models.py:49-51 keeps): channel-generic NHWC convolutions, csrc/conv_nhwc.hip.  k in {1, 3}, stride in {1, 2},
 * pad < k, Ci and Co multiples of 64 (weight gradient: Co a multiple of 128); input [B,H,W,Ci], output
 * [B,Ho,Wo,Co] with Ho = (H + 2 pad - k) / stride + 1.  f32 MFMA (exact f32 products), no float atomics. */
/* OIHW [Co,Ci,k,k] -> forward operand [k*k*Ci][Co] and data-gradient operand [k*k*Co][Ci] (either nullable) */
int cova_conv_nhwc_prep(const float *w_oihw, float *w_fwd, float *w_dgrad, int Co, int Ci, int k, void *stream);
int cova_conv_nhwc_fwd(const float *in, const float *w_fwd, float *out, int B, int H, int W, int Ci, int Co, int k,
                       int stride, int pad, void *stream);
/* dx [B,H,W,Ci] = data gradient of the (k, stride, pad) convolution for dy [B,Ho,Wo,Co] (+ that of a 1x1 pad-0
 * convolution of the same stride for dy2, nullable with w2_dgrad) (+ addend [B,H,W,Ci], nullable).  Every element of dx
 * is written, positions no output reads included (zeros). */
int cova_conv_nhwc_dgrad(const float *dy, const float *w_dgrad, const float *dy2, const float *w2_dgrad,
                         const float *addend, float *dx, int B, int H, int W, int Ci, int Co, int k, int stride, int pad,
                         void *stream);
/* dw OIHW = sum over pixels of in (x) dy: per-block partial sums in ws, folded in a fixed order by a second launch */
int cova_conv_nhwc_wgrad_num_partials(int B, int Ho, int Wo, int Ci, int Co, int k);
int cova_conv_nhwc_wgrad_workspace_floats(int B, int Ho, int Wo, int Ci, int Co, int k);
int cova_conv_nhwc_wgrad(const float *in, const float *dy, float *dw, float *ws, int B, int H, int W, int Ci, int Co,
                         int k, int stride, int pad, void *stream);

/* ------------------------------------------------------------------ BatchNorm / ReLU / MaxPool
 * replaces: nn.BatchNorm2d / nn.BatchNorm1d (train: batch statistics + running-stat update with
 * momentum, unbiased running_var; eval: running statistics), nn.ReLU, the BasicBlock residual
 * add and nn.MaxPool2d(3,2,1) -- models.py:49-51, :68, :73, :86 and their autograd. */
/* deterministic pre-reduction of per-tile / per-chunk partial rows (fp64 inside a group) */
int cova_partials_fold(const float *partial, int nparts, int width, int group, float *out,
                       void *stream);
int cova_colreduce_rows_per_chunk(long long R, int C);
int cova_colreduce_num_chunks(long long R, int C);
int cova_colstats(const float *x, int ldx, long long R, int C, float *partial /*[chunks,2,C]*/,
                  void *stream);
int cova_bn_finalize_fwd(const float *partial, int nparts, int C, double count, const float *gamma,
                         const float *beta, float *running_mean /*nullable*/, float *running_var,
                         long long *num_batches_tracked /*nullable: += 1, like nn.BatchNorm in train mode*/,
                         float momentum, float eps, float *scale, float *shift, float *mean,
                         float *invstd, void *stream);
int cova_bn_eval_params(const float *gamma, const float *beta, const float *running_mean,
                        const float *running_var, float eps, int C, float *scale, float *shift,
                        float *mean /*nullable*/, float *invstd /*nullable*/, void *stream);
int cova_bn_act_fwd(const float *z, int ldz, const float *scale, const float *shift,
                    const float *res /*nullable*/, int ldres, float *out, int ldo, long long R, int C,
                    int relu, void *stream);
/* cova_bn_act_fwd with ReLU for a contiguous [R,64] map (res nullable), also writing the ReLU decisions as one bit per
 * element: bits [R][2] words, bit k of word w = (out[r][32 w + k] > 0) */
int cova_bn_act_fwd_bits(const float *z, const float *scale, const float *shift, const float *res, float *out,
                         uint32_t *bits, long long R, void *stream);
/* out = act(bn(z) + bn2(z2)): join of a Bottleneck whose identity branch is conv + BatchNorm */
int cova_bn_act2_fwd(const float *z, const float *scale, const float *shift, const float *z2,
                     const float *scale2, const float *shift2, float *out, long long R, int C, int relu,
                     void *stream);
int cova_bn_bwd_reduce(const float *dout, int ldd, const float *act /*nullable: relu mask source*/,
                       int lda, const float *z, int ldz, const float *mean, const float *invstd,
                       long long R, int C, float *partial /*[chunks,2,C]*/, void *stream);
int cova_bn_finalize_bwd(const float *partial, int nparts, int C, double count,
                         float *dgamma /*nullable*/, float *dbeta /*nullable*/, float *coef /*[2,C]*/,
                         void *stream);
/* same + the apply step in affine form: dz = abc[0]*dy + abc[1]*z + abc[2]; abc [3,C] */
int cova_bn_finalize_bwd_abc(const float *partial, int nparts, int C, double count,
                             float *dgamma /*nullable*/, float *dbeta /*nullable*/, const float *mean,
                             const float *invstd, const float *scale, float *abc, void *stream);
int cova_bn_bwd_apply(const float *dout, int ldd, const float *act, int lda, const float *z, int ldz,
                      const float *mean, const float *invstd, const float *scale, const float *coef,
                      float *dz, int lddz, float *dres /*nullable*/, int lddres, long long R, int C,
                      void *stream);
/* nn.BatchNorm1d in train mode over box rows x [R,C] (models.py:68 bbox_feat_encoder.1, :73 bn_additional_feat, :86
 * decoder.2) as ONE launch: column statistics, running-statistics update, scale/shift/mean/invstd, out = bn(x) (ReLU if
 * `relu`), and -- dropped != NULL -- nn.Dropout(p) of the result (models.py:88; mask [R,C] generated from `seed` and
 * stored, or taken as given), i.e. cova_colstats + cova_bn_finalize_fwd + cova_bn_act_fwd (+ cova_dropout_fwd). */
int cova_bn1d_fwd(const float *x, int ldx, int R, int C, const float *gamma, const float *beta,
                  float *running_mean /*nullable*/, float *running_var, long long *num_batches_tracked /*nullable*/,
                  float momentum, float eps, int relu, float *out, int ldo, float *dropped /*nullable*/, int ld_dropped,
                  uint8_t *mask, float p, unsigned long long seed, int mask_given, float *scale, float *shift,
                  float *mean, float *invstd, void *stream);
/* its backward in ONE launch: dy = dout (* drop_mask/(1-p) if drop_mask: the Dropout behind the layer) (* (act > 0) if
 * act: the ReLU behind it); dgamma, dbeta (nullable); dz [R,C]; dz_colsum (nullable) [C] = column sums of dz (the bias
 * gradient of the nn.Linear in front, models.py:85) -- i.e. (cova_dropout_bwd +) cova_bn_bwd_reduce +
 * cova_bn_finalize_bwd + cova_bn_bwd_apply (+ cova_colsum).  dz must not alias dout. */
int cova_bn1d_bwd(const float *dout, int ldg, const uint8_t *drop_mask /*nullable*/, float p,
                  const float *act /*nullable*/, int lda, const float *z, int ldz, const float *mean,
                  const float *invstd, const float *scale, int R, int C, float *dgamma, float *dbeta, float *dz,
                  int lddz, float *dz_colsum /*nullable*/, void *stream);
int cova_bn_relu_maxpool_fwd(const float *y /*[B,H1,W1,64]*/, const float *scale, const float *shift,
                             float *out /*[B,H2,W2,64]*/, uint8_t *idx,
                             float *ymax /*nullable [B,H2,W2,64]: raw y at the arg-max*/, int B, int H1,
                             int W1, void *stream);
int cova_bn_relu_maxpool_bwd_num_partials(int B, int H1, int W1);
int cova_bn_relu_maxpool_bwd_reduce(const float *dp, const uint8_t *idx, const float *y,
                                    const float *scale, const float *shift, const float *mean,
                                    const float *invstd, float *partial, int B, int H1, int W1,
                                    void *stream);
int cova_bn_relu_maxpool_bwd_apply(const float *dp, const uint8_t *idx, const float *y,
                                   const float *scale, const float *shift, const float *mean,
                                   const float *invstd, const float *coef, float *dz, int B, int H1,
                                   int W1, void *stream);

/* ------------------------------------------------------------------ RoIPool (models.py:58,125)
 * replaces: torchvision.ops.RoIPool(output_size, spatial_scale)(feat, rois) and its backward.
 * feat NHWC [B,H,W,C]; rois [N,5] = [batch_idx,x1,y1,x2,y2]; row n of the output (C*PH*PW
 * values, index c*PH*PW + ph*PW + pw exactly like `.view(N, n_visual_feat)` at models.py:125-127)
 * is written at out + n*ld_out so it can land directly in the concatenated feature matrix.
 * Memory safety: a box whose page index is outside [0,B) pools nothing (all bins 0, argmax -1). */
int cova_roipool_fwd(const float *feat, const float *rois, int n_rois, int B, int C, int H, int W,
                     int PH, int PW, float spatial_scale, float *out, int ld_out, int32_t *argmax,
                     void *stream);
/* backward: gfeat NHWC [B,H,W,C] (fully written: no zero-fill needed) = gout routed to the arg-max positions.
 * Deterministic -- no float atomics: every feature row has one owner wave that adds the boxes touching it in
 * ascending box order (the reference's scatter collides constantly: DOM parents contain their children). */
int cova_roipool_bwd(const float *gout, int ld_g, const float *rois, const int32_t *argmax,
                     int n_rois, int B, int C, int H, int W, int PH, int PW, float spatial_scale,
                     float *gfeat, void *ws /*cova_roipool_bwd_workspace_words x 4 bytes*/, void *stream);
int cova_roipool_bwd_workspace_words(int n_rois, int B, int C, int PH, int PW);
/* same for a map produced as relu(bn(z) + residual) and pooled by cova_roipool_fwd_bn: the routed gradient
 * is masked by that ReLU (pooled > 0: the pooled value is the map's value at the arg-max) and the producer's
 * BatchNorm-backward partial sums [cova_roipool_bwd_bn_num_partials][2][C] = (sum g', sum g' * xhat(zmax)) are
 * taken per pooled entry -- no map is read.  gfeat = the ReLU-masked gradient map. */
int cova_roipool_bwd_bn_num_partials(int n_rois);
int cova_roipool_bwd_bn(const float *gout, int ld_g, const float *pooled, int ld_p, const float *zmax,
                        const float *rois, const int32_t *argmax, int n_rois, int B, int C, int H, int W,
                        int PH, int PW, float spatial_scale, const float *mean, const float *invstd,
                        float *gfeat, float *partial, void *ws /*cova_roipool_bwd_workspace_words x 4 bytes*/,
                        void *stream);
/* ... with cova_bn_finalize_bwd_abc of those sums as the tail of the entry pass (tail: host pointer, mode 2; C = 64) */
int cova_roipool_bwd_bn_tail(const float *gout, int ld_g, const float *pooled, int ld_p, const float *zmax,
                             const float *rois, const int32_t *argmax, int n_rois, int B, int C, int H, int W,
                             int PH, int PW, float spatial_scale, const float *mean, const float *invstd,
                             float *gfeat, float *partial, void *ws, const cova_bn_tail *tail, void *stream);
/* RoIPool over relu(scale*z + shift + x) formed on the fly (last BasicBlock's bn2+residual+ReLU) */
int cova_roipool_fwd_bn(const float *z, const float *x, const float *scale, const float *shift,
                        const float *rois, int n_rois, int B, int C, int H, int W, int PH, int PW,
                        float spatial_scale, float *out, int ld_out, int32_t *argmax,
                        float *zmax /*nullable [N, C*PH*PW]: z at each arg-max, for cova_roipool_bwd_bn*/,
                        void *stream);

/* RoIAlign -- EXTENSION: north_star names it, the reference calls RoIPool (models.py:58), which stays the parity
 * operator.  torchvision.ops.RoIAlign semantics (bilinear samples, sampling_ratio^2 per bin, or ceil(roi/bin)^2
 * when sampling_ratio <= 0; `aligned` half-pixel shift); same tensor conventions as cova_roipool_fwd / _bwd;
 * backward deterministic (one owner wave per feature row), ws >= (2*B + 16) ints. */
int cova_roialign_fwd(const float *feat, const float *rois, int n_rois, int B, int C, int H, int W, int PH,
                      int PW, float spatial_scale, int sampling_ratio, int aligned, float *out, int ld_out,
                      void *stream);
int cova_roialign_bwd(const float *gout, int ld_g, const float *rois, int n_rois, int B, int C, int H, int W,
                      int PH, int PW, float spatial_scale, int sampling_ratio, int aligned, float *gfeat,
                      void *ws, void *stream);

/* ------------------------------------------------------------------ positional encoder
 * replaces: CoVA._get_bbox_features up to nn.Linear(5, Hd) (models.py:134-144):
 * raw = [x1, y1, x2-x1, y2-y1, (x2-x1)/(y2-y1)], z = raw W^T + b */
int cova_bbox_linear_fwd(const float *bboxes, const float *W /*[Hd,5]*/, const float *bias,
                         float *raw /*[N,5]*/, float *z /*[N,Hd]*/, int N, int Hd, void *stream);
int cova_bbox_linear_bwd(const float *dz, const float *raw, float *dW, float *db, int N, int Hd,
                         void *stream);

/* ------------------------------------------------------------------ dense layers
 * replaces: nn.Linear forward/backward GEMMs (models.py:85,161-162): C (+)= op(A) op(B) (+ bias)
 * Row-major operands: A is [M,K] (transA = 0, lda >= K) or [K,M] (transA = 1, lda >= M), B is [K,N] (transB = 0, ldb >= N) or
 * [N,K] (transB = 1, ldb >= K), C is [M,N] with ldc >= N.  A negative M, N or K, a null A, B or C and a leading dimension
 * shorter than its operand's row are refused (COVA_ERR_BAD_ARG, nothing is launched); M == 0 or N == 0 returns 0 and writes
 * nothing; K == 0 leaves C = bias (or 0), added to the old C under accumulate. */
int cova_sgemm(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B,
               int ldb, float *C, int ldc, const float *bias /*nullable [N]*/, int accumulate,
               void *stream);
/* cova_sgemm (no bias, no accumulate) with cova_dropout_bwd applied to its result in the epilogue:
 * C = keep ? op(A) op(B) / (1 - p) : 0, keep [M,N] uint8 contiguous -- the decoder's first Dropout backward
 * (models.py:84) behind the data gradient of decoder.1 (models.py:85); bit-identical to the two launches.  cova_sgemm's refusals, and a null keep, p < 0 or p >= 1 */
int cova_sgemm_dropout_bwd(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B,
                           int ldb, float *C, int ldc, const uint8_t *keep /*[M,N]*/, float p, void *stream);

/* ------------------------------------------------------------------ graph attention (models.py:171-212)
 * replaces: GraphAttentionLayer.forward after the projections: gather, score, LeakyReLU, mask,
 * softmax, weighted sum.  Wh [N,2D] = h [W_i;W_j]^T.  K <= 256 (the K slots of a node are held by one wavefront in
 * ceil(K/64) passes over its lanes; models.py:171-177 takes any n_context).  Neighbour ids >= N are treated like the
 * -1 pad (the reference's h_i_padded[context_indices] raises an index error for them). */
int cova_gat_fwd(const float *Wh, int ldw, const float *att_w /*[2D]*/, const float *att_b /*[1]*/,
                 const int64_t *ctx /*[N,K]*/, int N, int K, int D, float slope, float *s /*[N]*/,
                 float *t /*[N]*/, float *attn /*[N,K]*/, float *hprime, int ldh, void *stream);
/* transposed neighbour index (CSR over destination nodes) of ctx: csr[0..N] row offsets, then the flat slots
 * i*K+k naming each node, ascending.  Lets the backward gather with a fixed summation order instead of
 * scattering with float atomics (torch's index_select backward): bit-identical reruns for ANY index table. */
int cova_gat_transpose_ints(int N, int K);
int cova_gat_transpose(const int64_t *ctx, int N, int K, int *csr /*[cova_gat_transpose_ints]*/, void *stream);
/* ... into a workspace kept from call to call (one per stream): the last 2N + 16 ints of csr must be zero on entry --
 * zero the buffer once when allocating it -- and are left zero: three launches, no memsets */
int cova_gat_transpose_reuse(const int64_t *ctx, int N, int K, int *csr, void *stream);
/* backward of cova_gat_fwd: gathers through csr (cova_gat_transpose) with du [N,K] as scratch -- fixed summation order, no
 * float atomics, bit-identical reruns.  csr and du are REQUIRED: NULL returns COVA_ERR_BAD_ARG before anything is launched. */
int cova_gat_bwd(const float *g, int ldg, const float *Wh, int ldw, const float *s, const float *t,
                 const float *attn, const int64_t *ctx, const float *att_w, int N, int K, int D,
                 float slope, float *dWh /*[N,2D]*/, int lddw, float *ds /*[N]*/, float *dt /*[N]*/,
                 float *d_att_w /*[2D]*/, float *d_att_b /*[1]*/, const int *csr, float *du /*[N,K]*/, void *stream);
/* ---- edge geometry in the attention score (opt-in: CoVA(edge_geometry=True); the reference has no such term) ----
 * cova_gat_fwd_edge: cova_gat_fwd with the pre-activation of slot k of node i extended by an additive edge term,
 *   u = s[i] + t[j] + sum_e edge_w[e] * phi[i,k,e]   (one fma chain, e ascending, added to s[i] + t[j] last),
 * phi [N,K,8] from cova_edge_geometry (16-byte aligned), edge_w [8] (`edge_layer.weight`, no bias: att_b is there).
 * LeakyReLU, the -9e15 mask, softmax and aggregation are cova_gat_fwd's; pads and ids >= N read no phi.  With edge_w = 0
 * every output has cova_gat_fwd's bits.  The same launches as cova_gat_fwd (scores, then the EDGE instantiation of the
 * wave-per-node kernel): no LDS, no workspace, capturable. */
int cova_gat_fwd_edge(const float *Wh, int ldw, const float *att_w /*[2D]*/, const float *att_b /*[1]*/,
                      const int64_t *ctx /*[N,K]*/, const float *phi /*[N,K,8]*/, const float *edge_w /*[8]*/, int N,
                      int K, int D, float slope, float *s /*[N]*/, float *t /*[N]*/, float *attn /*[N,K]*/,
                      float *hprime, int ldh, void *stream);
/* cova_gat_bwd_edge: cova_gat_bwd for a forward made by cova_gat_fwd_edge: the LeakyReLU slope of a slot follows the
 * forward's u bit for bit.
 * Also d_edge_w[e] = sum_{i,k} du[i,k] * phi[i,k,e] [8]: per-block partials of fixed 4096-slot chunks in `workspace`
 * (cova_gat_edge_workspace_floats(N, K) floats), then summed in index order by one block -- no atomics, bits independent
 * of timing and grid.  There is no gradient with respect to the boxes.  With edge_w = 0, dWh / d_att_w / d_att_b have
 * cova_gat_bwd's bits. */
int cova_gat_edge_workspace_floats(int N, int K);
int cova_gat_bwd_edge(const float *g, int ldg, const float *Wh, int ldw, const float *s, const float *t,
                      const float *attn, const int64_t *ctx, const float *att_w, const float *phi /*[N,K,8]*/,
                      const float *edge_w /*[8]*/, int N, int K, int D, float slope, float *dWh /*[N,2D]*/, int lddw,
                      float *ds /*[N]*/, float *dt /*[N]*/, float *d_att_w /*[2D]*/, float *d_att_b /*[1]*/,
                      float *d_edge_w /*[8]*/, const int *csr, float *du /*[N,K]*/, float *workspace, void *stream);
/* ---- GATv2 dynamic attention (gat_v2.hip; opt-in: CoVA(attention="gatv2"); Brody et al., ICLR 2022) ----
 * The static score above is LeakyReLU(s[i] + t[j]): every node ranks a given set of neighbours alike.  cova_gat2_fwd scores
 *   z[i,k,d] = Wh[i,d] + Wh[j,D+d]  (j = ctx[i,k]; one f32 add),   u[i,k] = att_b + sum_d att_w[d] * lrelu(z[i,k,d]),
 *   lrelu(z) = z > 0 ? z : slope * z  (z == +-0 takes the slope branch),   att_w [D] (not [2D]),
 * and, when phi [N,K,8] (16-byte aligned) and edge_w [8] are given (together or not at all), u += edge_w . phi[i,k,:], added
 * LAST and OUTSIDE the non-linearity -- cova_gat_fwd_edge has its edge term inside the LeakyReLU.  Mask (-9e15 on pads and
 * ids >= N), softmax over k and h'[i] = sum_k attn[i,k] * Wh[j, D:2D] are cova_gat_fwd's; an all-pad row gives 1/K and a zero
 * h'.  edge_w = 0 gives the bits of the call without phi.  One launch: a wave per node, float4 lanes over channels when
 * D % 4 == 0 and Wh / att_w / hprime (and ldw, ldh) are 16-byte aligned, else a scalar form; D <= 2048 (scalar form 1024).
 * cova_gat2_bwd: g = dL/dh'; writes du [N,K] = attn * (dattn - sum attn * dattn) (pads exactly 0), all of dWh [N,2D]
 *   dWh[i,d]   = att_w[d] * sum_k du[i,k] * gate(z[i,k,d])                             gate(z) = z > 0 ? 1 : slope
 *   dWh[j,D+d] = sum_{(i,k): ctx[i,k] = j} attn[i,k] * g[i,d] + du[i,k] * att_w[d] * gate(z[i,k,d])   through csr, ascending
 * (the gates re-formed by the forward's add and compare: identical decisions), and d_att_w[d] = sum du * lrelu(z),
 * d_att_b = sum du, d_edge_w[e] = sum du * phi[..,e] (with phi / edge_w / d_edge_w: all three or none): partial sums of
 * fixed blocks of four nodes in `workspace` (cova_gat2_workspace_floats(N, K, D) floats), folded in index order -- no float
 * atomics, bit-identical reruns.  Three launches.  csr from cova_gat_transpose(_reuse).  Bad arguments (K outside
 * [1, 1024], D outside the range above, ld* too small, a NULL operand, phi without edge_w) return COVA_ERR_BAD_ARG before
 * anything is launched; N == 0 launches nothing. */
int cova_gat2_fwd(const float *Wh, int ldw, const float *att_w /*[D]*/, const float *att_b /*[1]*/,
                  const int64_t *ctx /*[N,K]*/, const float *phi /*[N,K,8] or NULL*/, const float *edge_w /*[8] or NULL*/,
                  int N, int K, int D, float slope, float *attn /*[N,K]*/, float *hprime, int ldh, void *stream);
int cova_gat2_workspace_floats(int N, int K, int D);
int cova_gat2_bwd(const float *g, int ldg, const float *Wh, int ldw, const float *attn, const int64_t *ctx,
                  const float *att_w /*[D]*/, const float *phi /*[N,K,8] or NULL*/, const float *edge_w /*[8] or NULL*/,
                  int N, int K, int D, float slope, float *dWh /*[N,2D]*/, int lddw, float *d_att_w /*[D]*/,
                  float *d_att_b /*[1]*/, float *d_edge_w /*[8] or NULL*/, const int *csr, float *du /*[N,K]*/,
                  float *workspace, void *stream);
/* ---- attention dropout (opt-in: CoVA(attention_dropout=p); Velickovic et al., ICLR 2018, section 3.3) ----
 * Inverted dropout on the softmax output of both scoring modes.  For the flat slot e = i*K + k:
 *   keep[e]   = hash_uniform(seed, e) >= p     (f32 compare; the counter hash of cova_dropout_fwd, element e of stream seed)
 *   alphad[e] = keep[e] ? attn[e] * inv : 0    inv = 1.f / (1.f - p), ONE rounded f32 multiply
 *   h'[i]     = sum_k alphad[i,k] * Wh[ctx[i,k], D:2D]      (pads weigh 0, slot order as without dropout)
 * attn [N,K] as written is the softmax output BEFORE dropout, bit-equal to the plain entry point's.  Backward:
 *   dattn[e] = keep[e] ? (g[i] . Wh[j, D:2D]) * inv : 0;   du = attn * (dattn - sum_k attn * dattn) [* LeakyReLU'] -- a dropped
 *   slot still takes -attn * sum through the softmax -- and the destination side weighs g[i] with alphad[e].
 * No mask is stored: the forward, the source-side and the destination-side kernels regenerate keep from (seed, e) and form
 * alphad by the same expression.  A row whose valid slots are all dropped has h' = 0 and passes no gradient.  The same
 * launches as the plain entry points, on the DROP instantiations of the wave-per-node kernels: fixed summation orders, no
 * float atomics, bit-identical reruns for one seed.
 * cova_gat_fwd_drop / cova_gat_bwd_drop: cova_gat_fwd / cova_gat_bwd, or with phi and edge_w (backward: and d_edge_w and
 * workspace) -- all of the group or none -- cova_gat_fwd_edge / cova_gat_bwd_edge.  cova_gat2_fwd_drop / cova_gat2_bwd_drop:
 * cova_gat2_fwd / cova_gat2_bwd.  p outside [0, 1) (NaN included), a mismatched group and every bad argument of the plain
 * entry points return COVA_ERR_BAD_ARG before anything is launched; N == 0 is COVA_OK where the plain entry point has it
 * (not in cova_gat_bwd_drop). */
int cova_gat_fwd_drop(const float *Wh, int ldw, const float *att_w /*[2D]*/, const float *att_b /*[1]*/,
                      const int64_t *ctx /*[N,K]*/, const float *phi /*[N,K,8] or NULL*/, const float *edge_w /*[8] or NULL*/,
                      int N, int K, int D, float slope, float p, unsigned long long seed, float *s /*[N]*/,
                      float *t /*[N]*/, float *attn /*[N,K]*/, float *hprime, int ldh, void *stream);
int cova_gat_bwd_drop(const float *g, int ldg, const float *Wh, int ldw, const float *s, const float *t,
                      const float *attn, const int64_t *ctx, const float *att_w, const float *phi /*[N,K,8] or NULL*/,
                      const float *edge_w /*[8] or NULL*/, int N, int K, int D, float slope, float p,
                      unsigned long long seed, float *dWh /*[N,2D]*/, int lddw, float *ds /*[N]*/, float *dt /*[N]*/,
                      float *d_att_w /*[2D]*/, float *d_att_b /*[1]*/, float *d_edge_w /*[8] or NULL*/, const int *csr,
                      float *du /*[N,K]*/, float *workspace /*or NULL*/, void *stream);
int cova_gat2_fwd_drop(const float *Wh, int ldw, const float *att_w /*[D]*/, const float *att_b /*[1]*/,
                       const int64_t *ctx /*[N,K]*/, const float *phi /*[N,K,8] or NULL*/,
                       const float *edge_w /*[8] or NULL*/, int N, int K, int D, float slope, float p,
                       unsigned long long seed, float *attn /*[N,K]*/, float *hprime, int ldh, void *stream);
int cova_gat2_bwd_drop(const float *g, int ldg, const float *Wh, int ldw, const float *attn, const int64_t *ctx,
                       const float *att_w /*[D]*/, const float *phi /*[N,K,8] or NULL*/,
                       const float *edge_w /*[8] or NULL*/, int N, int K, int D, float slope, float p,
                       unsigned long long seed, float *dWh /*[N,2D]*/, int lddw, float *d_att_w /*[D]*/,
                       float *d_att_b /*[1]*/, float *d_edge_w /*[8] or NULL*/, const int *csr, float *du /*[N,K]*/,
                       float *workspace, void *stream);

/* ------------------------------------------------------------------ decoder tail, loss, optimizer
 * replaces: nn.Dropout (models.py:84,88), nn.Linear(T, n_classes) (models.py:89),
 * nn.CrossEntropyLoss(reduction="sum") + output.argmax(dim=1) (main.py:139, train.py:53,56),
 * torch.optim.Adam(lr, weight_decay).step() (main.py:133-135, train.py:60). */
int cova_dropout_fwd(const float *x, int ldx, float *out, int ldo, uint8_t *mask /*[R,C]*/,
                     long long R, int C, float p, unsigned long long seed, int mask_given,
                     void *stream);
int cova_dropout_bwd(const float *g, int ldg, const uint8_t *mask, float *dx, int ldx, long long R,
                     int C, float p, void *stream);
int cova_linear_small_fwd(const float *x, int ldx, const float *W /*[NC,Cin]*/, const float *b,
                          float *y /*[N,NC]*/, int N, int Cin, int NC, void *stream);
int cova_linear_small_bwd(const float *dy, const float *x, int ldx, const float *W, float *dx,
                          int lddx, float *dW, float *db, int N, int Cin, int NC, void *stream);
int cova_ce_sum(const float *logits, const int64_t *labels /*nullable*/, int N, int NC, float gscale,
                float *loss /*nullable [1]*/, float *dlogits /*nullable*/, int64_t *pred /*nullable*/,
                void *stream);
int cova_adam_step(float *p, const float *g, float *m, float *v, long long n, int step, double lr,
                   double beta1, double beta2, double eps, double weight_decay, void *stream);
int cova_colsum(const float *x, int ldx, int R, int C, float *out, void *stream);

/* ------------------------------------------------------------------ parameter-group optimizers (optim.hip)
 * replaces: torch.optim.Adam / torch.optim.AdamW / torch.optim.SGD(param_groups).step() and
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) for HotPathTrainer(optimizer=, param_groups=,
 * max_grad_norm=).
 * segs: DEVICE int64 [n_seg][4] = {lo, hi, group, start}: row r updates elements [lo, hi) of p / g / m / v with the
 * hyper-parameters of group `group`; `start` = the sum of the lengths of rows 0..r-1, total = the sum of all lengths.
 * Rows must not overlap (frozen tensors are simply left out); 0 <= lo <= hi <= n, or the row is skipped.
 * groups: HOST double [n_groups][9] = lr, weight_decay, beta1, beta2, eps, momentum, dampening, nesterov (0/1),
 * momentum buffer exists (0/1); n_groups <= 16.  Read at launch time (kernel arguments: no copy, no synchronisation);
 * bias corrections come from `step` in double as in cova_adam_step.
 * algo 0 = adam: L2 added to the gradient; per element the arithmetic of cova_adam_step (one group = its bits);
 * algo 1 = adamw: p *= 1 - lr*wd, then the Adam update without the L2 term;
 * algo 2 = sgd (torch semantics): g += wd*p (wd != 0); with momentum != 0: buf = g on a group's first step (buffer
 *          flag 0), else buf = momentum*buf + (1-dampening)*g; g = nesterov ? g + momentum*buf : buf; p -= lr*g.
 *          m = momentum buffer (nullable when every momentum is 0), v unused (nullable).
 * gscale (nullable, DEVICE [1]): multiplied into g as it is loaded (the clip coefficient of cova_grad_norm); g itself
 * is not written. */
int cova_optim_step(int algo, float *p, const float *g, float *m, float *v, long long n, const long long *segs, int n_seg,
                    long long total, const double *groups, int n_groups, int step, const float *gscale, void *stream);
/* doubles of cova_grad_norm's workspace for `total` elements (one partial per block of its first launch) */
int cova_grad_norm_workspace_doubles(long long total);
/* global L2 norm of the segments of g (same table; group ignored), deterministic: per-block sums of squares in double over
 * fixed slices, folded in a fixed order by a second launch (no float atomics: reruns and ranks holding the same
 * gradients get the same bits).  out: DEVICE float [2] = norm, clip coefficient min(1, max_norm / (norm + 1e-6)) in f32 as torch computes
 * it; a non-finite norm propagates (NaN -> NaN coefficient, inf -> 0), error_if_nonfinite=False. */
int cova_grad_norm(const float *g, long long n, const long long *segs, int n_seg, long long total, double max_norm,
                   double *workspace, float *out, void *stream);
/* ------------------------------------------------------------------ weight averaging (optim.hip)
 * replaces: torch.optim.swa_utils.AveragedModel.update_parameters (equal-weight running mean, SWA) and timm's
 * ModelEmaV2.update (exponential moving average) for HotPathTrainer(average=).
 * Per element of the table's rows, with w = (float)one_minus_decay converted once on the host:
 *   avg[i] = avg[i] + w * (p[i] - avg[i])
 * the difference, the product and the sum each rounded to f32 on their own (no fused multiply-add): a numpy float32
 * statement bit for bit, with p[i] == avg[i] a fixed point.  EMA: one_minus_decay = 1 - decay; SWA: 1 / (n_averaged + 1).
 * segs: the table of cova_optim_step ({lo, hi, group, start}, group ignored) under the same rules: rows must not
 * overlap; a row outside 0 <= lo <= hi <= n is skipped and never written; elements outside the rows (gaps, alignment
 * padding, frozen tensors) are not touched.  n_seg == 0 or total == 0: no launch, returns 0.  One launch, no atomics, no
 * workspace, no host read. */
int cova_weight_average(float *avg, const float *p, long long n, const long long *segs, int n_seg, long long total,
                        double one_minus_decay, void *stream);
/* ------------------------------------------------------------------ gradient accumulation (optim.hip)
 * replaces: the implicit `.grad +=` of several loss.backward() calls between two optimizer.step() calls and the
 * `loss / accum_steps` scaling that goes with it, for HotPathTrainer(accumulate_steps=).
 * g is the gradient bucket the backward overwrites at every micro-batch, acc the accumulator of the same layout.  Per
 * element i of the table's rows that also lies in the clip range [clip_lo, clip_hi) of flat elements, with
 * s = (float)scale converted once on the host:
 *   mode 0 (open):      acc[i] = g[i]                     acc is not read: no memset, garbage (NaN) in it is harmless
 *   mode 1 (add):       acc[i] = acc[i] + g[i]
 *   mode 2 (close):     g[i]   = acc[i] * s               g is not read
 *   mode 3 (add-close): g[i]   = (acc[i] + g[i]) * s
 * the sum and the product each rounded to f32 on their own (no fused multiply-add): a numpy float32 statement bit for
 * bit in a fixed order, and with scale == 1.0 the result is the sum's bits.  g is only read in modes 0 and 1, acc only
 * read in modes 2 and 3.
 * segs: the table of cova_optim_step ({lo, hi, group, start}, group ignored) under the rules of cova_weight_average:
 * rows must not overlap; a row outside 0 <= lo <= hi <= n is skipped and never written; elements outside the rows
 * (gaps, alignment padding, frozen tensors) or outside the clip keep their bits in both buffers.  The clip may cut a row
 * at any element, aligned or not (it is clamped to [0, n]); an empty clip launches nothing.  n_seg == 0 or total == 0: no
 * launch, returns 0; total > n is an error.  One launch, no atomics, no workspace, no host read. */
int cova_grad_accumulate(int mode, float *acc, float *g, long long n, const long long *segs, int n_seg, long long total,
                         long long clip_lo, long long clip_hi, double scale, void *stream);
/* ------------------------------------------------------------------ configurable criterion (loss.hip)
 * replaces: F.cross_entropy(logits, labels, weight=, ignore_index=, label_smoothing=, reduction="sum" | "mean"), the focal
 * loss, and the per-step .item() reads of loss and accuracy (train.py:54,57), for HotPathTrainer(class_weight=,
 * label_smoothing=, focal_gamma=, ignore_index=, loss_reduction=, track_metrics=) and models.CrossEntropyLoss.
 * cova_ce_sum stays the criterion of a trainer without those options.
 * Per kept row n with label y, p = softmax(l_n), C = NC, w = class_weight (1 when NULL):
 *   focal_gamma == 0: (1-eps) w[y] (-log p_y) + (eps/C) sum_k w[k] (-log p_k), eps = label_smoothing in [0, 1);
 *   focal_gamma >= 1: w[y] (1-p_y)^gamma (-log p_y), label_smoothing must be 0; 1-p_y = sum of the other p_k.
 * A row whose label equals ignore_index (has_ignore_index != 0) is skipped: no loss, a zero dlogits row, in no count.  A
 * row whose label is outside [0, NC) and not the ignore label is skipped the same way and counted as a bad label.  No
 * logit is read out of bounds.  NC <= 16.
 * Two phases, so that the denominator can be summed over ranks between them:
 * fwd: acc DEVICE double [3] = loss numerator, denominator (sum of w[y] over kept rows), kept rows; pred (nullable) =
 *   per-row argmax as cova_ce_sum (first maximum wins, every row); metrics (nullable) DEVICE int64 [NC*NC + 4], ADDED
 *   to: [label*NC + pred] confusion counts of kept rows, [NC*NC] kept rows, [NC*NC+1] bad labels, and, as float64 bit
 *   patterns, [NC*NC+2] numerator and [NC*NC+3] denominator running sums.  workspace: DEVICE double
 *   [cova_ce_loss_workspace_doubles(N)], any contents.
 * bwd: reads acc_total[0..1] from DEVICE memory; reduction_mean == 0: loss = numerator, dlogits unscaled; != 0: both
 *   divided by the denominator (a zero denominator gives loss 0 and dlogits 0).  grad_scale (nullable, DEVICE [1]) is
 *   multiplied into dlogits (autograd's incoming gradient).  loss_out (f32 [1]) and dlogits ([N,NC]) are each nullable.
 * Row arithmetic in f32 as cova_ce_sum; sums over rows in float64 over fixed 2048-row slices folded in a fixed order:
 * bit-reproducible, a function of N alone, no float atomics, no host read.  Defaults (no weight, eps = gamma = 0, no
 * ignore label, sum) give cova_ce_sum's dlogits and pred bit for bit and its loss to one f32 ulp. */
int cova_ce_loss_workspace_doubles(int N);
int cova_ce_loss_fwd(const float *logits, const int64_t *labels, int N, int NC, const float *class_weight /*nullable [NC]*/,
                     double label_smoothing, double focal_gamma, long long ignore_index, int has_ignore_index,
                     double *acc, int64_t *pred /*nullable [N]*/, int64_t *metrics /*nullable*/, double *workspace,
                     void *stream);
int cova_ce_loss_bwd(const float *logits, const int64_t *labels, int N, int NC, const float *class_weight /*nullable [NC]*/,
                     double label_smoothing, double focal_gamma, long long ignore_index, int has_ignore_index,
                     const double *acc_total, int reduction_mean, const float *grad_scale /*nullable*/,
                     float *loss_out /*nullable*/, float *dlogits /*nullable*/, void *stream);
/* per-page hard-negative mining (mine.hip; HotPathTrainer(hard_negative_ratio=, hard_negative_min=) and
 * models.CrossEntropyLoss(hard_negative_ratio=)): between the forward and cova_ce_loss_fwd, every page keeps its positives
 * and its k hardest background rows; the other background rows get drop_label (the criterion's ignore label) in labels_out.
 * Page p owns rows [s_p, e_p), s_p = clamp(page_start[p], 0, N), e_p = clamp(page_start[p+1], s_p, N) (page_start DEVICE
 * int64 [B+1], non-decreasing by the caller's contract; otherwise the only guarantee is that no access is out of bounds).
 * A row of a page is positive when 1 <= label < NC, background when label == 0; any other label (the caller's ignore
 * label, a bad label) is neither and passes through.  Quota, in float64 on the device:
 *   q = max((double)min_keep, floor(ratio * (double)n_pos)),  k_p = q >= n_bg ? n_bg : (int)q.
 * Score of a row: its cross-entropy against background, s = lse - l[0], in f32 with cova_ce_loss_fwd's row arithmetic
 * (max, expf sum, m + logf(se)); class weights, smoothing and the focal term play no part.  Key (uint32): 0x7FC00000 when
 * s is NaN (above +inf: a NaN row is kept and surfaces in the loss), the bits of s when s > 0, else 0.
 *   rank_n = #{background rows j of the page: key_j > key_n, or key_j == key_n and j < n}
 *   labels_out[n] = drop_label for a background row with rank_n >= k_p, else labels[n].
 * Every one of the N entries of labels_out is written; rows before page_start[0] or from page_start[B] on keep their label.
 * score_out (nullable) receives s_n of every row n in [0, N), counts (nullable) DEVICE int32 [B,3] = n_pos, n_bg, k_p.
 * 2 <= NC <= 16, B >= 1, N >= 1, ratio finite and >= 0, min_keep >= 0; any page size (0, 1, thousands of rows: a page of
 * more than 2048 rows walks its keys in LDS tiles).  One launch, one block per page, no workspace, no atomics, no host
 * read: bit-reproducible, a page's result does not depend on the batch around it. */
int cova_hard_negative_select(const float *logits, const int64_t *labels, const int64_t *page_start, int B, int N, int NC,
                              double ratio, int min_keep, long long drop_label, int64_t *labels_out /*[N]*/,
                              float *score_out /*nullable [N]*/, int *counts /*nullable [B,3]*/, void *stream);
/* per-page listwise ranking loss (rank.hip; HotPathTrainer(page_rank_weight=) and models.CrossEntropyLoss(page_rank_weight=)):
 * the training term over the lists cova_eval_page_ranks ranks.  Page p owns rows [s_p, e_p), clamped as for
 * cova_hard_negative_select above (page_start DEVICE int64 [B+1], non-decreasing by the caller's contract; otherwise the
 * only guarantee is that no access is out of bounds).  A list is (page p, class c), c in 1..NC-1, with v_n = logits[n, c].
 * A row of the page is a candidate when 0 <= label < NC and it does not carry the ignore label (has_ignore_index != 0 and
 * label == ignore_index); a candidate is a target of the list when label == c.  Rows with the ignore label or a bad
 * label, and rows outside [page_start[0], page_start[B]), take no part.  A list with at least one target is scored:
 *   L_pc       = lse_candidates(v) - lse_targets(v)                     (one target t: lse - v_t)
 *   dL_pc/dv_n = softmax_cand(v)_n - [n is a target] softmax_tgt(v)_n
 * Arithmetic, so that a list's result is a function of its page's rows alone: per list one wave; the two maxima m are
 * f32 compares (a NaN never wins); each term is expf(v - m) in f32; the terms are summed in float64, lane i taking the
 * page's rows i, i + 64, ... in turn, then the xor butterfly (offsets 32, 16, .., 1); lse = (double)m + log(sum) in
 * double.  lists DEVICE float64 [B, NC-1, 4] = lse of the candidates, lse of the targets, candidate count, target count;
 * an unscored list writes its counts and zeros for the lse fields.  acc DEVICE float64 [3] = sum w_c L_pc, sum w_c and
 * the number of scored lists, w_c = class_weight[c] (1 when NULL), folded from the table by one wave (lane i: lists i,
 * i + 64, ...; then the butterfly).  The rank term is R = acc[0] ("sum") or acc[0] / acc[1] ("mean"; a zero denominator
 * gives 0 and a zero gradient); under data parallelism acc is all-reduced between the two calls.
 * cova_page_rank_loss_bwd, per candidate row n and class c >= 1 of a scored list:
 *   x = (float)((double)v - lseA),  d = g * (expf(x) - [target] expf((float)((double)v - lseT))),
 *   g = (float)(rank_weight * s * w_c), times grad_scale[0] when given (DEVICE [1]); s = 1 or 1 / acc[1].
 * accumulate != 0: d is added to dlogits[n, c] and (float)(rank_weight * R) to loss_inout[0] (one f32 add each; every
 * other entry keeps its bits; the call is stream-ordered after the cova_ce_loss_bwd that wrote them).  accumulate == 0:
 * every entry of dlogits [N, NC] and the loss are written; column 0, non-candidates, rows outside the pages and unscored
 * lists get zeros.  No multiply-add is fused.  2 <= NC <= 16, B >= 1, N >= 1, rank_weight finite and >= 0; at least
 * one of loss_inout / dlogits.  Forward: two launches; backward: one, a thread per row.  No atomics, no workspace beyond
 * lists, no host read; non-finite logits reach their own list only. */
int cova_page_rank_loss_fwd(const float *logits, const int64_t *labels, const int64_t *page_start, int B, int N, int NC,
                            const float *class_weight /*nullable*/, long long ignore_index, int has_ignore_index,
                            double *lists /*[B,NC-1,4]*/, double *acc /*[3]*/, void *stream);
int cova_page_rank_loss_bwd(const float *logits, const int64_t *labels, const int64_t *page_start, int B, int N, int NC,
                            const float *class_weight /*nullable*/, long long ignore_index, int has_ignore_index,
                            const double *lists, const double *acc_total, double rank_weight, int reduction_mean,
                            const float *grad_scale /*nullable*/, float *loss_inout /*nullable*/,
                            float *dlogits /*nullable*/, int accumulate, void *stream);
/* ---- page readout (readout.hip; opt-in: CoVA(page_context_dim=G); Li et al. 2016, PyG AttentionalAggregation) ----
 * One attention-pooled vector per page, handed to every box of the page.  P [N, G] (rows at P + n*ldp) are the projected
 * own features; page p owns rows [s_p, e_p), clamped as for cova_hard_negative_select above (page_start DEVICE int64 [B+1]).
 *   u_i = att_w . P_i + att_b[0],  e_i = u_i > 0 ? u_i : alpha * u_i   (u == +-0 takes the alpha branch, as cova_gat2_fwd)
 *   beta_i = exp(e_i - max_p e) / sum_p exp(e_j - max_p e),  r_p = sum_{i in p} beta_i P_i,  out[i, 0:G] = r_page(i)
 * cova_page_readout_fwd writes u [N], beta [N], r [B, G] and the rows out + n*ldo of every box of a page; an empty page
 * writes nothing (its row of r included), rows outside [page_start[0], page_start[B]) are not written.
 * cova_page_readout_bwd, given g = dL/dout (rows at g + n*ldg) and gr_p = sum_{i in p} g_i:
 *   de_i = beta_i (gr_p . P_i - gr_p . r_p),  du_i = de_i * (u_i > 0 ? 1 : alpha),  dP_i = beta_i gr_p + du_i att_w,
 *   d_att_w = sum_i du_i P_i [G],  d_att_b = sum_i du_i [1]
 * writes dP (rows at dP + n*lddp) of every box of a page and d_att_w / d_att_b through per-page partials in ws
 * (cova_page_readout_workspace_floats(B, G) = B * (G + 1) floats; 0 for B <= 0 or G outside [1, 512]), folded over pages in
 * ascending order by a second launch.
 * A block of sixteen waves per page; waves stride over the page's rows, lanes over channels: float4 chunks when G % 4 == 0
 * and every base and leading dimension is 16-byte aligned, scalar otherwise.  All sums are f32 in a fixed order that is a
 * function of the page's own row count and G alone: a dot product is a lane's channels ascending as one fma chain, then
 * the xor butterfly (offsets 32 .. 1); the maximum is per wave over rows w, w + 16, ... (f32 compares), then waves 0..15;
 * the softmax denominator is thread t over rows t, t + 1024, ..., the butterfly, then the tree of adjacent pairs over the
 * waves, ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) ...; r_p, gr_p and the d_att partials are per wave over rows w,
 * w + 16, ... in turn, then the same tree.  So reruns are bit-identical,
 * a page's u, beta, r, out and dP keep their bits whatever other pages share the batch, and nothing depends on an atomic
 * or a host read.  LDS is bounded by G and the block size: a page of any length runs.
 * 1 <= G <= 512, N >= 0, B >= 0, ld* >= G, else COVA_ERR_BAD_ARG before anything is launched; N == 0 or B == 0 launches
 * nothing and needs no pointer; otherwise a NULL operand is COVA_ERR_BAD_ARG.  Forward: one launch; backward: two. */
int cova_page_readout_workspace_floats(int B, int G);
int cova_page_readout_fwd(const float *P, int ldp, const float *att_w /*[G]*/, const float *att_b /*[1]*/,
                          const int64_t *page_start /*[B+1]*/, int B, int N, int G, float alpha, float *u /*[N]*/,
                          float *beta /*[N]*/, float *r /*[B,G]*/, float *out, int ldo, void *stream);
int cova_page_readout_bwd(const float *g, int ldg, const float *P, int ldp, const float *u, const float *beta,
                          const float *r, const float *att_w, const int64_t *page_start, int B, int N, int G, float alpha,
                          float *dP, int lddp, float *d_att_w /*[G]*/, float *d_att_b /*[1]*/, float *ws, void *stream);
/* ---- page self-attention (page_attn.hip; opt-in: CoVA(page_attention_dim=E, page_attention_heads=Hh)) ----
 * Multi-head scaled dot-product self-attention restricted to pages.  qkv [N, 3E] (rows at qkv + n*ldq) holds [Q | K | V];
 * head a owns the columns a*dh .. a*dh + dh of each third, dh = E / Hh.  Page p owns rows [s_p, e_p), clamped as for
 * cova_page_readout_fwd above (page_start DEVICE int64 [B+1]).  For a row i of page p and a head a:
 *   s_ij = (Q_i . K_j) * (1 / sqrt(dh)) over ALL rows j of page p (i included),  A_ij = softmax_j s_ij,  O_i = sum_j A_ij V_j
 * cova_page_attn_fwd writes O (out + n*ldo, E columns) and lse [N, Hh] = max_j s_ij + log sum_j exp(s_ij - max) of every row
 * of a page; an empty page writes nothing, rows outside [page_start[0], page_start[B]) are not written.  No probability is
 * stored: cova_page_attn_bwd, given g = dL/dO (rows at g + n*ldg), recomputes A_ij = exp(s_ij - lse_i) and writes
 *   delta_i = g_i . O_i,  dA_ij = g_i . V_j,  ds_ij = A_ij (dA_ij - delta_i)
 *   dQ_i = sum_j ds_ij K_j / sqrt(dh),  dK_j = sum_i ds_ij Q_i / sqrt(dh),  dV_j = sum_i A_ij g_i
 * as [dQ | dK | dV] into dqkv (rows at dqkv + n*lddq) for every row of a page.
 * Both products of every kernel run on the f32 matrix pipe (v_mfma_f32_16x16x4_f32); a block of four waves per (page, head,
 * tile of 64 rows) walks the page's other rows through LDS in ascending tiles (two passes in the forward: maximum, then
 * sums), so a page of any length runs.  Every summation order is a function of the page's own row count, E and Hh alone
 * (page_attn.hip's header lists them): reruns are bit-identical, a page's rows keep their bits whatever other pages share
 * the batch, and nothing depends on an atomic, a host read or a workspace.
 * out, g and dqkv rows may sit at any leading dimension and alignment (16-byte stores where aligned, scalar otherwise); qkv
 * must be 16-byte aligned with ldq % 4 == 0.  1 <= Hh, Hh divides E, E <= 512, dh a multiple of 4 in [4, 128], N >= 0,
 * B >= 0, ldq >= 3E, lddq >= 3E, ldo >= E, ldg >= E, else COVA_ERR_BAD_ARG before anything is launched; N == 0 or B == 0
 * launches nothing and needs no pointer; otherwise a NULL operand is COVA_ERR_BAD_ARG.  Forward: one launch; backward: two
 * (query side, key side). */
int cova_page_attn_fwd(const float *qkv, int ldq, const int64_t *page_start /*[B+1]*/, int B, int N, int E, int Hh,
                       float *out, int ldo, float *lse /*[N,Hh]*/, void *stream);
int cova_page_attn_bwd(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                       const float *lse /*[N,Hh]*/, const int64_t *page_start /*[B+1]*/, int B, int N, int E, int Hh,
                       float *dqkv, int lddq, void *stream);
/* ---- box-geometry bias of the page self-attention (page_attn.hip, the GEO instantiations; opt-in:
 * CoVA(page_attention_geometry=True)) ----
 * The pair above with a relative-geometry term on every score, formed inside the kernels from the two boxes of the pair
 * (no [n, n, 8] table exists).  bboxes [N,5] = page,x1,y1,x2,y2 as cova_edge_geometry reads them; geo_w [Hh, 8], one row of
 * weights per head; img_w, img_h the page size in pixels.  For rows i, j of one page and head a:
 *   phi_ij = the eight f32 features of cova_edge_geometry with box a = the QUERY i, box b = the KEY j, dj = j - i
 *            (one definition, csrc/geometry.h: the same bits, correctly rounded divisions included)
 *   b_ij   = fma chain from +0 over e = 0..7 of geo_w[a][e] * phi_ij[e]
 *   s_ij   = (Q_i . K_j) * (1 / sqrt(dh)) + b_ij          one rounded multiply, then one rounded add
 * and A, O, lse as for cova_page_attn_fwd on these s_ij.  The diagonal i = j is a pair like any other (phi_ii has IoU 1
 * for a box with area).  With geo_w == 0 every output has the plain pair's bits.  The boxes have no gradient.
 * cova_page_attn_bwd_geo: ds_ij = A_ij (dA_ij - delta_i) with A recomputed from the biased scores against lse; dQ, dK, dV
 * keep their expressions; d_geo_w[a][e] = sum over pages, i, j of ds_ij * phi_ij[e], every entry of [Hh, 8] written.  Its
 * order (page_attn.hip's header): on the query side a lane's fma chain over its pairs (tiles, sub-tiles, r ascending), the
 * xor butterfly 32 .. 1 over the wave, the block's four waves in wave order, eight sums per block into workspace
 * [blocks][8] (blocks = B * Hh * ceil(N / 64), block = (page * Hh + head) * ceil(N / 64) + tile; a block behind its page's
 * end writes zeros), then one fold launch per (head, e) over pages ascending and a page's tiles ascending.  No atomics, no
 * host read: reruns are bit-identical, d_geo_w included; O, lse and dqkv rows of a page keep their bits whatever other
 * pages share the batch.  Every workspace entry is written before it is read; the caller need not clear it.
 * cova_page_attn_geo_workspace_floats(B, N, Hh) = 8 * B * Hh * ceil(N / 64) floats; 0 for B <= 0, N <= 0, Hh < 1 or a
 * count beyond an int.
 * Refusals are those of the plain pair, plus img_w <= 0 or img_h <= 0 (always), and, where N > 0 and B > 0, a NULL bboxes,
 * geo_w, d_geo_w or workspace or a workspace count beyond an int: COVA_ERR_BAD_ARG before anything is launched.  N == 0
 * or B == 0 launches nothing, needs no pointer and leaves d_geo_w unwritten.  Forward: one launch; backward: three (query
 * side, key side, fold). */
int cova_page_attn_geo_workspace_floats(int B, int N, int Hh);
int cova_page_attn_fwd_geo(const float *qkv, int ldq, const int64_t *page_start /*[B+1]*/, const float *bboxes /*[N,5]*/,
                           const float *geo_w /*[Hh,8]*/, float img_w, float img_h, int B, int N, int E, int Hh, float *out,
                           int ldo, float *lse /*[N,Hh]*/, void *stream);
int cova_page_attn_bwd_geo(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                           const float *lse /*[N,Hh]*/, const int64_t *page_start /*[B+1]*/, const float *bboxes /*[N,5]*/,
                           const float *geo_w /*[Hh,8]*/, float img_w, float img_h, int B, int N, int E, int Hh, float *dqkv,
                           int lddq, float *d_geo_w /*[Hh,8]*/, float *workspace, void *stream);
/* ---- dropout on the page attention's probabilities (page_attn.hip, the DROP instantiations; opt-in:
 * CoVA(page_attention_dropout=p) and, as site 0 of every encoder layer, CoVA(page_encoder_dropout=p)) ----
 * replaces: the dropout_p of F.multi_head_attention_forward / F.scaled_dot_product_attention in train mode (the `dropout`
 * argument of nn.MultiheadAttention inside nn.TransformerEncoderLayer): F.dropout on softmax(s) before the product with V.
 * Inverted dropout at rate p, inv = 1.f / (1.f - p) (one f32 division).  The score of (query batch row i, head a, key batch
 * row j) is kept (D_ij = 1) when hash_uniform(seed, ((uint64)(i * Hh + a) << 32) | (uint64)j) >= p, compared in f32.  No mask
 * and no probability is stored: the forward and both sides of the backward regenerate D from the same integers and form
 * the dropped value by one helper, ONE rounded multiply v * inv on a kept score and +0 on a dropped one.
 *   A_ij = softmax_j s_ij as in the plain pair (with the geometry bias in the _geo_ forms); lse is the UNDROPPED one, bit-equal
 *   to the plain forward's on the same inputs (row maximum and sum run over all keys)
 *   O_i = sum_j D_ij inv A_ij V_j
 *   delta_i = g_i . O_i,  dA_ij = D_ij inv (g_i . V_j),  ds_ij = A_ij (dA_ij - delta_i)       (a dropped score still takes
 *   -A_ij delta_i through the softmax),  dV_j = sum_i (D_ij inv A_ij) g_i;  dQ, dK and d_geo_w follow from ds as before.
 * Summation orders, launches and workspace are those of the plain pairs.  A row whose keys are all dropped has O = 0 and
 * zero dqkv rows.  D depends on (seed, i, a, j) alone: reruns are bit-identical, and a page keeps its bits whatever other
 * pages share the batch as long as it occupies the same batch rows.
 * Refusals are those of the plain (or _geo) pair, plus p outside (0, 1) (NaN included) or N * Hh >= 2**32: COVA_ERR_BAD_ARG
 * before anything is launched. */
int cova_page_attn_fwd_drop(const float *qkv, int ldq, const int64_t *page_start /*[B+1]*/, int B, int N, int E, int Hh,
                            float *out, int ldo, float *lse /*[N,Hh]*/, float p, unsigned long long seed, void *stream);
int cova_page_attn_bwd_drop(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                            const float *lse /*[N,Hh]*/, const int64_t *page_start /*[B+1]*/, int B, int N, int E, int Hh,
                            float *dqkv, int lddq, float p, unsigned long long seed, void *stream);
int cova_page_attn_fwd_geo_drop(const float *qkv, int ldq, const int64_t *page_start /*[B+1]*/,
                                const float *bboxes /*[N,5]*/, const float *geo_w /*[Hh,8]*/, float img_w, float img_h,
                                int B, int N, int E, int Hh, float *out, int ldo, float *lse /*[N,Hh]*/, float p,
                                unsigned long long seed, void *stream);
int cova_page_attn_bwd_geo_drop(const float *g, int ldg, const float *qkv, int ldq, const float *out, int ldo,
                                const float *lse /*[N,Hh]*/, const int64_t *page_start /*[B+1]*/,
                                const float *bboxes /*[N,5]*/, const float *geo_w /*[Hh,8]*/, float img_w, float img_h,
                                int B, int N, int E, int Hh, float *dqkv, int lddq, float *d_geo_w /*[Hh,8]*/,
                                float *workspace, float p, unsigned long long seed, void *stream);
/* ---- row kernels of the page encoder (page_encoder.hip; opt-in: CoVA(page_encoder_dim=P)) ----
 * LayerNorm over the C channels of each of R rows (rows at x + r*ldx), float32:
 *   mean_r = sum_c x_rc / C,  rstd_r = 1 / sqrt(sum_c (x_rc - mean_r)^2 / C + eps)   (the biased variance, formed in TWO
 *   passes over the row, which a wave holds in registers: never E[x^2] - mean^2),
 *   out_rc = ((x_rc - mean_r) * rstd_r) * weight_c + bias_c       (the last two operations one fma)
 * cova_layernorm_fwd writes out (rows at out + r*ldo), mean [R] and rstd [R].
 * cova_layernorm_bwd, given g = dL/dout (rows at g + r*ldg), with xhat = (x - mean) * rstd re-formed from the saved mean
 * and rstd by the forward's own operations and gw = g * weight:
 *   dx_rc = (res ? res_rc : 0) + rstd_r * ((gw_rc - sum_c gw_rc / C) - xhat_rc * (sum_c gw_rc xhat_rc / C))
 *   dweight_c = sum_r g_rc xhat_rc,  dbias_c = sum_r g_rc                 every entry of [C] written
 * res (nullable; rows at res + r*ldr) is the gradient already on the residual stream: the add is fused, and res may BE dx
 * (in place: an element is read and written by the one lane that owns it).  g and x must not alias dx.
 * One wave per row, lanes over channels: float4 chunks lane, lane + 64 when C % 4 == 0 and every base and leading
 * dimension is 16-byte aligned, scalar channels otherwise; no LDS in the forward, LDS only for the wave combine in the
 * backward.  Orders (all f32): a row sum is a lane's channels ascending (plain adds; an fma chain for the two sums of
 * products), then the xor butterfly (offsets 32 .. 1).  dweight / dbias: a block of four waves owns the rows
 * [32 b, 32 b + 32); wave w adds the rows 32 b + w, + 4, ... ascending, the waves combine in wave order into the
 * workspace [blocks][2][C], and a fold launch sums the blocks ascending.  cova_layernorm_workspace_floats(R, C) =
 * ceil(R / 32) * 2 * C floats; 0 for R <= 0 or C outside [1, 512] (a negative value for a count beyond an int).  Every
 * workspace entry is written before it is read.  Plain stores only, no host read: every order is a function of (R, C) alone, so
 * reruns are bit-identical, and a row's out, mean, rstd and dx do not depend on the rows around it.
 * 1 <= C <= 512, R >= 0, eps >= 0, ld* >= C, else COVA_ERR_BAD_ARG before anything is launched; R == 0 launches nothing and
 * needs no pointer; otherwise a NULL operand (res excepted) is COVA_ERR_BAD_ARG.  Forward: one launch; backward: two.
 * GELU, exact (erf) form, elementwise over R rows of C values:
 *   cova_gelu_fwd: out = 0.5 z (1 + erff(z / sqrt 2));  cova_gelu_bwd: dz = g (0.5 (1 + erff(z / sqrt 2)) + z expf(-z^2 / 2) / sqrt(2 pi))
 * z == 0 gives out == 0 and dz == 0.5 g exactly.  float4 under the alignment rule above, scalar otherwise; one grid-stride
 * launch each.  C >= 1, R >= 0, ld* >= C, else COVA_ERR_BAD_ARG; R == 0 launches nothing and needs no pointer; otherwise a
 * NULL operand is COVA_ERR_BAD_ARG.  The operands of one call must not alias. */
int cova_layernorm_workspace_floats(int R, int C);
int cova_layernorm_fwd(const float *x, int ldx, int R, int C, const float *weight /*[C]*/, const float *bias /*[C]*/,
                       float eps, float *out, int ldo, float *mean /*[R]*/, float *rstd /*[R]*/, void *stream);
int cova_layernorm_bwd(const float *g, int ldg, const float *x, int ldx, const float *mean /*[R]*/,
                       const float *rstd /*[R]*/, const float *weight /*[C]*/, int R, int C, const float *res /*nullable*/,
                       int ldr, float *dx, int lddx, float *dweight /*[C]*/, float *dbias /*[C]*/, float *ws, void *stream);
int cova_gelu_fwd(const float *z, int ldz, long long R, int C, float *out, int ldo, void *stream);
int cova_gelu_bwd(const float *g, int ldg, const float *z, int ldz, long long R, int C, float *dz, int lddz, void *stream);
/* ---- dropout of the page encoder's sublayers (page_encoder.hip; opt-in: CoVA(page_encoder_dropout=p)) ----
 * replaces: the `dropout`, `dropout1` and `dropout2` submodules of nn.TransformerEncoderLayer(norm_first=True) in train
 * mode (F.dropout on the FFN hidden activations and on each sublayer's output before its residual add).
 * Inverted dropout at rate p, inv = 1.f / (1.f - p) (one f32 division): element (r, c) of an [R, C] operand is kept when
 * hash_uniform(seed, r * C + c) >= p, compared in f32 (cova_dropout_fwd's convention).  No mask is stored: a backward
 * regenerates it from the same (seed, r * C + c).  Every `* inv` is ONE rounded f32 multiply; a dropped element is +0.
 *   cova_gelu_fwd_drop      out = keep ? gelu(z) * inv : 0           (gelu as cova_gelu_fwd; z stays the saved tensor)
 *   cova_gelu_bwd_drop      dz  = keep ? (g * inv) * gelu'(z) : 0    (gelu' as cova_gelu_bwd, from the same saved z)
 *   cova_dropout_add_fwd    out = x + (keep ? y * inv : 0)           two roundings; out may be neither y nor x
 *   cova_dropout_regen_bwd  dy  = keep ? g * inv : 0                 dy may not be g
 * float4 under the alignment rule of the GELU pair, scalar otherwise; one grid-stride launch each; reruns are bit-identical.
 * 0 < p < 1 (NaN refused), C >= 1, R >= 0, ld* >= C, else COVA_ERR_BAD_ARG before anything is launched; R == 0 launches
 * nothing, writes nothing and needs no pointer; otherwise a NULL or aliased operand is COVA_ERR_BAD_ARG. */
int cova_gelu_fwd_drop(const float *z, int ldz, long long R, int C, float *out, int ldo, float p, unsigned long long seed,
                       void *stream);
int cova_gelu_bwd_drop(const float *g, int ldg, const float *z, int ldz, long long R, int C, float *dz, int lddz, float p,
                       unsigned long long seed, void *stream);
int cova_dropout_add_fwd(const float *y, int ldy, const float *x, int ldx, float *out, int ldo, long long R, int C, float p,
                         unsigned long long seed, void *stream);
int cova_dropout_regen_bwd(const float *g, int ldg, float *dy, int lddy, long long R, int C, float p,
                           unsigned long long seed, void *stream);
/* evaluation decision (train.py:131-153): per page and class column, page-local indices of the k
 * highest-scoring boxes, best first; page_start [n_pages+1] are box offsets; out [n_pages,NC,k] */
int cova_page_class_topk(const float *logits, const int64_t *page_start, int n_pages, int NC, int k,
                         int64_t *out, void *stream);
/* evaluation of a split (eval.hip; train.py:131-154 over a whole loader, for evaluation.evaluate_split): page p of the
 * batch owns boxes page_start[p] .. page_start[p+1] (DEVICE int64 [B+1]).  For class c in 1..NC-1 let t be the lowest
 * page-local index with labels == c (the [0, 0] of train.py:151).  rank[row, c-1] = number of boxes j of the page with
 * v_j > v_t, or v_j == v_t and j < t, in column c: the position of the labelled box in cova_page_class_topk's order (score
 * descending, ties to the lower index), so "the labelled box is among the top k" is 0 <= rank < k for every k.  A page
 * without a box of class c gets -1.  top1[row, c-1] (nullable) = page-local index of the best box of the column in that
 * order, -1 for an empty page.  row = page_ids[p] (DEVICE int32 [B]), or p when page_ids is NULL; a row outside [0, P) is
 * skipped (the host validates ids), rows of pages not in the batch are not written (the caller pre-fills the [P, NC-1]
 * int32 tables with -2 = not evaluated).  Labels outside [0, NC) match no class.  Any page size (0, 1, thousands of
 * boxes); 2 <= NC <= 16.  One launch, one wave per (page, class), no workspace, no atomics, no host read. */
int cova_eval_page_ranks(const float *logits, const int64_t *labels, const int64_t *page_start,
                         const int *page_ids /*nullable [B]*/, int B, int NC, int P, int *rank,
                         int *top1 /*nullable [P,NC-1]*/, void *stream);
/* joint page decoding (decode.hip; evaluate_split / predict_split / HotPathTrainer.evaluate / fit with decode="joint"): one
 * DISTINCT box per non-background class, the most probable labelling of a page that holds exactly one box of each class.
 * Page p of the batch owns rows [page_start[p], page_start[p+1]) as for cova_eval_page_ranks (DEVICE int64 [B+1],
 * non-decreasing by the caller's contract; a negative start counts as 0, an end below its start as an empty page).  n is
 * its box count, C = NC - 1, i the page-local index.
 *   score of box i for class c in 1..C, float32: score_mode 0 ("logit") logits[i, c]; score_mode 1 ("map")
 *     logits[i, c] - logits[i, 0], one float32 subtraction.  A NaN score counts as -inf.
 *   order of a column: score descending, ties to the lower index (cova_page_class_topk's order).
 *   candidates of class c: the first m = min(n, C + 1) boxes of its column in that order.
 *   assignment: a tuple of ranks (r_1..r_C), each in [0, m), whose candidate boxes are pairwise distinct.
 *   total: the float64 sum of the C float32 scores, added in class order ((s_1 + s_2) + s_3) ...; a NaN total counts as -inf.
 *   result: the assignment with the greatest total, among equal totals the lexicographically smallest rank tuple;
 *     choice[row, c-1] = page-local index of class c's box.
 *   gap[row] (nullable, float64) = the best total minus the greatest total of any other assignment: +inf when there is no
 *     other assignment, 0 on a tie (also when both totals are -inf, or both +inf).
 *   0 < n < C (the classes cannot all be served): choice is the column decision (the first of each column's order),
 *     gap = +inf.  n = 0: choice = -1, gap = +inf.
 *   hit[row, c-1] (nullable; needs labels): 1 when labels[choice] == c, 0 when not, -1 when the page has no box labelled c.
 * labels is nullable when hit is NULL.  row = page_ids[p] (DEVICE int32 [B]), or p when page_ids is NULL; a row outside
 * [0, P) is skipped, rows of pages not in the batch are not written (the caller pre-fills choice and hit with -2 and gap
 * with -1.0, so one all-reduce(MAX) merges the tables of several ranks).  Any page size (0, 1, thousands of boxes);
 * 2 <= NC <= 7 (7^6 = 117649 tuples at most) and score_mode in {0, 1}, else a status and no launch.  Only additions and
 * compares, none contracted or reordered; tests/decode_oracle.py is the numpy statement.  One launch, one block per page,
 * no workspace, no atomics, no host read: a page's result does not depend on the batch around it. */
int cova_page_joint_decode(const float *logits, const int64_t *labels /*nullable*/, const int64_t *page_start,
                           const int *page_ids /*nullable [B]*/, int B, int NC, int P, int score_mode,
                           int *choice /*[P,NC-1]*/, int *hit /*nullable [P,NC-1]*/, double *gap /*nullable [P]*/,
                           void *stream);

/* ---- device-side input pipeline --------------------------------------
 * ToTensor of datasets.py:41-45,96-97: u8 [B,H,W,3] -> f32 [B,3,H,W], value/255 (bit-exact) */
int cova_images_u8_to_f32(const uint8_t *u8_nhwc, float *f32_nchw, int B, int H, int W, void *stream);
/* WebDataset.__getitem__ box part + custom_collate_fn (datasets.py:110-128,159-178):
 * rows [N,5] = x,y,w,h,label of B pages back to back, page_offsets int32 [B+1] (device) ->
 * bboxes [N,5] = page,x1,y1,x2,y2; labels [N] i64; ctx [N,2*context_size] i64 batch-global ids, -1 pads */
int cova_collate_boxes(const float *rows, const int *page_offsets, int B, int N, int context_size,
                       float *bboxes, long long *labels, long long *ctx /*nullable if context_size==0*/,
                       void *stream);
/* ---- device-resident dataset: page gather, background-box sampling, collation of the kept boxes ----
 * cova_pages_u8_gather_f32: cova_images_u8_to_f32 of the pages page_idx[0..B) (DEVICE int32, each in [0,P)) of a
 *   resident u8 [P,H,W,3] store -> f32 [B,3,H,W]; the same arithmetic, bit-identical results; page offsets are 64-bit
 *   (the store may exceed 4 GiB).  The host checks the index list; an index outside [0,P) leaves its output page unwritten.
 * cova_sample_boxes (datasets.py:101-110): page p of the batch owns n = page_offsets[p+1] - page_offsets[p] boxes
 *   (page_offsets DEVICE int32 [B+1], page_offsets[B] = N); its box i is row row_starts[p] + i of `rows` ([*,5] =
 *   x,y,w,h,label; row_starts DEVICE int32 [B], NULL: page_offsets[p], the rows of the batch back to back).  Box i is kept
 *   if its rank among the page's (key, i) pairs -- smaller key first, ties to the lower i -- is < keep_counts[p] (DEVICE
 *   int32 [B]; the host computes int(sampling_fraction * n) in float64 as the reference does), or if rows[.,4] != 0 (the
 *   float test of datasets.py:106).  sel (int32 [N]) receives the kept SOURCE row ids in ascending order, first N_out
 *   valid; out_offsets (int32 [B+1]) the page offsets of the kept boxes, out_offsets[B] = N_out.  Any n is valid (0, 1,
 *   thousands), and so is a page that keeps nothing.
 *   keys (nullable): DEVICE int64 [N], non-negative, compared as integers, keys[page_offsets[p] + i] for box i (tests
 *   inject the reference's permutation: key[perm[j]] = j).  NULL: the key is 63 bits of a counter hash,
 *       mix(s, x) = z ^ (z >> 31),  z = (z ^ (z >> 27)) * 0x94D049BB133111EB,  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9,
 *                   z = s + 0x9E3779B97F4A7C15 * (x + 1)              (all modulo 2^64; the mixer of the dropout masks)
 *       key(p, i) = mix(mix(stream_seed, pid), i) >> 1,   pid = page_ids[p] (DEVICE int32 [B]), or p when page_ids is NULL
 *   so a page's sample depends on (stream_seed, pid) alone -- not on the batch it lands in, its position, the batch size,
 *   the rank or the world size.  The host folds seed and epoch: stream_seed = mix(mix(0, seed), epoch).
 *   workspace: DEVICE int32 [cova_sample_boxes_workspace_ints(B, N)] = N + B, any contents.  Two launches, no atomics, no
 *   host read: bit-deterministic.
 * cova_collate_selected: cova_collate_boxes over the kept boxes: box g of the output is source row sel[g], its page the
 *   p with out_offsets[p] <= g < out_offsets[p+1]; the context window runs over the kept boxes of the page (the reference
 *   builds it after sampling, datasets.py:117-128).  addl_out [N_out,A] = addl_in[sel[g], :] (both nullable when A == 0).
 *   N_out is a host value (out_offsets[B], the one host read of a sampled batch).  Bit-exact as cova_collate_boxes. */
int cova_pages_u8_gather_f32(const uint8_t *store_u8, const int *page_idx, int P, int B, int H, int W, float *f32_nchw,
                             void *stream);
int cova_sample_boxes_workspace_ints(int B, int N);
int cova_sample_boxes(const float *rows, const int *page_offsets, const int *row_starts /*nullable*/,
                      const int *page_ids /*nullable*/, const int *keep_counts, int B, int N,
                      const long long *keys /*nullable*/, unsigned long long stream_seed, int *workspace, int *sel,
                      int *out_offsets, void *stream);
int cova_collate_selected(const float *rows, const int *sel, const int *out_offsets, int B, int N_out, int context_size,
                          float *bboxes, long long *labels, long long *ctx /*nullable if context_size==0*/,
                          const float *addl_in /*nullable if A==0*/, int A, float *addl_out /*nullable if A==0*/,
                          void *stream);
/* ---- page augmentation in the page gather (augment.hip; pipeline.PageAugment, DeviceDataset.batches(augment=)) ----
 * The reference augments nothing: an opt-in extension.  The host draws, per page, an integer viewport shift (dx, dy) and a
 * 3x4 affine colour transform as a function of (seed, epoch, page id) and uploads them once per epoch.
 * cova_pages_u8_augment_f32: cova_pages_u8_gather_f32 with both applied; f32_nchw [B,3,H,W].  For output page b, channel c,
 *   row y, column x:
 *     source page = page_idx[b] (DEVICE int32 [B]), or b itself when page_idx is NULL (then P >= B, else a status); an index
 *       outside [0,P) leaves the output page unwritten, as the gather does
 *     sx = x - dx_b, sy = y - dy_b in 64 bits (shift DEVICE int32 [B,2] = dx,dy, any int32 value; NULL = 0,0)
 *     v_k (k = R,G,B) = the source byte at (sy, sx) when 0 <= sx < W and 0 <= sy < H, else byte k of fill_rgb = 0xRRGGBB
 *     t_k = (float)v_k / 255.f, correctly rounded: the arithmetic of cova_images_u8_to_f32
 *     y_c = ((m[4c]*t_0 + m[4c+1]*t_1) + m[4c+2]*t_2) + m[4c+3],  m = color[b] (DEVICE f32 [B,12], row-major 3x4, m[4c+3] the
 *       offset; NULL = the identity), float32 with EVERY multiply and add rounded on its own (no fused multiply-add)
 *     out = y_c > 0 ? fminf(y_c, 1.f) : 0.f          in [0,1], never -0, 0 for a NaN
 *   With the identity y_c is exactly t_c, so NULL / zero shift and NULL / identity colour give the bits of
 *   cova_pages_u8_gather_f32.  tests/augment_oracle.py is the numpy statement.  Page offsets are 64-bit (the store may exceed
 *   4 GiB); no thread reads a byte outside [store_u8, store_u8 + P*H*W*3).  With W % 4 == 0, store_u8 4-byte and f32_nchw
 *   16-byte aligned a thread makes 4 pixels of a row from the aligned dwords that cover their 12 source bytes (any dx);
 *   otherwise a pixel-per-thread kernel writes the same bytes.  H, W, P >= 1, store_u8 and f32_nchw non-NULL, else a status;
 *   B == 0 returns without a launch.  One launch, no workspace, no atomics, no host read: capturable, bit-deterministic.
 * cova_boxes_translate: boxes moved with the pixels, in place.  Row g of bboxes [N,5] = page,x1,y1,x2,y2: p = (int)bboxes[g,0];
 *   if 0 <= p < B, columns 1 and 3 += (float)dx_p and columns 2 and 4 += (float)dy_p (one float32 add each), otherwise the row
 *   is untouched.  Nothing is clipped or dropped: RoIPool / RoIAlign clamp, a box pushed off the page pools zeros.  N == 0
 *   returns without a launch (no pointer is read); N < 0 or B < 0, and for N > 0 a NULL bboxes or shift or B == 0, return a
 *   status.  One launch, one thread per box. */
int cova_pages_u8_augment_f32(const uint8_t *store_u8, const int *page_idx /*nullable*/, int P, int B, int H, int W,
                              const int *shift /*nullable [B,2]*/, const float *color /*nullable [B,12]*/, int fill_rgb,
                              float *f32_nchw, void *stream);
int cova_boxes_translate(float *bboxes, int N, const int *shift, int B, void *stream);
/* ---- page zoom in the page gather (augment.hip; pipeline.PageAugment(scale=)) ----
 * cova_pages_u8_resample_f32: cova_pages_u8_augment_f32 with the integer shift replaced by a bilinear resample in 16.16 fixed
 *   point with 8-bit weights; integer arithmetic up to one correctly rounded division.  step DEVICE int32 [B,2] = inv_x, inv_y
 *   (source pixels per output pixel, times 65536), origin DEVICE int64 [B,2] = org_x, org_y (the source position of output
 *   pixel (0,0), times 65536; fraction 0 = exactly pixel i).  For output page b, row y, column x, channel c:
 *     p_x = org_x + x*inv_x, p_y = org_y + y*inv_y                       in int64
 *     i = p >> 16 (arithmetic: the floor), f = (p >> 8) & 255           per axis
 *     the taps i and i+1 of an axis carry the integer weights 256 - f and f
 *     a tap (ix, iy) with 0 <= ix < W and 0 <= iy < H is the page's byte v_c, any other tap byte c of fill_rgb = 0xRRGGBB
 *     q_c = sum over the four taps of wy*wx*byte_c                      an integer <= 255*65536 = 16711680 < 2^24
 *     t_c = (float)q_c / 16711680.f, correctly rounded
 *     then color[b] (nullable: the identity) and the clamp exactly as cova_pages_u8_augment_f32 (unfused, never -0, NaN -> 0)
 *   A tap of weight 0 changes nothing, wherever it lies.  With inv = 65536 on both axes and org = (-dx*65536, -dy*65536) the
 *   output is bit-equal to cova_pages_u8_augment_f32 with shift = (dx, dy) (q_c = 65536*v_c, and the quotient is v_c/255's).
 *   page_idx, P, B, an index outside [0,P) (the page stays unwritten), the 64-bit page offsets and the statuses are those of
 *   cova_pages_u8_augment_f32; step and origin are required (NULL with B > 0 is a status).  Every address is formed from
 *   a position already tested against (or clipped to) the page, so no table contents make a thread read outside the store;
 *   the arithmetic above holds for 1 <= inv <= 2^22 and |org| < 2^62.  With W % 4 == 0, store_u8 4-byte and f32_nchw 16-byte
 *   aligned a thread makes 4 pixels of a row; a page with 1 <= inv_x <= 131072 then takes its taps from the row segments its
 *   wave staged in LDS (clipped to the page, the fill colour beside them), any other inv_x one by one from the store.  Otherwise a pixel-per-thread kernel writes the same bytes.  tests/resample_oracle.py is
 *   the numpy statement.  One launch, no workspace, no atomics, no host read: capturable, bit-deterministic.
 * cova_boxes_affine: cova_boxes_translate with a scale.  affine DEVICE f32 [B,4] = sx, sy, tx, ty; under the same guard on the
 *   page column (NaN, negative, >= B: the row stays) x' = x*sx + tx for columns 1 and 3, y' = y*sy + ty for columns 2 and 4,
 *   one float32 multiply then one float32 add, not fused.  With sx = sy = 1 and integer tx, ty: the bits of
 *   cova_boxes_translate.  N == 0 returns without a launch; N < 0 or B < 0, and for N > 0 a NULL pointer or B == 0, a status. */
int cova_pages_u8_resample_f32(const uint8_t *store_u8, const int *page_idx /*nullable*/, int P, int B, int H, int W,
                               const int *step /*[B,2]*/, const long long *origin /*[B,2]*/,
                               const float *color /*nullable [B,12]*/, int fill_rgb, float *f32_nchw, void *stream);
int cova_boxes_affine(float *bboxes, int N, const float *affine /*[B,4]*/, int B, void *stream);
/* ---- context graphs (graph.hip; pipeline.DeviceCollate / DeviceDataset(spatial_k=)) ----
 * cova_context_knn: the context table with spatial neighbours, ctx [N, 2*context_size + k_spatial] int64 batch-global ids,
 *   -1 pads.  bboxes [N,5] = page,x1,y1,x2,y2 exactly as cova_collate_boxes / cova_collate_selected wrote them (the page
 *   column is not read); page p owns boxes page_offsets[p] .. page_offsets[p+1] (DEVICE int32 [B+1], page_offsets[B] = N:
 *   the page_offsets of cova_collate_boxes, the out_offsets of cova_sample_boxes).  The graph runs over the boxes it is
 *   given, i.e. over the KEPT boxes of a sampled page (the reference builds its window after sampling, datasets.py:117-128).
 *   For box i (page-local index) of a page with n boxes:
 *   columns 0 .. 2*context_size: the DOM-order window exactly as cova_collate_boxes writes it: max(0,i-cs) .. i-1, then
 *     i+1 .. min(n-1,i+cs), page-local index + page_offsets[p], trailing -1.  The collate kernels are called with
 *     context_size = 0 and ctx = NULL in this mode: this one launch writes the whole table.
 *   the remaining k_spatial columns: the nearest other boxes of the same page, nearest first.  Box i itself and every j
 *     with |i-j| <= context_size (the window's members) are excluded, so a row never names a neighbour twice; with fewer
 *     than k_spatial candidates the tail is -1.  Candidates are ordered lexicographically by (gap2, ctr2, j), smallest
 *     first, in float32 with EVERY operation rounded on its own (no fused multiply-add):
 *       dx = max(0, max(x1_i,x1_j) - min(x2_i,x2_j)), dy likewise     the gap between the rectangles, 0 where they overlap
 *       gap2 = (dx*dx) + (dy*dy)
 *       sx = x1 + x2, sy = y1 + y2, ex = sx_i - sx_j, ey = sy_i - sy_j
 *       ctr2 = (ex*ex) + (ey*ey)                                       four times the squared centre distance
 *     Both keys are sums of squares: non-negative and, for finite boxes, not NaN, so their bit patterns order as unsigned
 *     integers and the kernel compares ((bits(gap2) << 32) | bits(ctr2), j).  tests/graph_oracle.py is the numpy statement.
 *   Any n is valid (0, 1, thousands).  N == 0 or a table of width 0 returns without a launch (no pointer is read).
 *   context_size >= 0, k_spatial >= 0, 2*context_size + k_spatial <= 1024 (the K of cova_gat_fwd).  Non-finite
 *   coordinates: the launch stays memory-safe and every id written is -1 or a valid id of the page, without repeats; the
 *   order is unspecified (the host refuses such rows).  A page_offsets table that does not hold box g writes a row of -1.
 *   One launch (one wave per box), no workspace, no atomics, no host read: capturable and bit-deterministic. */
int cova_context_knn(const float *bboxes, const int *page_offsets, int B, int N, int context_size, int k_spatial,
                     long long *ctx, void *stream);
/* cova_edge_geometry: phi [N,K,8] float32 (16-byte aligned), the relative geometry of every edge of a context table; computed
 *   once per batch and shared by every head and layer.  Slot k of box i, neighbour j = ctx[i,k] (batch-global id), boxes =
 *   columns 1..4 of bboxes [N,5], w = x2 - x1, h = y2 - y1, W = img_w, H = img_h (pixels).  float32, EVERY operation rounded on
 *   its own (no fused multiply-add), `/` correctly rounded:
 *     phi0 = ((x1_j + x2_j) - (x1_i + x2_i)) / (2*W)           phi1 likewise in y with H     centre offset
 *     phi2 = (w_j - w_i) / ((w_j + w_i) + 1)                   phi3 likewise with h          size contrast
 *     phi4 = max(0, max(x1_i,x1_j) - min(x2_i,x2_j)) / W       phi5 likewise in y with H     the gap of cova_context_knn
 *     phi6 = uni > 0 ? inter / uni : 0                                                       IoU, with
 *            iw = max(0, min(x2_i,x2_j) - max(x1_i,x1_j)), ih likewise, inter = iw*ih, uni = ((w_i*h_i) + (w_j*h_j)) - inter
 *     phi7 = clamp(j - i, -64, 64) / 64                                                      DOM-order offset (exact)
 *   A pad (j < 0) or an id >= N (a pad to the GAT kernels too) gives eight zeros; no box is read for it.  Bit-equal to the
 *   numpy float32 statement (tests/edge_oracle.py) for finite boxes with x2 >= x1, y2 >= y1; anything else is memory-safe and
 *   deterministic.  One launch, one thread per slot: no LDS, no workspace, no atomics, no host read, capturable. */
int cova_edge_geometry(const float *bboxes, const long long *ctx, int N, int K, float img_w, float img_h, float *phi,
                       void *stream);
/* attention export rows (extract_attn_wts_and_visualize.py:104-135): out [N, 5+5K] =
 * x,y,w,h,label, K x (x,y,w,h) of the context boxes (0 for pads), K attention weights */
int cova_attn_export_rows(const float *bboxes, const long long *ctx, const float *attn,
                          const long long *labels, int N, int K, float *out, void *stream);

/* ---- cached RoI visual features (feat.hip; features.FeatureCache) ----
 * out[g*ld_out + c] = table[row_ids[g]*C + c] for c < C: rows row_ids[0..N) (DEVICE int32, the SOURCE row ids `sel` of
 * cova_sample_boxes) of a dense f32 table [R, C] into the first C columns of out (leading dimension ld_out >= C, e.g.
 * comb[:, :n_vis] with ld_out = T).  Columns C..ld_out of out are not touched.  Row offsets into the table are 64-bit (the
 * table may exceed 4 GiB).  A row id outside [0, R) writes a row of zeros (memory-safe and defined; the host refuses such
 * ids where it knows them).  float4 loads and stores when C % 4 == 0, ld_out % 4 == 0 and both bases are 16-byte aligned,
 * else a scalar path with the same bytes out (an odd T makes every row start of comb unaligned).  N == 0 returns without
 * a launch.  One launch, no atomics, no workspace, capturable. */
int cova_feat_rows_gather(const float *table /*[R,C] dense*/, long long R, int C, const int *row_ids /*DEVICE int32 [N]*/,
                          int N, float *out, int ld_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COVA_HIP_H */
