/*
 * cwf_hip.h -- C ABI of libcwf_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * ClsWiseFormer forward/backward hot path.
 *
 * The reference (mathwrx/Decouple-and-Couple_Learning_in_Multi-Modal_Brain_Tumor_Segmentation) is
 * pure Python over ATen; it owns no native code, so there is no reference FFI to mirror.  Each entry
 * point below replaces the ATen op sequence the cited reference lines dispatch, and is what the
 * reference-side ctypes stub in INTEGRATION.md binds.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless named h_*.
 *   - activations are fp32, channels-last: [N][D][H][W][C] ("NDHWC"); a tensor argument is
 *     (ptr, ldc) where ldc = floats between consecutive voxels (>= C, multiple of 4; ptr 16-B aligned).
 *     Channel slices / zero-copy concatenation are expressed by offsetting ptr and keeping ldc.
 *   - token matrices are row-major [B][T][E].
 *   - no allocation, no host synchronisation, no ownership transfer inside; work buffers are passed in.
 *   - every call enqueues on `stream` (a hipStream_t passed as void*) and returns 0 on success,
 *     a negative CWF_E_* for argument errors, or the positive hipError_t of the failed launch.
 *   - arithmetic: fp32 in / fp32 accumulate; contractions use v_mfma_f32_16x16x4_f32 (exact f32).
 */
#ifndef CWF_HIP_H
#define CWF_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CWF_E_BADARG   (-1)
#define CWF_E_TOOLARGE (-2)
#define CWF_E_ALIGN    (-3)

int cwf_version(void);            /* ABI version, bumped on any signature change */
const char* cwf_arch(void);       /* "gfx950" */

/* ------------------------------------------------------------------------------------------------
 * K1  implicit-GEMM 3-D convolution family on MFMA (fwd and data-gradient of every conv in the model)
 *
 * op selects the geometry; all share one tap-table driven kernel:
 *   CWF_CONV3_S1      3x3x3, stride 1, pad 1      nn.Conv3d(k=3,p=1)        Unet_skipconnection.py:26,42,46
 *   CWF_CONV3_S2      3x3x3, stride 2, pad 1      EnDown                     Unet_skipconnection.py:63
 *   CWF_CONV1         1x1x1                       down_channel/DeUp/endconv  cls_wise_former.py:623,719,721,642
 *   CWF_CONVT2        ConvTranspose3d k=2 s=2     DeUp_Cat.conv2             cls_wise_former.py:720
 *   CWF_CONV3_S2_DGRAD  data gradient of CWF_CONV3_S2 (x = dy at half res, y = dx at full res)
 *   CWF_CONVT2_DGRAD    data gradient of CWF_CONVT2   (x = dy at double res, y = dx)
 *   (the data gradients of CONV3_S1 / CONV1 are the same ops with flipped / transposed packed weights)
 *
 * y = out_scale[n,co] * ( sum_taps sum_ci act(x*in_scale[n,ci]+in_shift[n,ci]) * W + bias[co] + residual )
 *   act(v) = v > 0 ? v : in_slope*v   (in_slope 0 = ReLU, 0.01 = LeakyReLU, 1 = identity); zero padding is
 *   applied AFTER the activation (pads the activated tensor, as conv(relu(IN(x))) does).
 *   in_scale/in_shift, bias, residual, out_scale may be NULL.
 * stats (nullable): double [N][Cout][2], accumulates sum(y), sum(y*y) per (n, co)  -- the InstanceNorm
 *   statistics of the output, fused into the epilogue.  Must be zeroed by the caller.
 * Input dims (Di,Hi,Wi,Cin), output dims (Do,Ho,Wo,Cout) are the tensor extents of x and y.
 *
 * precision selects the MFMA operand form (activations and weights stay fp32 in HBM in every form):
 *   CWF_FP32    v_mfma_f32_16x16x4_f32, exact f32; wpk packed by cwf_gather_batched ([class][ci_chunk16][tap][co_tile16][lane64][4])
 *   CWF_BF16X3  split bf16 on v_mfma_f32_16x16x32_bf16: v = hi + lo per operand, hi.hi + hi.lo + lo.hi (~2^-16 per product)
 *   CWF_BF16    hi.hi only (2^-9 per product)
 *   The bf16 forms take wpk packed by cwf_gather_split_bf16 ([class][ci_chunk16][tap pair][co_tile16][lane64][hi 8 | lo 8]).
 *   Layouts and index maps: cwf/packing.py.
 * ---------------------------------------------------------------------------------------------- */
enum { CWF_CONV3_S1 = 0, CWF_CONV3_S2 = 1, CWF_CONV1 = 2, CWF_CONVT2 = 3, CWF_CONV3_S2_DGRAD = 4, CWF_CONVT2_DGRAD = 5 };
enum { CWF_FP32 = 0, CWF_BF16X3 = 1, CWF_BF16 = 2 };

/* One forward or data-gradient launch.  Zero-initialise the struct; every optional field is NULL / 0 when unused.  The library
 * chooses the kernel from the descriptor; a field that no kernel for the layer can honour makes the call return CWF_E_BADARG.
 *   nb_*     data gradients whose output g feeds the backward of act(IN(nb_x)) (Unet_skipconnection.py:31-77,
 *            cls_wise_former.py:157-204): stats receives per (n, channel) S1 = sum g*act'(h), S2 = sum g*act'(h)*h with
 *            h = nb_x*nb_scale + nb_shift (what cwf_in_bwd_stats computes in a pass of its own) instead of (sum y, sum y^2).
 *            bf16 forms only; stats required.
 *   x16      the input as a bf16 image [N][D][H][W][Cin] (x is then not read), zero16 = 16 zero bytes: the single-bf16 data gradient
 *            of a 3x3x3 stride-1 layer reading the image of dy that cwf_in_bwd_apply_ex wrote -- the 16 -> 16 layers of >= 32768
 *            voxels (EnBlock1 / EnBlock1_1 / DeBlock2 / DeBlock2_1) and the 32- / 64-channel layers at 64^3 / 32^3 that the
 *            weight-stationary kernel takes: exactly the layers for which cwf_conv_x16_ok answers 1; any other layer returns
 *            CWF_E_BADARG.  No prologue, no out_scale.  Results are those of the same launch reading the fp32 tensor.
 *   y16      also write the output as a bf16 image [N][Do*Ho*Wo][Cout] (DeUp_Cat.conv3, cls_wise_former.py:716-729: the input of the
 *            next block's first conv, whose weight gradient reads that image): in the same launch where the pointwise stream
 *            kernel takes the layer, otherwise by a cwf_to_bf16 pass after it.  No nb_x, no out_scale.
 *   w_raw    the raw nn.Conv3d weight of a forward launch: lets the stem (4 -> 16 channels, InitConv, Unet_skipconnection.py:22-33)
 *            and the first down-sampling layer (stride 2, 16 -> 32, EnDown1, :60-68) run kernels that read it directly.
 *   groups   2 or 3 channel-grouped 3x3x3 stride-1 convs in one launch (the three sub-regions' supervision-head convs,
 *            SuperviseLabel.py:58-81, EdgeSuperviseLabel.py:56-76): group q reads input channels [q*x_goff, q*x_goff + Cin) and
 *            writes output channels [q*y_goff, q*y_goff + Cout) of the same voxel rows with weights wpk_g[q] and bias bias_g[q]
 *            (wpk / bias unused).  Bias only: no prologue, residual, out_scale, statistics or images.  0 = an ordinary launch. */
struct cwf_conv_args {
  int op, precision;
  const float* x; int x_ldc; const void* wpk; const float* bias; float* y; int y_ldc;
  const float* in_scale; const float* in_shift; float in_slope;
  const float* residual; int r_ldc; const float* out_scale; double* stats;
  const float* nb_x; int nb_ldc; const float* nb_scale; const float* nb_shift; float nb_slope;
  const void* x16; const void* zero16; void* y16;
  const float* w_raw;
  int groups, x_goff, y_goff; const void* wpk_g[3]; const float* bias_g[3];
  int N, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout;
};
int cwf_conv(const struct cwf_conv_args* args /* host */, void* stream);
/* 1 if cwf_conv takes a single-bf16 3x3x3 stride-1 launch of these dimensions (Cin / Cout of the LAUNCH: for a data gradient the forward
 * layer's Cout / Cin) with its input as a bf16 image (x16); 0 otherwise.  Host code only; the same code the dispatch evaluates. */
int cwf_conv_x16_ok(int op, int N, int D, int H, int W, int Cin, int Cout);
/* Tests and tools: the route of the wave-specialised weight-in-LDS single-bf16 kernel (the data gradients of the 128 / 256-channel
 * 3x3x3 stride-1 layers at 16^3).  cwf_debug_wsd: 1 = the product route (default), 0 = never (the tap-table kernel's result), 2 = every
 * eligible launch whatever its size, 3 = as 2 with 32 output channels per workgroup wherever Cout allows; returns the previous value.
 * cwf_debug_wsd_launches: launches of that kernel so far (host-side count).  Results do not depend on the route: y bit-identical, the
 * statistics / norm-backward sums equal up to the order of their float64 summation. */
int cwf_debug_wsd(int v);
long long cwf_debug_wsd_launches(void);

/* Weight gradient (+ bias gradient) of the same family (op in {CONV3_S1, CONV3_S2, CONV1, CONVT2}):
 *   dW[tap][ci][co] = sum_{n,vox} act(x*in_scale+in_shift)[n, vox*is+tap, ci] * dy[n, vox, co]
 * in two launches: cwf_wgrad writes partial slabs (MFMA accumulator layout) into `partial` (cwf_wgrad_partial_floats() floats)
 * and reports how many in *nsplit_used (<= cwf_wgrad_nsplit()); cwf_wgrad_reduce sums the slabs in a fixed order (four
 * partial sums over the slabs k = l, l + 4, ... for l = 0..3, combined as (s0 + s1) + (s2 + s3): the order of
 * cwf_wgrad_reduce_batched, so both give the same bits) and scatters
 * through a host-built INVERSE map (int32 [slab_floats]: >= 0 index into dW ([Cout][Cin][k][k][k] as nn.Conv3d.weight), <= -2
 * bias index -2-v into db ([Cout], may be NULL), -1 padding).  The slab layout depends on (op, Cin, Cout) only.
 * Descriptor (zero-initialise; x / dy with their row pitches; precision as for cwf_conv):
 *   xa16 / dy16  both operands as bf16 images (xa16 = bf16(act(IN(x))) [N][D][H][W][Cin], dy16 [N][D][H][W][Cout]; x / dy are then
 *                not read), zero16 = 16 zero bytes: single-bf16 3x3x3 stride-1 layers, 16 -> 16 of >= 32768 voxels
 *                (EnBlock1 / EnBlock1_1 / DeBlock2 / DeBlock2_1) or Cin a multiple of 16 (>= 32) and Cout a multiple of 32
 *                (EnBlock2/3/4, DeBlock3/4, Enblock8, decouplers; Unet_skipconnection.py:36-57, cls_wise_former.py:691-754).
 *   dy_scale     dy is taken as dy * dy_scale[n][co]: the backward of the always-on dropout3d behind InitConv
 *                (Unet_skipconnection.py:29-33) folded into the stem's weight gradient; bf16 forms, 3x3x3 stride-1 layers with
 *                Cin <= 16, Cout = 16 and >= 32768 voxels.
 *   groups       2 or 3 same-shape 3x3x3 stride-1 layers in one launch: group q has its own activation view x_g[q], gradient view
 *                dy_g[q] (row pitches x_ldc / dy_ldc) and slab buffer partial_g[q] (each sized like a single layer's); no
 *                prologue; bf16 forms.  Reduce each group like a single layer.  0 = an ordinary launch.                  */
int cwf_wgrad_nsplit(int op, int N, int Do, int Ho, int Wo, int Cin, int Cout);
int64_t cwf_wgrad_partial_floats(int op, int N, int Do, int Ho, int Wo, int Cin, int Cout);
int64_t cwf_wgrad_slab_floats(int op, int Cin, int Cout);
struct cwf_wgrad_args {
  int op, precision;
  const float* x; int x_ldc; const float* in_scale; const float* in_shift; float in_slope;
  const float* dy; int dy_ldc;
  const float* dy_scale; const void* xa16; const void* dy16; const void* zero16;
  float* partial;
  int groups; const float* x_g[3]; const float* dy_g[3]; float* partial_g[3];
  int N, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout;
};
int cwf_wgrad(const struct cwf_wgrad_args* args /* host */, int* nsplit_used /* host out, nullable */, void* stream);
/* Tests and tools: the plan cwf_wgrad makes for a descriptor in a bf16 form (CWF_BF16, CWF_BF16X3; images and grouped launches
 * included) -- the same host code the launch runs, so what it answers is what the launch does.  Read-only: launches nothing and
 * dereferences no pointer of the descriptor (only their values and alignment count).  Returns what cwf_wgrad would return before
 * its launch (0 or a negative CWF_E_*; CWF_E_BADARG also for a plain CWF_FP32 descriptor, whose plan is cwf_debug_wgrad_fp32_plan's)
 * and on 0 fills out[CWF_WGB_PLAN_FIELDS]:
 *   [0] kernel instance (enum below)      [1..3] grid x, y, z                  [4] threads per workgroup
 *   [5] tile walk (CWF_WGB_WALK_*)        [6] tiles_per_split (WALK_RANGES), grid x (WALK_STRIDED), 4-voxel groups per wave (WALK_PW)
 *   [7] workgroups per sample (WALK_PW, else 0)                                [8] waves that share the walk (WALK_PW, else 0)
 *   [9] work items in all: spatial tiles of the launch; WALK_PW: 4-voxel groups per sample
 *   [10] slab floats                      [11] nsplit_used: slabs written       [12] operand form: 0 bf16 products, 1 exact fp32 products
 *   [13] fewest, [14] most work items of one workgroup (WALK_PW: of one workgroup's waves together)
 * Tile walks: WALK_RANGES    workgroup x = s takes tiles [s * tiles_per_split, min(tiles, (s + 1) * tiles_per_split));
 *             WALK_STRIDED   workgroup b of G takes tiles first, first + G, ... below tiles, first = (b & 7) * (G / 8) + (b >> 3);
 *             WALK_PW        workgroup b = n * wps + w works in sample n; its wave v takes the 4-voxel groups
 *                            [(w * waves + v) * gpw, min(groups, (w * waves + v + 1) * gpw)) of that sample (possibly none).
 * cwf_debug_wgrad_bf16_name: a short name of an instance id (NULL outside [0, CWF_WGB_COUNT)). */
enum cwf_wgrad_bf16_instance {
  CWF_WGB_WGRAD16 = 0, CWF_WGB_WGRAD16_X3,                               /* wgrad16_kernel<X3> */
  CWF_WGB_PW_1_1_1, CWF_WGB_PW_2_1_1, CWF_WGB_PW_4_2_1, CWF_WGB_PW_8_4_1, /* pw_wgrad_kernel<NCH, NTL, 1>: 1x1x1 */
  CWF_WGB_PW_1_1_8, CWF_WGB_PW_2_2_8,                                     /* pw_wgrad_kernel<NCH, NTL, 8>: ConvTranspose */
  CWF_WGB_S1_1, CWF_WGB_S1_2,                                             /* wgrad_s1_kernel<NTW> */
  CWF_WGB_TILED_7_1, CWF_WGB_TILED_7_1_X3, CWF_WGB_TILED_7_2, CWF_WGB_TILED_7_2_X3,        /* wgrad_bf16_kernel<7, NTW, true, X3> */
  CWF_WGB_TILED_2_1, CWF_WGB_TILED_2_1_X3, CWF_WGB_TILED_2_2, CWF_WGB_TILED_2_2_X3,        /* wgrad_bf16_kernel<2, NTW, false, X3> */
  CWF_WGB_TILED_2_4, CWF_WGB_TILED_2_4_X3,
  CWF_WGB_WGRAD16D, CWF_WGB_S1D,                                          /* wgrad16d_kernel, wgrad_s1d_kernel (bf16 images) */
  CWF_WGB_COUNT
};
enum { CWF_WGB_WALK_RANGES = 0, CWF_WGB_WALK_STRIDED = 1, CWF_WGB_WALK_PW = 2 };
#define CWF_WGB_PLAN_FIELDS 15
int cwf_debug_wgrad_bf16_plan(const struct cwf_wgrad_args* args /* host */, int64_t* out /* host, CWF_WGB_PLAN_FIELDS */);
const char* cwf_debug_wgrad_bf16_name(int instance);
/* Tests and tools: the route of the single-bf16 3x3x3 stride-2 launches behind CWF_WGB_TILED_7_1 / CWF_WGB_TILED_7_2 (fp32 operands, dy
 * 16-byte aligned with a row pitch that is a multiple of 4).  cwf_debug_wgrad_s2: 1 = wgrad_s2_kernel, which keeps all of a tile's
 * loads in flight (default), 0 = never (the tiled kernel wgrad_bf16_kernel); returns the previous value.
 * cwf_debug_wgrad_s2_launches: launches of that kernel so far (host-side count).  The plan that cwf_debug_wgrad_bf16_plan reports and
 * the slabs do not depend on the route: the slabs are bit-identical. */
int cwf_debug_wgrad_s2(int v);
long long cwf_debug_wgrad_s2_launches(void);
int cwf_wgrad_reduce(const float* partial, int nsplit, int64_t slab_floats,
                     const int32_t* inv_map, float* dW, float* db, void* stream);
/* every layer of a backward phase in one launch: table = DEVICE array of descriptors (same slab / inverse-map conventions as
 * cwf_wgrad_reduce); dW / db may point into one flat gradient buffer */
struct cwf_wgrad_reduce_desc { const float* partial; const int32_t* inv; float* dW; float* db; int64_t slab; int32_t nsplit; int32_t pad_; };
int cwf_wgrad_reduce_batched(const struct cwf_wgrad_reduce_desc* table, int nlayers, void* stream);

struct cwf_gather_desc { const float* src; float* dst; const int32_t* map; int64_t n; };

/* the bf16 packing: cwf_gather_batched's table, each value written as its bf16 hi and lo parts (the index map has one int32 per
 * bf16 element of the hi image, 8 per lane) */
int cwf_gather_split_bf16(const struct cwf_gather_desc* table, int nlayers, int64_t max_n, void* stream);

/* dst[i] = map[i] >= 0 ? src[map[i]] : 0 for a table of `nlayers` descriptors resident in device memory
 * (struct cwf_gather_desc).  Used once per step to pack every layer's weights for K1.               */
int cwf_gather_batched(const struct cwf_gather_desc* table, int nlayers, int64_t max_n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3  InstanceNorm3d (affine=False, eps)  nn.InstanceNorm3d -- Unet_skipconnection.py:13,39-45;
 *     cls_wise_former.py:207-223,697-700,737-742
 * ---------------------------------------------------------------------------------------------- */
/* stats double[NC][2] (sum, sumsq over V voxels) -> scale = rstd, shift = -mean*rstd  (float[NC] each) */
int cwf_in_finalize(const double* stats, float* scale, float* shift, int NC, int64_t V, float eps, void* stream);
/* sum / sumsq of a tensor that no conv epilogue produced */
int cwf_in_stats(const float* x, int x_ldc, double* stats, int N, int64_t V, int C, void* stream);
/* y = act(x*scale+shift) + residual                     EnBlock2/DeBlock tail, cls_wise_former.py:709-711,751-752 */
int cwf_norm_act_add(const float* x, int x_ldc, const float* scale, const float* shift, float slope,
                     const float* residual, int r_ldc, float* y, int y_ldc, int N, int64_t V, int C, void* stream);
/* backward of y = act(IN(x)): g = dy*act'(xhat);  sums[NC][2] += (sum g, sum g*xhat)  (zeroed by caller) */
int cwf_in_bwd_stats(const float* dy, int dy_ldc, const float* x, int x_ldc, const float* scale, const float* shift,
                     float slope, double* sums, int N, int64_t V, int C, void* stream);
/* dx = scale*(g - S1/V - xhat*S2/V) (+ dx_add if not NULL) */
int cwf_in_bwd_apply(const float* dy, int dy_ldc, const float* x, int x_ldc, const float* scale, const float* shift,
                     float slope, const double* sums, const float* dx_add, int a_ldc, float* dx, int dx_ldc,
                     int N, int64_t V, int C, void* stream);

/* cwf_in_bwd_apply with bf16 side outputs (each nullable; dx or dx16 must be given):
 *   dx16 [N*V][C] bf16 = bf16(dx)                 -- the gradient image the 16-channel weight-gradient kernel below takes
 *   xa16 [N*V][C] bf16 = bf16(act(x*scale+shift)) -- the activated input of the layer whose backward this is, i.e. the x operand of
 *                                                   its weight gradient (convolution_backward's `input`, Unet_skipconnection.py:39-56) */
int cwf_in_bwd_apply_ex(const float* dy, int dy_ldc, const float* x, int x_ldc, const float* scale, const float* shift,
                        float slope, const double* sums, const float* dx_add, int a_ldc, float* dx, int dx_ldc,
                        void* dx16, void* xa16, int N, int64_t V, int C, void* stream);
/* cwf_norm_act_add that also writes y16 [N*V][C] bf16 = bf16(y) (nullable) */
int cwf_norm_act_add_ex(const float* x, int x_ldc, const float* scale, const float* shift, float slope,
                        const float* residual, int r_ldc, float* y, int y_ldc, void* y16, int N, int64_t V, int C, void* stream);
/* y16 [N*V][C] bf16 = bf16(act(x*scale+shift))  (scale == NULL: bf16(x)) */
int cwf_to_bf16(const float* x, int x_ldc, const float* scale, const float* shift, float slope, void* y16,
                int N, int64_t V, int C, void* stream);
/* ------------------------------------------------------------------------------------------------
 * K6/K7  token path: LayerNorm, Linear (strided batched MFMA GEMM), softmax rows, GELU
 *        ResidualNorm.py:4-47, SelfAttention.py:74-102
 * ---------------------------------------------------------------------------------------------- */
/* C[z][m][n] = act( sum_k A[z](m,k)*B[z](k,n) + bias[n] ) + residual[z][m][n]
 * element strides are given explicitly so that NT / NN / TN products and per-head slices need no copies.
 * z = zb*H + zh with separate strides for the outer (zb) and inner (zh) batch index.
 * act: 0 none, 1 exact GELU (erf).  alpha scales the product (attention 1/sqrt(d)).                     */
int cwf_gemm(const float* A, int64_t sa_m, int64_t sa_k, int64_t sa_zb, int64_t sa_zh,
             const float* B, int64_t sb_k, int64_t sb_n, int64_t sb_zb, int64_t sb_zh,
             float* C, int64_t sc_m, int64_t sc_zb, int64_t sc_zh,
             const float* bias, const float* residual, int64_t sr_m, int64_t sr_zb, int64_t sr_zh,
             int M, int Nn, int K, int ZB, int ZH, float alpha, int act, int accumulate, void* stream);
/* Extended form: the same product with the fusions that keep a coupler block at a handful of launches.  Zero-initialise the
 * struct; fields beyond `accumulate` are optional.
 *   A2/split_n   output columns n >= split_n read A2 (same strides) instead of A: q = LN1(x) Wq^T and k|v = LN2(x2) Wkv^T over the
 *                reference's single [1536,512] qkv weight in ONE launch (SelfAttention.py:80-93); split_n % 64 == 0
 *   B2/split_m   output rows m >= split_m read B2: the weight gradient [dq^T a ; dkv^T b] of the same layer in one launch
 *   C2           receives alpha*AB + bias BEFORE the activation (the GELU input, kept for backward; ResidualNorm.py:40-41)
 *   rowsum       rowsum[m] (+)= sum_k A'(m,k): with A' = dy^T this is the bias gradient of a Linear, from one extra MFMA
 *   a_drop_*     A' = A * keep(offset of the element inside A): dropout of dy recomputed, not stored (backward of
 *                x + Dropout(Linear(.)), ResidualNorm.py:9-10,25-31); *_n = numel of the dropped tensor, p2 = a second chained dropout
 *   c_drop_*     epilogue order: alpha*AB + bias -> C2 -> act -> dropout -> + residual -> (accumulate) -> C
 *   rng          device uint64[2] {seed, step} (cwf_rng_advance)                                                           */
struct cwf_gemm_args {
  const float* A; int64_t sa_m, sa_k, sa_zb, sa_zh;
  const float* B; int64_t sb_k, sb_n, sb_zb, sb_zh;
  float* C; int64_t sc_m, sc_zb, sc_zh;
  const float* bias; const float* residual; int64_t sr_m, sr_zb, sr_zh;
  int M, N, K, ZB, ZH; float alpha; int act; int accumulate;
  const float* A2; int split_n;
  const float* B2; int split_m;
  float* C2;
  float* rowsum; int rowsum_acc;
  const uint64_t* rng;
  uint64_t a_drop_off, a_drop_n; float a_drop_p, a_drop_p2;
  uint64_t c_drop_off, c_drop_n; float c_drop_p, c_drop_p2;
  /* grouped form (the three sub-regions' couplers in one launch, z = group): per-z pointers override B / bias / C / rowsum
   * when the first entry is non-NULL (separate weight tensors per group; A, residual, C2 stay strided) */
  const float* B_tab[4]; const float* bias_tab[4]; float* C_tab[4]; float* rowsum_tab[4];
};
int cwf_gemm_ex(const struct cwf_gemm_args* args /* host */, void* stream);
/* Tests and tools: the route of the K-panel GEMM kernels (the whole contraction as straight-line code over compile-time panels, several
 * panels of 16-byte loads in flight; instantiated for the contraction lengths the training step launches).  cwf_debug_gemm_panel: 1 = the
 * product route (the shape classes measured faster there), 0 = never (the 16-byte-load kernel's result), 2 = every launch that has an
 * instantiation; returns the previous value.  cwf_debug_gemm_panel_launches: launches that took the route so far (host-side count).
 * Results do not depend on the route: every output is bit-identical. */
int cwf_debug_gemm_panel(int v);
long long cwf_debug_gemm_panel_launches(void);

/* The attention core of one coupler block in one launch each way (SelfAttention.py:94-98; K6):
 *   qkv [Z*T][ld] holds q | k | v side by side (columns [0,E) [E,2E) [2E,3E), head-major), T <= 144, E = heads*64
 *   o[z*T+t][h*64+d] = sum_key dropout(softmax_key(scale * q.k))[t][key] * v[key][d]
 *   backward recomputes the probabilities in LDS: dqkv (same layout as qkv) from d_o.  Attention dropout is keep(drop_off +
 *   ((z*heads+h)*T + t)*T + key) from the device generator state -- no mask tensor, no [Z,heads,T,T] probabilities in HBM. */
int cwf_attn_fwd(const float* qkv, int64_t ld, float* o, int64_t ldo, int Z, int T, int E, int heads, float scale,
                 const uint64_t* rng, uint64_t drop_off, float drop_p, void* stream);
int cwf_attn_bwd(const float* qkv, int64_t ld, const float* d_o, int64_t ldo, float* dqkv, int Z, int T, int E, int heads,
                 float scale, const uint64_t* rng, uint64_t drop_off, float drop_p, void* stream);
/* The same backward pass in two launches that fill the device: A, one workgroup per (query tile, sequence, head), runs scores, row
 * step and dQ and leaves the dropped probabilities and dS*scale in `ws`; B, one workgroup per (key tile, sequence, head), forms
 * dK / dV from them.  No sum and no order across workgroups: dqkv is bit-identical to cwf_attn_bwd's.  ws: caller-owned device
 * memory, 16-byte aligned, at least cwf_attn_bwd_ws_bytes(Z, T, heads) = 2 * Z*heads * ceil(T/32)*32 * 144 * 4 bytes; a null,
 * misaligned or too small workspace is CWF_E_BADARG and nothing is written.  cwf_debug_attn_split: 1 = two launches (default), 0 = the
 * one-launch kernel; cwf_debug_attn_split_waves: 4, 8 or 16 waves per workgroup of launch A (results do not depend on it); both
 * return the previous value.  cwf_debug_attn_split_launches: calls that took the two-launch route so far (host-side count). */
int64_t cwf_attn_bwd_ws_bytes(int Z, int T, int heads);
int cwf_attn_bwd_ws(const float* qkv, int64_t ld, const float* d_o, int64_t ldo, float* dqkv, int Z, int T, int E, int heads,
                    float scale, const uint64_t* rng, uint64_t drop_off, float drop_p, void* ws, int64_t ws_bytes, void* stream);
int cwf_debug_attn_split(int v);
int cwf_debug_attn_split_waves(int v);
long long cwf_debug_attn_split_launches(void);

/* Paired LayerNorm of a coupler block (PreNormDrop: norm(x), norm2(x2); ResidualNorm.py:23-32):
 *   ya = LN(x; g1,b1) ; yb[r] = LN(x2[perm(r)]; g2,b2) ; stats [2][rows][2] = (mean, rstd) ; x2 may be NULL (PreNorm of the FFN)
 *   perm_T > 0: the second operand is read with the two halves of every sequence pair swapped (rows = pairs * 2 * perm_T),
 *   which is how "a attends b, b attends a" (ClsWiseTransformer.py:47-50) runs as one batch.
 * backward (one launch for the inputs, one for the four parameter gradients, both deterministic, nothing pre-zeroed):
 *   dx2 != NULL:  dx = dy + LN1'(da) ; dx2 = LN2'(db)                    (perm_T == 0)
 *   dx2 == NULL:  dx[r] = dy[r] + LN1'(da[r]) + LN2'(db[perm(r)])        (x2 is x; db may be NULL -> single LayerNorm)
 *   dg*, db* (+)= per-column sums (accumulate_params: the weight-sharing sum over the uses of one block)                  */
int cwf_ln_pair_fwd(const float* x, const float* x2, int perm_T, const float* g1, const float* b1, const float* g2, const float* b2,
                    float* ya, float* yb, float* stats, int rows, int E, float eps, void* stream);
/* grouped forms: rows = groups * rows_per_group, group g uses the g-th LayerNorm parameter set (host arrays of `groups` <= 4 device
 * pointers; the parameter-gradient outputs likewise) -- the three sub-regions' couplers normalised in one launch */
struct cwf_ln_group_params { const float* g1[4]; const float* b1[4]; const float* g2[4]; const float* b2[4];
                             float* dg1[4]; float* db1[4]; float* dg2[4]; float* db2[4]; };
int cwf_ln_pair_fwd_g(const float* x, const float* x2, int perm_T, const struct cwf_ln_group_params* h_params, int groups,
                      float* ya, float* yb, float* stats, int rows, int E, float eps, void* stream);
int cwf_ln_pair_bwd_g(const float* dy, const float* da, const float* db, const float* x, const float* x2, int perm_T,
                      const struct cwf_ln_group_params* h_params, int groups, const float* stats, float* dx, float* dx2,
                      int rows, int E, int accumulate_params, void* stream);
int cwf_ln_pair_bwd(const float* dy, const float* da, const float* db, const float* x, const float* x2, int perm_T,
                    const float* g1, const float* g2, const float* stats, float* dx, float* dx2,
                    float* dg1, float* db1, float* dg2, float* db2, int rows, int E, int accumulate_params, void* stream);
/* dz = dh * keep(off + i) * gelu'(z)      backward of Dropout(GELU(z)), mask recomputed (p may be 0) */
int cwf_gelu_bwd_drop(const float* z, const float* dh, float* dz, int64_t n, const uint64_t* rng, uint64_t off, float p, void* stream);

/* rows x E LayerNorm (eps 1e-5): y = (x-mean)*rstd*gamma+beta; saves mean/rstd [rows] */
int cwf_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                      int rows, int E, float eps, void* stream);
/* dx (+= if accumulate); dgamma/dbeta are WRITTEN (deterministic column reduction, no zero-initialisation needed) */
int cwf_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                      float* dx, float* dgamma, float* dbeta, int rows, int E, int accumulate, void* stream);
/* in-place row softmax over `cols` (rows are contiguous, stride ld) and its backward dS = P*(dP - sum(dP*P)) */
int cwf_softmax_rows(float* s, int64_t rows, int cols, int ld, void* stream);
int cwf_softmax_rows_bwd(const float* p, float* dp_inout, int64_t rows, int cols, int ld, void* stream);
/* dx = dy * gelu'(x) */
int cwf_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* out[c] (+)= sum_rows x[row][c]   (bias gradients of the Linear layers) */
int cwf_colsum(const float* x, int64_t rows, int cols, int ld, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K4/K5  window <-> token reshapes, scoring, top-k, gather / scatter / gate
 *        cls_wise_former.py:15-39 (convert_dim/split_dim), :345-376 (selection), :457-543 (scatter + gate)
 * ---------------------------------------------------------------------------------------------- */
/* tok[b][ (d/p0,h/p1,w/p2) ][ ((c*p0+i)*p1+j)*p2+k ] = x[b][d][h][w][c]   (and the inverse) */
int cwf_window_to_tokens(const float* x, int x_ldc, float* tok, int B, int D, int H, int W, int C,
                         int p0, int p1, int p2, void* stream);
int cwf_tokens_to_window(const float* tok, float* x, int x_ldc, int B, int D, int H, int W, int C,
                         int p0, int p1, int p2, int accumulate, void* stream);
/* score[b][t] = dot(feats[b][t][:], query[b or 0][:])      token @ X^T, fp32 */
int cwf_token_scores(const float* feats, const float* query, int64_t query_bstride, float* score,
                     int B, int T, int E, void* stream);
/* indices of the k largest scores per sample, sorted descending (ties: lower index first)  -> int32 [B][k] */
int cwf_topk(const float* score, int32_t* index, int B, int T, int k, void* stream);
/* seq[b][0] = head[b or 0]; seq[b][1+j] = (feats[b][index[b][j]] + (e odd ? pe1 : 0)) * keep[b][j][e]
 * keep (nullable) is a pre-scaled dropout mask.  (:347-350; PositionalEncoding.py:20-22)   */
int cwf_gather_tokens(const float* feats, const int32_t* index, const float* head, int64_t head_bstride,
                      const float* keep, float pe_odd, float* seq, int B, int T, int k, int E, void* stream);
/* backward: dfeats[b][index[b][j]] += dseq[b][1+j]*keep ; dhead[e] += sum_b dseq[b][0][e] (both pre-zeroed or live) */
int cwf_gather_tokens_bwd(const float* dseq, const int32_t* index, const float* keep, float* dfeats, float* dhead,
                          int64_t dhead_bstride, int B, int T, int k, int E, void* stream);
/* out = feats with rows index[b][j] replaced by rows[b][j] (row stride rows_ld, batch stride rows_bs);
 * optional gate: out[b][t][e] *= gate[b][e]  (gate batch stride gate_bs)                   (:467,481) */
int cwf_scatter_rows(const float* feats, const int32_t* index, const float* rows, int64_t rows_ld, int64_t rows_bs,
                     const float* gate, int64_t gate_bs, float* out, int B, int T, int k, int E, void* stream);
/* backward of scatter (+gate): given dout, pre-gate values `scat` (= scatter result before gating; may be NULL if no gate):
 *   dgate[b][e] = sum_t dout*scat ; g = dout*gate ; dfeats = g with selected rows zeroed (+= if accumulate) ;
 *   drows[b][j] = g[b][index[b][j]]                                                                    */
int cwf_scatter_rows_bwd(const float* dout, const int32_t* index, const float* scat, const float* gate, int64_t gate_bs,
                         float* dfeats, int accumulate, float* drows, int64_t drows_ld, int64_t drows_bs,
                         float* dgate, int64_t dgate_bs, int B, int T, int k, int E, void* stream);

/* ---- round-2 forms: one launch per stage of a sub-region's selection / scatter, gradients written (not accumulated) ------- */
/* s1[b][t] = feats[b][t].q1[b or 0], s2 likewise for q2 (nullable): both class tokens of a region against one token matrix */
int cwf_token_scores2(const float* feats, const float* q1, int64_t q1_bstride, const float* q2, int64_t q2_bstride,
                      float* s1, float* s2, int B, int T, int E, void* stream);
/* grouped: sample b belongs to group b / group_B and is scored against that group's shared queries (host arrays of pointers) */
int cwf_token_scores2_g(const float* feats, const float* const* h_q1, const float* const* h_q2, int groups, int group_B,
                        float* s1, float* s2, int B, int T, int E, void* stream);
/* top-k of one or two score vectors [B][T] (same T, k) in one launch; inv*[b][t] = rank of token t if selected else -1 (nullable);
 * NaN scores order as the largest value (torch.topk) */
int cwf_topk_inv(const float* score0, int32_t* index0, int32_t* inv0, const float* score1, int32_t* index1, int32_t* inv1,
                 int B, int T, int k, void* stream);
/* inverse map of a given index set (teacher-forced selections in tests) */
int cwf_index_inv(const int32_t* index, int32_t* inv, int B, int T, int k, void* stream);
/* up to four gathers in one launch: out[b][0] = head[b or 0] ; out[b][1+j] = (feats[b][index[b][j]] + pe) * keep
 * (the four 129-token sequences of a region written straight into the paired [B][2][129][E] operands; :345-376) */
struct cwf_gather_job { const float* feats; const int32_t* index; const float* head; float* out;
                        int64_t head_bstride, out_bstride; int T; uint64_t drop_off;
                        const float* head_g[4]; int group_B; /* group_B > 0: sample b takes head_g[b / group_B] (shared per group) */ };
int cwf_gather_multi(const struct cwf_gather_job* jobs /* host */, int njobs, int B, int k, int E, float pe_odd,
                     const uint64_t* rng, float p, void* stream);
/* scat = feats with the selected rows replaced (via inv) ; gated = scat * gate ; either output may be NULL      (:463-485) */
int cwf_scatter_inv(const float* feats, const int32_t* inv, const float* rows, int64_t rows_ld, int64_t rows_bs,
                    const float* gate, int64_t gate_bs, float* gated, float* scat, int B, int T, int E, void* stream);
/* backward of the above into the producer of (rows, gate): drows[b][j] = dgated[b][index[j]]*gate + dscat[b][index[j]] ;
 * dgate[b] = sum_t dgated*scat + dgate_extra[b]   (scat re-derived from feats / inv / rows; written, deterministic) */
int cwf_scatter_bwd(const float* dgated, const float* dscat, const float* feats, const int32_t* inv, const int32_t* index,
                    const float* rows, int64_t rows_ld, int64_t rows_bs, const float* gate, int64_t gate_bs,
                    const float* dgate_extra, int64_t extra_bs, float* drows, int64_t drows_ld, int64_t drows_bs,
                    float* dgate, int64_t dgate_bs, int B, int T, int k, int E, void* stream);
/* cwf_debug_scatter_bwd: 1 = the product route (default), 0 = scatter_bwd_kernel (64 columns per workgroup), 8 / 16 / 32 = the narrow-block
 * kernel at that many columns per workgroup; returns the previous value.  Every route sums dgate in the same chains: bit-identical.
 * (The narrow-block kernel reads 8 / 16 bytes per access: a launch whose dgated, feats or rows is not 16-byte aligned takes route 0.) */
int cwf_debug_scatter_bwd(int v);
/* gradient of a token matrix from its three uses in one pass (written): scatter pass-through of the non-selected rows
 * (dgated*gate + dscat) + adjoint of the primary gather (inv_p, dseq_p) + adjoint of the supplementary gather (inv_q, dseq_q) */
int cwf_token_grad(const float* dgated, const float* dscat, const float* gate, int64_t gate_bs,
                   const int32_t* inv_p, const int32_t* inv_q, const float* dseq_p, int64_t dseq_p_bs,
                   const float* dseq_q, int64_t dseq_q_bs, const uint64_t* rng, uint64_t drop_off_p, uint64_t drop_off_q, float p,
                   float* dfeats, int B, int T, int k, int E, void* stream);
/* class-token gradients: out1 = sum_b (a1[b] + c1[b]), out2 = sum_b (a2[b] + c2[b]) over rows of stride bstride */
int cwf_head_grad(const float* a1, const float* c1, const float* a2, const float* c2, int64_t bstride,
                  float* out1, float* out2, int B, int E, void* stream);
/* grouped: group g sums its samples [g*group_B, (g+1)*group_B) into h_out1[g] / h_out2[g] */
int cwf_head_grad_g(const float* a1, const float* c1, const float* a2, const float* c2, int64_t bstride,
                    float* const* h_out1, float* const* h_out2, int groups, int group_B, int E, void* stream);
/* window <-> token reshapes of `groups` channel groups of one NDHWC tensor in one launch:
 *   tok[g][b][t][f] = x[b][voxel][g*C + c]   and the inverse (x_ldc >= groups*C) */
int cwf_window_to_tokens_g(const float* x, int x_ldc, float* tok, int groups, int B, int D, int H, int W, int C,
                           int p0, int p1, int p2, void* stream);
int cwf_tokens_to_window_g(const float* tok, float* x, int x_ldc, int groups, int B, int D, int H, int W, int C,
                           int p0, int p1, int p2, void* stream);
/* y[v][g*C + c] = xs[g][v][c] (NULL source: zeros), g < 3: the adjoint of slicing one tensor into three channel groups */
int cwf_cat3_channels(const float* x0, const float* x1, const float* x2, float* y, int64_t nvox, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K8/K10  heads: trilinear upsample (align_corners=False) + channel softmax; 4-class channel softmax
 *         SuperviseLabel.py:62-64, EdgeSuperviseLabel.py:58-60, cls_wise_former.py:662-664
 * ---------------------------------------------------------------------------------------------- */
/* prob[n][D*s][H*s][W*s][C] = softmax_c( trilinear_up(logit[n][D][H][W][C (ldc)]) ), C in {2,4} */
int cwf_upsample_softmax(const float* logit, int l_ldc, float* prob, int N, int D, int H, int W, int C, int scale,
                         void* stream);
/* dlogit (low res) from dprob and prob (high res); workspace: N * D*scale * H * W * C floats (separable two-pass adjoint,
 * deterministic); writes only channels [0, C) of dlogit */
int cwf_upsample_softmax_bwd(const float* dprob, const float* prob, float* dlogit, int dl_ldc,
                             int N, int D, int H, int W, int C, int scale, float* workspace, void* stream);
/* prob = softmax over C contiguous channels per voxel; dlogit = p*(dp - sum p*dp) */
int cwf_channel_softmax(const float* logit, int l_ldc, float* prob, int64_t nvox, int C, void* stream);
int cwf_channel_softmax_bwd(const float* dprob, const float* prob, float* dlogit, int dl_ldc, int64_t nvox, int C,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * K9  fused Dice + weighted cross-entropy   utils/tools.py:8-34,112-231; models/criterions.py:49-62
 *   prob  [N][V][C] channels-last, C in {2,4};  label int64 [N][V]
 *   C==4: class = label (0..3).   C==2: class = (posmask >> label) & 1  (label in 0..15)
 *   sums double [N][C][4] += (sum p*t, sum p, sum t, sum t*log(clamp(p,0.005,1)))   (zeroed by caller)
 *   cwf_dice_ce_finalize -> loss[0] = dice + ce ; coef float [N][C][4] for the backward
 *   cwf_dice_ce_bwd: dprob = gscale[0] * dLoss/dprob
 * ---------------------------------------------------------------------------------------------- */
int cwf_dice_ce_sums(const float* prob, const int64_t* label, uint32_t posmask, double* sums,
                     int N, int64_t V, int C, void* stream);
int cwf_dice_ce_finalize(const double* sums, float* loss, float* coef, int N, int64_t V, int C, void* stream);
/* nmaps problems back to back (sums [nmaps][N][C][4], loss [nmaps], coef [nmaps][N][C][4]); total[0] = sum of the losses (nullable) */
int cwf_dice_ce_finalize_multi(const double* sums, float* loss, float* coef, float* total, int nmaps, int N, int64_t V, int C, void* stream);
/* Fused head -> loss (training mode): the sums above for up to three sub-region maps of one supervision call straight from their
 * LOW-resolution 2-channel logits [N][D][H][W][l_ldc] -- trilinear x scale (align_corners=False) + softmax evaluated in registers,
 * one shared read of the label volume, nothing written at full resolution (SuperviseLabel.py:58-81 -> tools.py:112-231).
 * h_logits / h_posmasks / h_dlogits are HOST arrays of nmaps entries.  Backward: dlogits[m] [N][D][H][W][dl_ldc] WRITTEN (channels
 * >= 2 zeroed) from (label, coef, gscale); workspace: nmaps * N * D*scale * H * W * 2 floats.                                      */
int cwf_head_loss_sums(const float* const* h_logits, int nmaps, int l_ldc, const uint32_t* h_posmasks, const int64_t* label,
                       double* sums, int N, int D, int H, int W, int scale, void* stream);
int cwf_head_loss_bwd(const float* const* h_logits, int nmaps, int l_ldc, const uint32_t* h_posmasks, const int64_t* label,
                      const float* coef, const float* gscale, float* const* h_dlogits, int dl_ldc, float* workspace,
                      int N, int D, int H, int W, int scale, void* stream);
/* Same, the maps being channel groups of ONE gradient buffer: dl_ca channels written per voxel (2 gradients + zeroed padding), voxel
 * rows dl_ldc floats apart (what the channel-grouped head convs below consume). */
int cwf_head_loss_bwd_ex(const float* const* h_logits, int nmaps, int l_ldc, const uint32_t* h_posmasks, const int64_t* label,
                         const float* coef, const float* gscale, float* const* h_dlogits, int dl_ca, int dl_ldc, float* workspace,
                         int N, int D, int H, int W, int scale, void* stream);
int cwf_dice_ce_bwd(const float* prob, const int64_t* label, uint32_t posmask, const float* coef, const float* gscale,
                    float* dprob, int N, int64_t V, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L2  boundary loss (Kervadec et al., MIDL 2019): dense exact signed distance maps of label maps + fused loss (csrc/boundary.hip)
 *   label int64 [B][D0][D1][D2]; region r = class bitmask posmasks[r] (host memory, R values, copied into the launches): a voxel is in
 *   G_r iff 0 <= label < 32 and (posmasks[r] >> label) & 1.  1 <= R <= 8, 1 <= D_d <= 512.
 *   phi float [B][R][D0][D1][D2]: with q the exact integer squared Euclidean distance (unit spacing) to the nearest voxel of the other
 *   side of G_r inside the volume, float32(sqrt((double)q)) outside G_r and float32(1.0 - sqrt((double)q)) inside; +0 throughout a
 *   (sample, region) whose G_r is empty or fills the volume.  Exact: bit-equal to the float64 statement.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of device workspace cwf_signed_distance needs (6 bytes per voxel, sample and region, 256-B aligned), or a negative CWF_E_*:
 * CWF_E_BADARG for B <= 0, R outside 1..8 or an extent outside 1..512; CWF_E_TOOLARGE for more than 2^31 - 1 workgroups. */
int64_t cwf_signed_distance_workspace(int B, int R, int D0, int D1, int D2);
/* Three launches, no host synchronisation, nothing read back, no kernel waits on another workgroup: capturable.  ws is fully rewritten
 * (nothing needs zeroing).  CWF_E_BADARG as above and for a null pointer, before any launch; CWF_E_ALIGN: ws off 256 bytes. */
int cwf_signed_distance(const int64_t* label, const uint32_t* posmasks, float* phi, int B, int R, int D0, int D1, int D2, void* ws,
                        void* stream);
/* prob float [N][V][C] channels-last, 1 <= C <= 32; p_r = float32 sum of prob[..][c] over the classes c < C of region r, increasing c.
 * sum[0] (double, zeroed by the caller) += sum over n, r, v of (double)phi_r * (double)p_r. */
int cwf_boundary_sums(const float* prob, const float* phi, const uint32_t* posmasks, double* sum, int N, int R, int64_t V, int C,
                      void* stream);
/* weight: one float in DEVICE memory.  loss[0] = float32((double)w / (N R V) * sum[0]);  coef[0] = k = float32((double)w / (N R V)). */
int cwf_boundary_finalize(const double* sum, const float* weight, float* loss, float* coef, int N, int R, int64_t V, void* stream);
/* dprob[n][v][c] = (gscale[0] * coef[0]) * s_c, s_c = float32 sum of phi_r over the regions r holding class c, increasing r, every
 * product rounded on its own; +0 for a class in no region.  dprob is fully written. */
int cwf_boundary_bwd(const float* phi, const uint32_t* posmasks, const float* coef, const float* gscale, float* dprob, int N, int R,
                     int64_t V, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L3  top-k (hard-voxel) cross-entropy with an exact on-device selection (csrc/topk.hip; this project's statement)
 *   prob float [N][V][C] channels-last, C = 4 or 2; label int64 [N][V]; target class t = label (C = 4, labels 0..3) or
 *   (posmask >> (label & 31)) & 1 (C = 2), as in cwf_dice_ce_*.  M = N V; the selection runs over the whole batch.
 *   pc = (p_t > 0) ? fminf(p_t, 1.0f) : 0.0f (NaN, negatives, -0 -> +0);  key = bits(pc) as uint32 (key order = value order);
 *   l = -logf(fmaxf(pc, 1e-7f));  tau = the k-th smallest key;  a = #{key < tau}, n = #{key = tau}, s = k - a.
 *   loss[0] = float32((double)w / k * (sum_{key < tau} (double)l + (double)s * (double)l(tau))), w = weight[0] in DEVICE memory.
 *   coef[0] = float32((double)w / k), coef[1] = float32((double)s / (double)n), coef[2] = bits of tau, coef[3] = +0.
 *   tau, s, n are exact and the loss repeats bit for bit from run to run (integer histograms, partials added in a fixed order).
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of device workspace cwf_topk_ce needs (4 bytes per voxel + 49,408, 256-B aligned), or a negative CWF_E_*: CWF_E_BADARG for
 * N <= 0 or V <= 0, CWF_E_TOOLARGE for more than 2^40 voxels. */
int64_t cwf_topk_ce_workspace(int N, int64_t V);
/* Nine launches, no host synchronisation, nothing read back, no kernel waits on another workgroup, no memcpy: capturable.  ws may
 * hold anything (what needs zeroing is zeroed by a kernel).  CWF_E_BADARG before any launch: a null pointer, C not 2 or 4, N <= 0,
 * V <= 0, k < 1 or k > N V; CWF_E_ALIGN: ws off 256 bytes. */
int cwf_topk_ce(const float* prob, const int64_t* label, uint32_t posmask, int64_t k, const float* weight, float* loss, float* coef,
                int N, int64_t V, int C, void* ws, void* stream);
/* One streaming launch.  g0 = gscale[0] * coef[0], r = -1.0f / fmaxf(pc, 1e-7f), every product rounded on its own:
 * dprob[v][t] = g0 * r for key < tau, (g0 * coef[1]) * r for key = tau (ties share the remaining weight equally), +0 for key > tau
 * and for every other class; dprob is fully written.  The gradient passes through the 1e-7 floor as -1 / 1e-7. */
int cwf_topk_ce_bwd(const float* prob, const int64_t* label, uint32_t posmask, const float* coef, const float* gscale, float* dprob,
                    int N, int64_t V, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L4  focal Tversky on class-bitmask regions + focal cross-entropy (csrc/focal.hip; this project's statement)
 *   prob float [N][V][4] channels-last; label int64 [N][V], class y = label & 3.  M = N V; every sum runs over the whole batch.
 *   regions r < R (0 <= R <= 8): class bitmasks posmasks[r] over bits 0..3, in HOST memory.  t_r = (m_r >> y) & 1;
 *   p_r = 0.0f + the p_c of the classes of m_r in ascending class order (float32).
 *   TP_r = sum t_r p_r, SP_r = sum p_r, ST_r = sum t_r (float64);  FN = ST - TP, FP = SP - TP, num = TP + smooth,
 *   den = ((TP + fn FN) + fp FP) + smooth, x = 1 - num / den;  FT = (1 / R) sum_r (x > 0 ? x pow(x, exponent - 1) : 0).
 *   q = fminf(fmaxf(p_y, 1e-7f), 1.0f);  SF = sum (double)k_y ((double)(1.0f - q)^gamma (double)(-logf(q))): the power by
 *   multiplication for gamma = 0, 1, 2, 3 and by powf otherwise; gamma and k = class_weight are rounded to float32 once.
 *   loss[0] = float32(w (FT + ce_ratio SF / M)), w = weight[0] in DEVICE memory.  R = 0: FT = 0 (focal cross-entropy alone);
 *   ce_ratio = 0: Tversky alone, no logarithm or power is evaluated.
 *   coef float [2 R + 1]: [2 r] = w K_r A_r and [2 r + 1] = w K_r B_r, the multipliers of t_r and of 1 in d loss / d p_r, with
 *   K_r = -(exponent / R) x^(exponent - 1), A_r = (den - num ((1 - fn) - fp)) / den^2, B_r = -(num fp) / den^2, both +0 where
 *   x <= 0;  [2 R] = w ce_ratio / M.
 *   No floating-point atomics: per-workgroup partials, added in workgroup-index order; the result repeats bit for bit.
 * ---------------------------------------------------------------------------------------------- */
struct cwf_focal_params {
  double fn, fp;          /* weights of the false negatives and the false positives: finite, >= 0, fn + fp > 0 */
  double exponent;        /* 0 < exponent <= 4 */
  double smooth;          /* finite, > 0 */
  double gamma;           /* 0, or 1 <= gamma <= 5 (a gamma in (0, 1) gives 0 * inf at p = 1) */
  double ce_ratio;        /* finite, >= 0; 0 needs R >= 1 and R = 0 needs ce_ratio > 0 */
  double class_weight[4]; /* finite, >= 0 */
};
/* Bytes of device workspace cwf_focal_loss needs (1024 rows of 3 R + 1 doubles, 256-B aligned), or a negative CWF_E_*:
 * CWF_E_BADARG for N <= 0, V <= 0 or R outside 0..8, CWF_E_TOOLARGE for more than 2^40 voxels. */
int64_t cwf_focal_workspace(int N, int64_t V, int R);
/* Two launches, no host synchronisation, no allocation, nothing read back, no kernel waits on another workgroup: capturable.  ws may
 * hold anything.  Before any launch: CWF_E_BADARG for a null pointer (posmasks may be null when R = 0), C != 4, N <= 0, V <= 0,
 * R outside 0..8, a zero mask or one with bits above 3, a parameter outside the ranges above; CWF_E_ALIGN for ws off 256 bytes,
 * prob off 16, label off 8. */
int cwf_focal_loss(const float* prob, const int64_t* label, const uint32_t* posmasks, int R, const struct cwf_focal_params* params,
                   const float* weight, float* loss, float* coef, int N, int64_t V, int C, void* ws, void* stream);
/* One streaming launch, one 16-byte store per voxel, dprob fully written; float32, every operation rounded on its own:
 *   u_r = t_r ? coef[2 r] + coef[2 r + 1] : coef[2 r + 1];  d_c = 0.0f + the u_r of the regions holding class c, ascending r;
 *   where c = y and 1e-7 <= p_y <= 1 (torch's clamp rule), with om = 1.0f - p_y and l = logf(p_y):
 *     h = -1 / p_y | l - om / p_y | (2 om) l - (om om) / p_y | (3 (om om)) l - ((om om) om) / p_y
 *         | (gamma powf(om, gamma - 1)) l - powf(om, gamma) / p_y          for gamma = 0 | 1 | 2 | 3 | otherwise
 *     d_y += coef[2 R] (k_y h);
 *   dprob[v][c] = gscale[0] d_c.  With ce_ratio = 0 prob is not read.  Errors as cwf_focal_loss (dprob off 16 bytes: CWF_E_ALIGN). */
int cwf_focal_loss_bwd(const float* prob, const int64_t* label, const uint32_t* posmasks, int R, const struct cwf_focal_params* params,
                       const float* coef, const float* gscale, float* dprob, int N, int64_t V, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L5  Lovasz-Softmax on class-bitmask regions, by an exact device-wide sort (csrc/lovasz.hip; this project's statement)
 *   prob float [N][V][4] channels-last; label int64 [N][V], class y = label & 3.  M = N V; the sort runs over the whole batch.
 *   regions r < R (1 <= R <= 8): class bitmasks posmasks[r] in 1..15, in HOST memory.  Per region and voxel:
 *   fg = (m_r >> y) & 1;  q = the p_c of the classes of m_r added in ascending class order (float32; one class: q = p_c);
 *   qc = (q > 0) ? fminf(q, 1.0f) : 0.0f;  e = fg ? 1.0f - qc : qc;  sgn = (e > 0) ? (fg ? -1 : +1) : 0.
 *   G = #{fg}.  Group j = the m_j voxels (f_j of them foreground) sharing the j-th largest distinct e; n_j, F_j the running sums.
 *   J(n, F) = n ? 1.0 - (double)(G - F) / (double)(G + n - F) : 0.0;  dJ_j = J(n_j, F_j) - J(n_{j-1}, F_{j-1});  L_r = sum_j (double)e_j dJ_j.
 *   A region is counted if G_r > 0, or always with only_present = 0; P = the number counted.
 *   loss[0] = float32((double)w / max(P, 1) * sum_counted L_r), w = weight[0] in DEVICE memory (+0 for P = 0).
 *   coef float [4]: [0] = float32((double)w / P) (+0 for P = 0), [1] = (float)P, [2] = [3] = +0.
 *   vcoef float [R][M]: float32(dJ_j / (double)m_j) * (float)sgn -- ties share their group's increment equally, so neither voxel order
 *   nor launch geometry enters; 0 in a region that is not counted.
 *   No floating-point atomics, no workgroup waits on another; loss, coef and vcoef repeat bit for bit.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of device workspace cwf_lovasz needs (two key arrays of 4 bytes per voxel and region, the per-tile digit counts, 73,728
 * bytes of totals and partials, a search tree of about 4 / 15 bytes per voxel and region; 256-B aligned), or a negative CWF_E_*: CWF_E_BADARG for N <= 0, V <= 0 or R outside 1..8,
 * CWF_E_TOOLARGE for more than 2^31 - 1 voxels (positions in the sorted arrays are 32-bit). */
int64_t cwf_lovasz_workspace(int N, int64_t V, int R);
/* Fifteen launches, no host synchronisation, no allocation, nothing read back: capturable.  ws may hold anything.  Before any
 * launch: CWF_E_BADARG for a null pointer, N <= 0, V <= 0, R outside 1..8, a mask outside 1..15; CWF_E_TOOLARGE as above;
 * CWF_E_ALIGN for ws off 256 bytes, prob off 16, label off 8. */
int cwf_lovasz(const float* prob, const int64_t* label, const uint32_t* posmasks, int R, int only_present, const float* weight,
               float* loss, float* coef, float* vcoef, int N, int64_t V, void* ws, void* stream);
/* One streaming launch, one 16-byte store per voxel, dprob [N][V][4] fully written; float32, every operation rounded on its own:
 * g0 = gscale[0] * coef[0];  dprob[v][c] = 0.0f + the (g0 * vcoef[r][v]) of the regions holding class c, ascending r.
 * Errors as cwf_lovasz (dprob off 16 bytes: CWF_E_ALIGN). */
int cwf_lovasz_bwd(const float* vcoef, const uint32_t* posmasks, int R, const float* coef, const float* gscale, float* dprob,
                   int N, int64_t V, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N1  sliding-window inference glue   predict_overlap.py:31-58 (tailor_and_concat), :134-141 + utils/tools.py:44-47,64-109
 *     and utils/hausdorff.py (Hausdorff distance / HD95)
 * ---------------------------------------------------------------------------------------------- */
/* y [B][4][240][240][155] (NCDHW) <- the eight 128^3 window outputs windows[(w*B + b)][128][128][128][4] (channels-last, the model's
 * own output memory), w in the reference's window order; hard overwrite by the later window incl. the reference's last-axis offset
 * quirk (voxels 123..149 of the second depth window land at 128..154).  Replaces x.clone() + eight slice assignments.              */
int cwf_stitch_windows(const float* windows, float* y, int B, void* stream);
/* seg[b][v] = argmax over the 4 classes of prob[b*sb + c*sc + v*sv] (first maximum in torch.argmax's order: a NaN is the maximum
 * and the first NaN wins, -0 == +0); with a target (int64 labels of any value, the rules applied to the whole 64 bits: WT is > 0, TC is
 * == 1 or == 3, ET is == 3, so a label outside 0..3 is whole tumour if positive and nothing else) also the
 * counts[k][3] += (|o & t|, |o|, |t|) of tools.softmax_output_dice's three regions k = WT, TC, ET (uint64, zeroed by the caller).
 * target may be NULL, and counts with it.  CWF_E_BADARG before any launch: a null prob or seg, B <= 0, V <= 0, a target without counts. */
int cwf_argmax_dice(const float* prob, int64_t sb, int64_t sc, int64_t sv, const int64_t* target, int64_t* seg, uint64_t* counts,
                    int B, int64_t V, void* stream);
/* the same plus the per-class counts of tools.softmax_mIOU_score (utils/tools.py:50-61, reported by predict_simple.py): counts[6][3] =
 * WT, TC, ET, class 1, class 2, class 3, each (|o & t|, |o|, |t|); IoU = |o & t| / (|o| + |t| - |o & t|).  target is required.      */
int cwf_argmax_metrics(const float* prob, int64_t sb, int64_t sc, int64_t sv, const int64_t* target, int64_t* seg, uint64_t* counts,
                       int B, int64_t V, void* stream);
/* Hausdorff metrics (medpy.metric.binary hd / hd95 as called by the reference's utils/hausdorff.py and tools.softmax_hd_dice).
 * Masks are bytes of region bits: bit r set = the voxel belongs to region r (R <= 8 regions per call).
 * bits[i] <- region bits of int64 labels[i] for tools.softmax_output_dice's regions: bit 0 WT (> 0), bit 1 TC (1 or 3), bit 2 ET (3). */
int cwf_region_bits(const int64_t* labels, uint8_t* bits, int64_t n, void* stream);
/* Bytes of device workspace cwf_hausdorff needs for B samples x R regions of D0 x D1 x D2 voxels (256-B aligned; about 32 bytes
 * per voxel plus 2 bytes per voxel and sample), or a negative CWF_E_* (CWF_E_TOOLARGE: D2 > 4096 or 2^31 voxels or more). */
int64_t cwf_hausdorff_workspace(int B, int R, int D0, int D1, int D2);
/* For every sample b and region r of the masks a, b [B][D0][D1][D2] (region bits): the borders dA, dB (mask & ~erosion under the
 * connectivity 1/2/3 footprint of 6/18/26 neighbours, out-of-volume unset; all_border != 0: border = mask, medpy's result for
 * [1, D0, D1, D2] arrays), the exact float64 Euclidean distances (spacing s0, s1, s2 along axes 0, 1, 2) from each voxel of dA to the
 * nearest of dB and from dB to dA, and
 *   hd[b][r]    max of both directions (medpy hd)
 *   hd95[b][r]  numpy's linear 95th percentile of the union of both directions (medpy hd95); NaN in both when a mask is empty
 *   counts[b][r][4] = |A|, |B|, |dA|, |dB|  (zeroed here).
 * ws: cwf_hausdorff_workspace(...) bytes, 256-B aligned.  Only the [B][R] results are written outside the workspace.            */
int cwf_hausdorff(const uint8_t* a, const uint8_t* b, int B, int R, int D0, int D1, int D2, double s0, double s1, double s2,
                  int connectivity, int all_border, double* hd, double* hd95, int64_t* counts, void* ws, int64_t ws_bytes,
                  void* stream);
/* N8  normalised surface Dice (NSD) and average surface distance on the borders and distances of cwf_hausdorff (same arguments, same
 * kernels; hd, hd95 and counts are bit-equal to that function's).  With q the float64 squared distance of the transform and
 * d(p) = sqrt(q), correctly rounded, for p in dA (to the nearest voxel of dB) and for p in dB (to dA), and tolerances tau[0..T):
 *   within[b][r][t][2]  int64: |{p in dA : d(p) <= tau[t]}|, the same over dB (a float64 <= on d)
 *   nsd[b][r][t]        (within[t][0] + within[t][1]) / (|dA| + |dB|): one float64 division of two integers converted exactly
 *   asd[b][r][2]        mean of d over dA, mean of d over dB (medpy asd(A, B), asd(B, A))
 *   assd[b][r]          (asd[0] + asd[1]) / 2 (medpy assd)
 * If either mask is empty every float output of that (b, r) is NaN and within is 0.  This is the voxel-border NSD (MONAI's
 * compute_surface_dice without sub-voxel handling), not the area-weighted surface-element form of DeepMind's surface-distance; with unit
 * spacing every tau < 1 counts coincident border voxels only.  within and nsd are exact.  asd is a float64 sum whose every addition has
 * fixed operands (per-line slots, then a fixed tree: csrc/metrics.hip), so it is bit-identical from run to run and does not depend on
 * B, R or the order in which atomics land; it lies within 2 n 2^-53 relative of the exact mean of the rounded d (n = border voxels).
 * tau: T values in host memory, copied into the launches; 0 <= T <= 4 (with T == 0 tau, within and nsd may be null).
 * ws: cwf_surface_metrics_workspace(...) bytes (cwf_hausdorff's plus 48 bytes per axis-(0, 1) line), 256-B aligned.  No host
 * synchronisation, no kernel waits on another workgroup: the call can be captured into a graph.
 * CWF_E_BADARG: T outside 0..4, a negative or NaN tau (+inf is allowed and counts every border voxel), a null pointer; otherwise as
 * cwf_hausdorff. */
int64_t cwf_surface_metrics_workspace(int B, int R, int D0, int D1, int D2);
int cwf_surface_metrics(const uint8_t* a, const uint8_t* b, int B, int R, int D0, int D1, int D2, double s0, double s1, double s2,
                        int connectivity, int all_border, const double* tau, int T, double* hd, double* hd95, double* asd, double* assd,
                        int64_t* within, double* nsd, int64_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N6  connected-component post-processing of predicted label maps (predict_overlap.postprocess): 3-D connected-component labelling
 *     of region-bit masks by block-based union-find, and the removal / relabelling policy on top of it.  All integer, exact.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of device workspace cwf_components needs (256-B aligned; about 4 bytes per voxel, sample and region), or a negative
 * CWF_E_*: CWF_E_BADARG for B, R or an extent <= 0 or R > 8, CWF_E_TOOLARGE for 2^31 voxels or more or B * R > 65535. */
int64_t cwf_components_workspace(int B, int R, int D0, int D1, int D2);
/* For every sample b and region r < R of bits [B][D0][D1][D2] (region bits, as cwf_region_bits writes them), V = D0 D1 D2:
 *   labels[b][r][V]   int32: 0 = background; components under the 6/18/26-neighbour footprint (connectivity 1/2/3) numbered 1..K
 *                     in increasing order of their smallest linear (C-order) voxel index -- scipy.ndimage.label's numbering
 *   sizes[b][r][cap]  cap = (V + 1) / 2: entry k - 1 = voxels of component k, entries >= K are 0
 *   count[b][r]       K
 *   largest[b][r][2]  (label, size) of the largest component, ties to the lowest label; (0, 0) for an empty mask.
 * The result does not depend on launch geometry or on the order in which atomics land.  ws: cwf_components_workspace(...) bytes,
 * 256-B aligned.  No kernel waits on another workgroup. */
int cwf_components(const uint8_t* bits, int B, int R, int D0, int D1, int D2, int connectivity, int32_t* labels, int32_t* sizes,
                   int32_t* count, int32_t* largest, void* ws, int64_t ws_bytes, void* stream);
/* seg_out[b][V] <- seg_in[b][V] (int64 classes 0..3; may be the same memory) under the policy below, from cwf_components' labels,
 * sizes and largest of R regions over the region bits of seg_in (wt_region: the region `seg > 0`, et_region: the region `seg == 3`).
 * Applied in this order, each rule off at 0:
 *   1  every WT component of fewer than min_component voxels is set to 0
 *   2  keep_largest: only the largest WT component that survived rule 1 is kept (ties: lowest label), every other voxel set to 0
 *   3  every ET component of fewer than et_min_component voxels is relabelled et_replace (0, 1 or 2)
 *   4  if fewer than et_min_voxels ET voxels remain after rules 1-3, all of them are relabelled et_replace
 * stats[b][4] (int64) = WT voxels removed, WT components removed, ET voxels relabelled (rules 3 and 4), ET voxels remaining.
 * ws: CWF_POSTPROCESS_WS_BYTES(B) bytes, 8-B aligned.  Two launches, the ET count of rule 4 is reduced on the device between them;
 * nothing is read back.  CWF_E_BADARG: a null pointer, a region index outside [0, R), a negative threshold, et_replace outside 0..2. */
#define CWF_POSTPROCESS_WS_BYTES(B) ((int64_t)(B) * 32)
int cwf_postprocess_labels(const int64_t* seg_in, int64_t* seg_out, const int32_t* labels, const int32_t* sizes, const int32_t* largest,
                           int B, int R, int D0, int D1, int D2, int wt_region, int et_region, int min_component, int keep_largest,
                           int et_min_component, int et_min_voxels, int et_replace, int64_t* stats, void* ws, void* stream);
/* counts[6][3] (uint64, accumulated: zero it first) += (|o & t|, |o|, |t|) of WT, TC, ET, class 1, class 2, class 3 of the int64 label
 * maps seg and target of n voxels: the counts of cwf_argmax_metrics for a label map that is already there. */
int cwf_label_metrics(const int64_t* seg, const int64_t* target, uint64_t* counts, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N7  lesion-wise Dice and HD95 (the BraTS 2023 ranking metrics; predict_overlap.lesionwise_metrics states the definition):
 *     binary dilation of region bits, and the per-lesion matching, counts, surface distances and aggregate built on
 *     cwf_components and cwf_hausdorff.  All integer up to the per-lesion ratios; the aggregate is float64.
 * ---------------------------------------------------------------------------------------------- */
/* out[B][D0][D1][D2] <- bits dilated `iterations` (0..8) times with the 6/18/26-neighbour footprint (connectivity 1/2/3), every bit
 * of the byte on its own and out-of-volume voxels unset: scipy.ndimage.binary_dilation(..., iterations) per bit.  0 iterations copy.
 * bits and out are distinct buffers.  ws: B * D0 * D1 * D2 bytes, distinct from both, needed from 2 iterations on (else may be
 * null).  CWF_E_BADARG: a null or aliased pointer, B or an extent <= 0, B > 65535, connectivity or iterations out of range;
 * CWF_E_TOOLARGE: 2^31 voxels or more, or ws_bytes too small. */
int cwf_dilate_bits(const uint8_t* bits, uint8_t* out, int B, int D0, int D1, int D2, int connectivity, int iterations, void* ws,
                    int64_t ws_bytes, void* stream);
/* Bytes of device workspace cwf_lesionwise needs (256-B aligned; about 4 bytes per voxel and sample plus 14 per voxel, sample and
 * region, plus the larger of the cwf_components (B, R) and cwf_hausdorff (B, 8) workspaces), or a negative CWF_E_* as those two
 * give it. */
int64_t cwf_lesionwise_workspace(int B, int R, int D0, int D1, int D2);
#define CWF_LESIONWISE_MAX 64
/* For every sample b and region r < R <= 8 of the region bits pred, gt [B][D0][D1][D2]:
 *   pred_cc = 26-neighbour components of pred, 1..P;  dil_cc = 26-neighbour components of gt dilated `dilation` (0..8) times with the
 *   18-neighbour footprint, 1..G;  lesion g = gt & (dil_cc == g);  component p touches lesion g if a voxel has pred_cc == p and
 *   dil_cc == g;  pred_g = the union of the components touching g.  Per lesion: gt_vol, pred_vol = |pred_g|, inter = |pred_g & lesion g|,
 *   dice_g = 2 inter / (pred_vol + gt_vol) and hd95_g = cwf_hausdorff's hd95 of (pred_g, lesion g) (unit spacing, connectivity 1), or
 *   0 and `penalty` if nothing touches it.  FP = components touching no lesion; kept = lesions with gt_vol > min_lesion_voxels;
 *   n = kept + FP.
 *   summary[b][r][2]      lw_dice = sum over kept of dice_g / n, lw_hd95 = (sum over kept of hd95_g + FP * penalty) / n, summed in
 *                         increasing g in float64; (1, 0) if n == 0
 *   counts[b][r][6]       G, kept, matched components (P - FP), FP, FN (kept lesions that nothing touches), P
 *   overflow[b][r]        1 if G > CWF_LESIONWISE_MAX: every other output of that (b, r) is then left untouched; else 0
 *   table[b][r][64][4]    gt_vol, pred_vol, inter, touching components of lesion g at row g - 1; rows >= G are 0
 *   lesion_hd95[b][r][64] hd95_g (penalty for a lesion nothing touches); entries >= G are 0
 * ws: cwf_lesionwise_workspace(...) bytes, 256-B aligned.  The call waits on the stream once, to read the B * R lesion counts that
 * size the cwf_hausdorff calls (eight lesions per call), so it cannot be captured into a graph.  No kernel waits on another workgroup.
 * CWF_E_BADARG: a null pointer, R > 8, B, R or an extent <= 0, dilation outside 0..8, a negative min_lesion_voxels, a negative or
 * non-finite penalty; CWF_E_TOOLARGE: 2^31 voxels or more, D2 > 4096, B * R > 65535 or ws_bytes too small. */
int cwf_lesionwise(const uint8_t* pred, const uint8_t* gt, int B, int R, int D0, int D1, int D2, int dilation, int64_t min_lesion_voxels,
                   double penalty, double* summary, int64_t* counts, int32_t* overflow, int64_t* table, double* lesion_hd95, void* ws,
                   int64_t ws_bytes, void* stream);
/* cwf_lesionwise plus the lesion-wise normalised surface Dice at tau[0..T), 0 <= T <= 4 (host memory): cwf_surface_metrics takes
 * cwf_hausdorff's place (unit spacing, connectivity 1, eight lesions per call), every other output is what cwf_lesionwise gives.
 *   lesion_nsd[b][r][64][T]  nsd of (pred_g, lesion g) as cwf_surface_metrics defines it; 0 for a lesion nothing touches; rows >= G are 0
 *   lw_nsd[b][r][T]          (sum over kept lesions of nsd_g) / (kept + FP), summed in increasing g in float64; 1 if kept + FP == 0
 *                            (false-positive components contribute 0, as to lw_dice)
 * Both are left untouched where overflow[b][r] is 1; with T == 0 tau and both may be null.  ws: cwf_lesionwise_ex_workspace(...)
 * bytes, 256-B aligned.  CWF_E_BADARG also for T outside 0..4 and a negative or NaN tau. */
int64_t cwf_lesionwise_ex_workspace(int B, int R, int D0, int D1, int D2);
int cwf_lesionwise_ex(const uint8_t* pred, const uint8_t* gt, int B, int R, int D0, int D1, int D2, int dilation, int64_t min_lesion_voxels,
                      double penalty, const double* tau, int T, double* summary, int64_t* counts, int32_t* overflow, int64_t* table,
                      double* lesion_hd95, double* lesion_nsd, double* lw_nsd, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N5  sliding-window inference over volumes of any size (predict_overlap.sliding_window_inference): overlapping r0 x r1 x r2
 *     windows on a Cartesian grid of starts, blended with a separable importance map.
 * ---------------------------------------------------------------------------------------------- */
#define CWF_WINDOW_MAX_STARTS 128
/* The window grid (host memory, passed by pointer, copied into the launch).  Window w = (i0 * n1 + i1) * n2 + i2 (axis 0 slowest)
 * covers voxels [start[a][i_a], start[a][i_a] + r[a]) of a [B][4][S0][S1][S2] volume along each axis a; every window must overlap
 * the volume (-r[a] < start < S[a]); voxels of a window outside the volume are zero padding.                                       */
struct cwf_window_grid {
  int B;
  int S[3];
  int r[3];
  int n[3];                                   /* 1 .. CWF_WINDOW_MAX_STARTS windows per axis */
  int start[3][CWF_WINDOW_MAX_STARTS];
};
/* windows[(j*B + b)][r0][r1][r2][4] (channels-last, 16-B aligned) <- x[b][4][S0][S1][S2] (contiguous NCDHW) cut at window w0 + j,
 * j < count, zeros outside the volume.  Viewed as NCDHW [count*B, 4, r0, r1, r2] it is the model's input with channels-last memory. */
int cwf_window_gather(const float* x, float* windows, const struct cwf_window_grid* grid, int w0, int count, void* stream);
/* acc[b][S0][S1][S2][4] (16-B aligned) += wt(v - s_w) * probs[(j*B + b)][v - s_w][4] for the windows w = w0 + j (j < count) that cover
 * voxel v, in window order, added one after another into the value loaded (accumulate = 0: into 0; the first chunk's launch then
 * also clears the voxels none of its windows covers).  probs: the model's output for the chunk in channels-last memory (16-B aligned).
 * weights: the 1-D importance tables g0[r0], g1[r1], g2[r2] back to back; wt(l) = fp32(fp32(g0[l0] * g1[l1]) * g2[l2]).
 * No atomics: the per-voxel sequence of fp32 operations does not depend on how the windows are split into chunks.                  */
int cwf_window_blend(const float* probs, const float* weights, float* acc, const struct cwf_window_grid* grid, int w0, int count,
                     int accumulate, void* stream);
/* y[b][c][S0][S1][S2] (NCDHW) = acc[b][v][c] / (sum of wt over all windows covering v, in window order); 0 / 0 = NaN where no
 * window covers v.                                                                                                                  */
int cwf_window_finalize(const float* acc, const float* weights, float* y, const struct cwf_window_grid* grid, void* stream);
/* CWF_E_BADARG (all three): a null pointer, a misaligned windows / probs / acc (16 B) or x / weights / y (4 B), B, S, r or n out of
 * range, a window entirely outside the volume, count <= 0 or windows past the last; CWF_E_TOOLARGE: 2^31 voxels or more in the
 * volume or a window, count * B > 65535.                                                                                             */
/* Windows on a sub-box of a volume, read and written in place (sliding_window_inference(crop_nonzero=True): the windows cover the
 * nonzero box of the brain only).  The box covers voxels [lo[a], lo[a] + grid->S[a]) of a [B][4][full0][full1][full2] volume: the
 * grid's S is the BOX's extent and its starts are box coordinates.                                                                  */
struct cwf_window_box {
  int full[3];                                /* the extent of the whole volume */
  int lo[3];                                  /* the box's low corner in it; lo[a] >= 0, lo[a] + S[a] <= full[a] */
};
/* cwf_window_gather of the contiguous copy x[:, :, lo0:lo0+S0, lo1:lo1+S1, lo2:lo2+S2], bit for bit, without the copy: x is the whole
 * volume; voxels of a window outside the BOX are zero, whatever the volume holds there.                                             */
int cwf_window_gather_box(const float* x, float* windows, const struct cwf_window_grid* grid, const struct cwf_window_box* box, int w0,
                          int count, void* stream);
/* acc[b][S0][S1][S2][4] in box coordinates, as cwf_window_blend leaves it; y[b][4][full0][full1][full2] the whole volume: inside the
 * box what cwf_window_finalize writes, bit for bit; outside it the background one-hot (1, 0, 0, 0).  One thread per voxel of the whole
 * volume: every element of y is written exactly once, no fill pass and no paste copy.                                                */
int cwf_window_finalize_box(const float* acc, const float* weights, float* y, const struct cwf_window_grid* grid,
                            const struct cwf_window_box* box, void* stream);
/* Both refuse what cwf_window_gather / cwf_window_finalize refuse, with the same codes, and CWF_E_BADARG: a null box, full < 1,
 * lo < 0 or lo + S > full along an axis; CWF_E_TOOLARGE: 2^31 voxels or more in the whole volume.  cwf_window_gather and
 * cwf_window_finalize are these two with the box the whole volume.                                                                   */

/* ------------------------------------------------------------------------------------------------
 * N3  training-batch preparation (utils/data.py prepare_batch / DeviceBraTS: crop, flips, intensity, label remap, edge codes)
 * ---------------------------------------------------------------------------------------------- */
/* One source subject: image fp32 [4][S0][S1][S2] and label uint8 [S0][S1][S2] (values 0..4), both contiguous device memory; crop
 * origin o* in [0, max(S* - C*, 0)]; flip bit i reverses output axis i; intensity != 0 applies x * scale[c] + shift[c]. */
struct cwf_prep_sample {
  const float* image; const uint8_t* label;
  int S0, S1, S2, o0, o1, o2, flip, intensity;
  float scale[4], shift[4];
};
/* For each of the B samples (h_samples is HOST memory, passed to the kernels by value: nothing is copied host-to-device, so the call
 * can be captured), with p the output voxel of the shared crop C0 x C1 x C2 and s_i = o_i + (flip_i ? C_i-1-p_i : p_i):
 *   x      [b*x_bstride + c*C0*C1*C2 + p]  image[c][s] (0 where some s_i >= S_i), or fadd_rn(fmul_rn(that, scale[c]), shift[c])
 *   target [b*t_bstride + p]               label[s] with 4 -> 3 (0 outside the volume), int64
 *   edge   [b*e_bstride + p]               utils.synthetic.edge_codes of the cropped, flipped target, int64
 * Eight samples per launch.  CWF_E_BADARG: B or a crop extent <= 0, an origin out of range, a flip mask > 7, a null or
 * misaligned pointer (image / x 4 B, target / edge 8 B), a stride smaller than one sample; CWF_E_TOOLARGE: 2^31 output voxels or more. */
int cwf_prepare_batch(const struct cwf_prep_sample* h_samples, int B, int C0, int C1, int C2, float* x, int64_t x_bstride,
                      int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride, void* stream);
/* cwf_prep_sample plus the linear part m[3*d + j] = M[d][j] of the output -> source map (rotation and zoom about the crop centre);
 * the origin may be any integer. */
struct cwf_prep_affine_sample {
  const float* image; const uint8_t* label;
  int S0, S1, S2, o0, o1, o2, flip, intensity;
  float scale[4], shift[4];
  float m[9];
};
/* cwf_prepare_batch with a resampled crop.  With c_d = (C_d - 1) / 2, p'_d = flip_d ? C_d-1-p_d : p_d, u_d = float(p'_d) - c_d and
 * every operation a float32 round-to-nearest one in the association written (no fused multiply-add):
 *   q_d    = ((m[3d]*u_0 + m[3d+1]*u_1) + m[3d+2]*u_2) + c_d                    crop-local source coordinate
 *   x      trilinear: i_d = floor(q_d), f_d = q_d - i_d, taps image[c][o + i + {0,1}^3] (0.0 where an index leaves [0, S_d)),
 *          lerp(a, b, f) = a + f*(b - a) along axis 2, then 1, then 0; then the intensity map of cwf_prepare_batch
 *   target label[o + floor(q + 0.5f)] with 4 -> 3 (0 outside the volume), int64
 *   edge   utils.synthetic.edge_codes of that target within the crop, int64
 * A voxel with some |q_d| >= 2^30 or NaN has every tap and its label outside the volume.  An identity m reproduces
 * cwf_prepare_batch's values.  Eight samples per launch, passed by value as there.  CWF_E_BADARG as for cwf_prepare_batch except
 * that every origin is accepted, and for a non-finite m entry; CWF_E_TOOLARGE: 2^31 output voxels or more. */
int cwf_prepare_batch_affine(const struct cwf_prep_affine_sample* h_samples, int B, int C0, int C1, int C2, float* x,
                             int64_t x_bstride, int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride, void* stream);
/* cwf_prep_affine_sample plus the control grid of an elastic deformation: disp is DEVICE memory, fp32 [3][G0][G1][G2] (4-byte
 * aligned), displacements in voxels of the crop-local source coordinate q; 4 <= G_d <= 8.  disp == NULL: no deformation, G* unused. */
struct cwf_prep_elastic_sample {
  const float* image; const uint8_t* label;
  int S0, S1, S2, o0, o1, o2, flip, intensity;
  float scale[4], shift[4];
  float m[9];
  const float* disp;
  int G0, G1, G2;
};
/* cwf_prepare_batch_affine with D added to the source coordinate, D a uniform cubic B-spline of the flipped output index p' over the
 * control grid.  Every operation is a float32 round-to-nearest one in the association written (no fused multiply-add); along axis d
 *   k_d  = float(G_d - 3) / float(C_d - 1)                      (correctly rounded; 0 when C_d == 1)
 *   g_d  = p'_d * k_d + 1;  i_d = floor(g_d);  t = g_d - i_d;  s = 1 - t;  h = float(1/6)
 *   w0 = ((s*s)*s)*h   w1 = ((((3*t - 6)*t)*t) + 4)*h   w2 = ((((-3*t + 3)*t + 3)*t) + 1)*h   w3 = ((t*t)*t)*h
 *   control index along d for j = 0..3: clamp(i_d - 1 + j, 0, G_d - 1)   (only i_d + 2 == G_d is ever clamped, where w3 is 0 or one
 *                                                                        rounding away from it)
 *   D_c  = sum_j0 w[0][j0] * (sum_j1 w[1][j1] * (sum_j2 w[2][j2] * disp[c][..][..][..])),  every 4-term sum as ((a + b) + c) + d
 *   q_c  = (cwf_prepare_batch_affine's q_c) + D_c
 * and x, target and edge follow from q as there, the |q_d| < 2^30 test being made on this final q: a NaN or huge control value makes
 * the voxels it reaches read nothing (image 0, label 0), and no value of disp can cause a read outside the volumes or the grid.  A
 * sample with disp == NULL gets no addition at all and is bit-equal to cwf_prepare_batch_affine's output for it.  The grids are read
 * when the kernel runs: they must stay valid until then.  CWF_E_BADARG as for cwf_prepare_batch_affine, and for a non-NULL disp that
 * is misaligned or comes with some G_d outside 4..8. */
int cwf_prepare_batch_elastic(const struct cwf_prep_elastic_sample* h_samples, int B, int C0, int C1, int C2, float* x,
                              int64_t x_bstride, int64_t* target, int64_t t_bstride, int64_t* edge, int64_t e_bstride, void* stream);
/* The intensity stage of one prepared sample x [4][C0][C1][C2] (utils/data.py: blur, noise, gamma).  blur / noise / gam are 4-bit
 * channel masks (bit c = channel c); taps[c] are the seven blur weights, amp[c] the noise amplitude, gamma[c] the exponent.  Values
 * of a channel whose bit is off are not used (taps and amp must still be finite, amp >= 0). */
struct cwf_intensity_sample {
  float taps[4][7];
  float amp[4];
  uint64_t key;
  float gamma[4];
  int blur, noise, gam;
};
#define CWF_INTENSITY_T0 10   /* the blur's tile: output voxels per workgroup along axis 0, 1, 2 (3-voxel halo on every side) */
#define CWF_INTENSITY_T1 10
#define CWF_INTENSITY_T2 32
/* dst[b][c] = the stage applied to src[b][c], for each of the B samples (h_samples is HOST memory, passed by value, eight samples
 * per launch: the call can be captured).  With V = C0*C1*C2, v = (p0*C1 + p1)*C2 + p2 and every operation a float32
 * round-to-nearest one in the association written (no fused multiply-add), per channel c, in this order:
 *   blur  (bit c of blur):  along axis 2, then 1, then 0, each pass rounded to float32,
 *           y[p] = (((((w0*a[p-3] + w1*a[p-2]) + w2*a[p-1]) + w3*a[p]) + w4*a[p+1]) + w5*a[p+2]) + w6*a[p+3],  w = taps[c],
 *           indices clamped to [0, C_d - 1] (replicate)
 *   noise (bit c of noise): h = splitmix64(key + uint64(c*V + v)) (wrapping),
 *           s = (h & 0xFFFF) + ((h >> 16) & 0xFFFF) + ((h >> 32) & 0xFFFF) + (h >> 48) - 131070,  x = x + float(s) * amp[c]
 *   gamma (bit c of gam):   mn, mx = the NaN-ignoring minimum and maximum of the channel after the two steps above, r = mx - mn;
 *           r not finite or not > 0: nothing; otherwise u = (x - mn) / r (correctly rounded), x = powf(u, gamma[c]) * r + mn
 * A channel with a bit off keeps its bits through that step (with all three off it is copied, or left alone when src == dst).
 * src and dst have their own sample strides (elements).  With a blur bit set anywhere src and dst must not overlap; without one
 * they may be the same buffer (in place) or disjoint.  ws: device scratch of at least 8 * B * tiles floats, tiles =
 * ceil(C0/T0) * ceil(C1/T1) * ceil(C2/T2), read and written only when some gam bit is set (the per-workgroup minima and maxima; a
 * second launch per eight samples reduces them and applies gamma in place on dst).  Nothing synchronises with the host.
 * CWF_E_BADARG, before any launch: B or a crop extent <= 0, a null or misaligned pointer (4 B), a stride smaller than one sample, a
 * mask outside 0..15, a non-finite tap or amplitude or a negative amplitude, a gamma that is not finite or not > 0 where its bit is
 * set, overlapping src and dst as above, gamma on with ws null or ws_floats too small; CWF_E_TOOLARGE: 2^31 voxels or more. */
int cwf_augment_intensity(const struct cwf_intensity_sample* h_samples, int B, int C0, int C1, int C2, const float* src,
                          int64_t src_bstride, float* dst, int64_t dst_bstride, float* ws, int64_t ws_floats, void* stream);
/* The acquisition stage of one prepared sample x [4][C0][C1][C2] (utils/data.py: bias field, contrast, low-resolution simulation).
 * bias_mask / contrast_mask / lowres_mask are 4-bit channel masks (bit c = channel c).  bias[c] is DEVICE memory, the control
 * multipliers of channel c, fp32 [G0][G1][G2] (4-byte aligned, 4 <= G_d <= 8, one grid shape for the sample's channels), read when
 * the kernel runs; factor[c] is the contrast factor; lattice[c][d] the extent n_d of channel c's coarse lattice along axis d.  Values
 * of a channel whose bit is off are not used. */
struct cwf_acquire_sample {
  const float* bias[4];
  int G0, G1, G2;
  int bias_mask, contrast_mask, lowres_mask;
  float factor[4];
  int lattice[4][3];
};
#define CWF_ACQUIRE_T0 32   /* voxels per workgroup along axis 0, 1, 2: one (float64 sum, min, max) partial per such tile */
#define CWF_ACQUIRE_T1 8
#define CWF_ACQUIRE_T2 32
/* dst[b][c] = the stage applied to src[b][c], for each of the B samples (h_samples is HOST memory, passed by value, eight samples
 * per launch: the call can be captured).  It runs after a prepare entry and before cwf_augment_intensity.  With V = C0*C1*C2, p =
 * (p0, p1, p2) the crop voxel and every operation a float32 round-to-nearest one in the association written (no fused
 * multiply-add), per channel c, in this order:
 *   bias (bit c of bias_mask):  x = x * m(p),  m(p) = sum_j0 w[0][j0] * (sum_j1 w[1][j1] * (sum_j2 w[2][j2] * bias[c][..][..][..]))
 *           with the weights w, the clamped control indices and the ((a + b) + c) + d sums of cwf_prepare_batch_elastic's D_c, taken
 *           at the crop index p itself (no flip: the stage acts on the finished crop)
 *   contrast (bit c of contrast_mask):  S = the float64 sum of the channel after the bias step, mean = float(S / V); mn, mx the
 *           NaN-ignoring minimum and maximum; mean not finite: nothing; otherwise
 *           x = fminf(fmaxf(((x - mean) * factor[c]) + mean, mn), mx).  S is formed from one float64 partial per tile of
 *           T0 x T1 x T2 voxels, each summed and then all reduced in a fixed order: the same input gives the same bits on every
 *           run, but S is not tied to any other summation order, so the result is bit-defined only where the float64 sum is exact.
 *   lowres (bit c of lowres_mask), n_d = lattice[c][d]:  lattice point k along axis d samples crop index s_d(k) = ((2k + 1) * C_d) /
 *           (2 * n_d) (integer division); r_d = float(n_d) / float(C_d) (correctly rounded), u = (float(p_d) + 0.5) * r_d - 0.5
 *           clamped to [0, float(n_d - 1)], k = min(floor(u), n_d - 2) (0 when n_d == 1), t = u - float(k), taps s_d(k) and
 *           s_d(min(k + 1, n_d - 1)); lerp(a, b, t) = a + t*(b - a) along axis 2, then 1, then 0, over the eight taps of the channel
 *           as the contrast step left it.  No coarse volume is formed.  (n_d == C_d gives t = 0 and tap p_d itself everywhere but
 *           at p_d = C_d - 1 > 0, where t = 1 and the result is a + (b - a).)
 * A channel with a bit off keeps its bits through that step.
 * Buffers: src and dst have their own sample strides (elements).  Without a lowres bit anywhere they may be the same buffer with
 * the same stride (in place) or disjoint, and src is only read.  With a lowres bit set anywhere they must be disjoint, and src is
 * also WRITTEN: a channel whose lowres bit is set gets its bias and contrast steps in place in src, from where the gather reads
 * its taps; the other channels of src are left alone.  Any other overlap is refused.  ws: device scratch of at least 12 * B * tiles
 * doubles (8-byte aligned), tiles = ceil(C0/T0) * ceil(C1/T1) * ceil(C2/T2), read and written only when some contrast bit is set.
 * Launches per eight samples: the partials (only with a contrast bit), the pointwise store (bias, contrast, copies), the gather
 * (only with a lowres bit).  Nothing is copied host to device and nothing synchronises with the host.
 * CWF_E_BADARG, before any launch: B or a crop extent <= 0, a null or misaligned pointer (src / dst 4 B, ws 8 B, a grid whose bit
 * is set 4 B), a stride smaller than one sample, a mask outside 0..15, some G_d outside 4..8 in a sample with a bias bit, a factor
 * that is not finite or not > 0 where its bit is set, a lattice entry outside [1, C_d] where its bit is set, overlapping src and dst
 * as above, contrast on with ws null or ws_doubles too small; CWF_E_TOOLARGE: 2^31 voxels or more. */
int cwf_augment_acquisition(const struct cwf_acquire_sample* h_samples, int B, int C0, int C1, int C2, float* src,
                            int64_t src_bstride, float* dst, int64_t dst_bstride, double* ws, int64_t ws_doubles, void* stream);
/* In place on one subject image fp32 [4][V]: over the voxels whose ((x0 + x1) + x2) + x3 > 0 (float32), each channel becomes
 * float32((x - mean_c) / std_c) with the float64 mean and population std of that channel over those voxels (two passes); other voxels,
 * and channels with std 0, are untouched.  ws: CWF_NORM_WS_DOUBLES doubles of device scratch. */
#define CWF_NORM_WS_DOUBLES 2568
int cwf_normalize_nonzero(float* image, int64_t V, double* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N4  class location tables of one subject's label, for foreground-oversampled crops (csrc/locations.hip)
 *   label uint8 [V] (any byte alignment), v the C-order linear index.  Values 0..4 are classes, 4 read as 3; any other value belongs to
 *   no region.  Region r = class bitmask posmasks[r] over classes 0..3 (host memory, R values, copied into the launches), 1 <= R <= 8;
 *   regions may overlap.
 *   counts int64 [R]: counts[r] = n_r, the voxels of region r.
 *   table int32 [R][K], 1 <= K <= 65536: with m_r = min(n_r, K), table[r][j] for j < m_r is the linear index of the region voxel of rank
 *   floor(j n_r / m_r), ranks counted in increasing linear index (exact integers); table[r][j] = -1 for j >= m_r.  With n_r <= K the
 *   row lists every voxel of the region, otherwise an evenly ranked sample.  The result depends on nothing but the label.
 * ---------------------------------------------------------------------------------------------- */
#define CWF_LOCATIONS_TILE 16384   /* consecutive voxels of one workgroup, counted from the 16-byte boundary at or below `label` */
/* Bytes of device workspace cwf_class_locations needs (4 R bytes per tile, 256-B aligned), or CWF_E_BADARG for V < 1, V > 2^31 - 1 or
 * R outside 1..8. */
int64_t cwf_class_locations_workspace(int64_t V, int R);
/* Three launches (count, scan, select); no atomics, no host synchronisation, nothing read back, no kernel waits on another workgroup:
 * capturable.  ws may hold anything; counts and table are fully written.  Before any launch: CWF_E_BADARG for a null pointer, V < 1 or
 * V > 2^31 - 1, R outside 1..8, K outside 1..65536, a posmask with bits above class 3; CWF_E_ALIGN for ws off 256 bytes. */
int cwf_class_locations(const uint8_t* label, int64_t V, const uint32_t* posmasks, int R, int K, int64_t* counts, int32_t* table,
                        void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N9  the nonzero bounding box of four-channel volumes (csrc/nonzero_box.hip): where the skull-stripped brain lies in a BraTS volume
 *   x fp32 [B][4][S0][S1][S2]: sample b at x + b * bstride floats (bstride >= 4 V, V = S0 S1 S2 <= 2^31 - 1), its four channels
 *   contiguous; any 4-byte alignment.  A voxel is nonzero iff (bits & 0x7fffffff) != 0 in some channel: +-0 is background, denormals,
 *   infinities and NaN are not (the bits are tested, not a float compare).
 *   box int32 [B][6] = lo0, lo1, lo2, hi0, hi1, hi2 (hi exclusive): the tightest box holding every nonzero voxel of the sample.
 *   count int64 [B]: its nonzero voxels.  A sample without one: lo = S, hi = 0, count = 0.  The result depends on nothing but x.
 * ---------------------------------------------------------------------------------------------- */
#define CWF_NONZERO_BOX_TILE 4096  /* consecutive voxels of one workgroup, counted from the 16-byte boundary at or below the sample */
/* Bytes of device workspace cwf_nonzero_box needs (32 bytes per tile and sample, 256-B aligned), or the code cwf_nonzero_box returns
 * for the same B and extents. */
int64_t cwf_nonzero_box_workspace(int B, int S0, int S1, int S2);
/* Two launches (per-tile partials stored plainly, a one-workgroup finalize per sample); no atomics, no host synchronisation, nothing
 * read back: capturable.  ws may hold anything; box and count are fully written.  Before any launch: CWF_E_BADARG for a null pointer,
 * B < 1, an extent < 1, bstride < 4 V; CWF_E_TOOLARGE for V > 2^31 - 1 or B > 65535; CWF_E_ALIGN for x or box off 4 bytes, count off
 * 8, ws off 256. */
int cwf_nonzero_box(const float* x, int64_t bstride, int B, int S0, int S1, int S2, int32_t* box, int64_t* count, void* ws,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * K11 fused Adam (amsgrad, L2 weight decay in the gradient)  torch.optim.Adam as used at train_no_amp.py:136,239
 *   table: device array of cwf_adam_desc; one launch updates every parameter.
 * ---------------------------------------------------------------------------------------------- */
struct cwf_adam_desc { float* p; const float* g; float* m; float* v; float* vmax; int64_t n; };
int cwf_adam_amsgrad(const struct cwf_adam_desc* table, int ntensors, int64_t max_n,
                     double lr, double beta1, double beta2, double eps, double weight_decay, int step, int amsgrad,
                     const float* hyper_dev, void* stream);
/* the same with the gradient read as g * grad_scale (1 / world size: the summed all-reduce result becomes the average here) */
int cwf_adam_amsgrad_scaled(const struct cwf_adam_desc* table, int ntensors, int64_t max_n,
                            double lr, double beta1, double beta2, double eps, double weight_decay, int step, int amsgrad,
                            const float* hyper_dev, float grad_scale, void* stream);
/* hyper-parameters in double: torch derives step_size = lr/(1-beta1^t) and sqrt(1-beta2^t) in double.  hyper_dev
 * (nullable): device float[2] = {step_size, sqrt(1-beta2^t)} overriding the values derived from lr/step -- lets the
 * launch be captured in a hipGraph and replayed while the host advances the schedule.                                  */

/* ------------------------------------------------------------------------------------------------
 * K13 step controls on the flat gradient buffer: accumulation over micro-batches, clipping by global norm, EMA weights
 * ---------------------------------------------------------------------------------------------- */
/* y[i] = a[i] + b[i], one rounded fp32 addition each; b == NULL: y[i] = a[i].  y may be a or b themselves (not a shifted overlap).
 * Pointers need 4-byte alignment only (slices of the flat buffer): 16-byte accesses when a, b and y are congruent mod 16, between
 * a scalar head and tail; grid-stride with a capped grid.  CWF_E_BADARG: a or y null, n <= 0; CWF_E_ALIGN: a pointer off 4 bytes. */
int cwf_grad_add(const float* a, const float* b, float* y, int64_t n, void* stream);
/* Global L2 norm of g * grad_scale and the clip coefficient of torch.nn.utils.clip_grad_norm_, both left on the device:
 *   out2[1] = grad_scale * sqrt(S),  S = sum g[i]^2 (every value widened to double before squaring, summed in double)
 *   out2[0] = grad_scale * min(1, max_norm / (out2[1] + 1e-6))      -- what cwf_adam_amsgrad_ex reads as its gradient scale
 * Two launches: CWF_GRADNORM_WS_DOUBLES workgroups each store the sum over a fixed contiguous range into ws (plain stores, no
 * atomics), one workgroup adds those partials in a fixed order: bit-identical from run to run.  max_norm = +inf gives
 * out2[0] = grad_scale (norm only).  A non-finite S propagates (inf: coefficient 0, NaN: NaN) as in torch; no step is skipped.
 * ws: CWF_GRADNORM_WS_DOUBLES doubles of device scratch, fully rewritten.  CWF_E_BADARG: a null pointer, n <= 0, a negative or NaN
 * max_norm, a NaN grad_scale; CWF_E_ALIGN: g / out2 off 4 bytes, ws off 8. */
#define CWF_GRADNORM_WS_DOUBLES 1024
int cwf_grad_norm_clip(const float* g, int64_t n, float grad_scale, float max_norm, double* ws, float* out2, void* stream);
/* cwf_adam_amsgrad_scaled with two optional additions.  gscale_dev (nullable): device float whose value replaces grad_scale, read
 * by the kernel (out2 of cwf_grad_norm_clip).  ema_table (nullable): device array of ntensors float pointers parallel to table;
 * after the update ema[i] += ema_weight * (p_new[i] - ema[i]), ema_weight = 1 - decay in (0, 0.5] (Tensor.lerp_, weight < 0.5).
 * CWF_E_BADARG: a null table, ema_weight outside (0, 0.5] with an ema_table, step <= 0 without hyper_dev. */
int cwf_adam_amsgrad_ex(const struct cwf_adam_desc* table, int ntensors, int64_t max_n,
                        double lr, double beta1, double beta2, double eps, double weight_decay, int step, int amsgrad,
                        const float* hyper_dev, float grad_scale, const float* gscale_dev, float* const* ema_table, float ema_weight,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * K14 further update rules of the fused step (csrc/optim_rules.hip): one launch over a cwf_adam_desc table, as above
 * ---------------------------------------------------------------------------------------------- */
/* CWF_RULE_ADAMW -- torch.optim.AdamW (decoupled decay), per element, g = g_raw * scale:
 *   p <- p * float(1 - lr * weight_decay * mul_t)                                (the factor is formed in double, once per workgroup)
 *   m <- m + (1 - beta1) (g - m);  v <- beta2 v + (1 - beta2) g g;  amsgrad: vmax <- max(vmax, v) takes v's place below
 *   p <- p - step_size * (m / (sqrt(v) / bc2_sqrt + eps)),  step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step), both
 *   derived in double here; hyper_dev (nullable): device float[2] = {step_size, bc2_sqrt} that replaces them, as in cwf_adam_amsgrad
 *   (the decay factor still uses the lr argument).  momentum, dampening, nesterov and first are ignored.
 * CWF_RULE_SGD -- torch.optim.SGD, per element:
 *   g <- g_raw * scale + float(weight_decay * mul_t) * p
 *   momentum > 0:  buf <- g if `first` (the buffers' first update: dampening is not applied), else momentum * buf + (1 - dampening) g
 *                  g <- g + momentum * buf with nesterov, else g <- buf
 *   p <- p - lr * g
 *   buf is the descriptor's m; v and vmax are never touched and may be null; with momentum = 0 neither is m.  beta1, beta2, eps,
 *   step, amsgrad and hyper_dev are ignored.
 * wd_mul (nullable): device array of ntensors floats, mul_t above -- 0 for a tensor that is not decayed, 1 otherwise; null: all ones.
 * scale is grad_scale, or the device float gscale_dev[0] when gscale_dev is given (out2 of cwf_grad_norm_clip); ema_table and
 * ema_weight as in cwf_adam_amsgrad_ex: ema += ema_weight * (p_new - ema) from the register that holds p_new.
 * Gradients need 4-byte alignment only (slices of the flat buffer); every access is one float.
 * CWF_E_BADARG, nothing launched: a null table; ntensors or max_n <= 0; a rule that is neither of the two; lr, weight_decay, momentum
 * or dampening NaN or negative; an ema_table with ema_weight outside (0, 0.5]; AdamW: step <= 0 without hyper_dev, a beta outside
 * [0, 1), eps NaN or negative; SGD: nesterov with momentum = 0 or dampening != 0 (torch's ValueError). */
#define CWF_RULE_ADAMW 1
#define CWF_RULE_SGD 2
int cwf_optim_step(int rule, const struct cwf_adam_desc* table, int ntensors, int64_t max_n, double lr, double weight_decay,
                   const float* wd_mul, double beta1, double beta2, double eps, int step, int amsgrad, const float* hyper_dev,
                   double momentum, double dampening, int nesterov, int first,
                   float grad_scale, const float* gscale_dev, float* const* ema_table, float ema_weight, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K12 / misc elementwise
 * ---------------------------------------------------------------------------------------------- */
/* y[i] = a[i]*b[i]  (dropout masks) ; y = a + b ; y[n][v][c] = x[n][v][c]*s[n][c] (dropout3d) ; fill */
/* K12: mask[i] = Bernoulli(1-p)/(1-p) [* Bernoulli(1-p2)/(1-p2)], counter-based (seed, offset + i): replaces the
 * rand / compare / cast / scale sequence behind F.dropout (SelfAttention.py:96-100, ResidualNorm.py:25-31,40-45) */
int cwf_dropout_mask(float* mask, int64_t n, float p, float p2, uint64_t seed, uint64_t offset, void* stream);
/* Device-resident generator state rng = uint64[2] {seed, step}.  cwf_rng_advance is a KERNEL (step += 1): captured in a hipGraph
 * it advances on every replay, so replayed training steps draw fresh masks.  Every fused dropout site evaluates
 * keep(i) = u01(seed, step, site_offset + i) >= p ? 1/(1-p) : 0 from the element index, forward and backward alike. */
int cwf_rng_advance(uint64_t* rng, void* stream);
int cwf_dropout_mask_rng(float* mask, int64_t n, float p, float p2, const uint64_t* rng, uint64_t offset, void* stream);
int cwf_mul(const float* a, const float* b, float* y, int64_t n, void* stream);
int cwf_add(const float* a, const float* b, float* y, int64_t n, void* stream);
int cwf_add3(const float* a, const float* b, const float* c, float* y, int64_t n, void* stream);   /* (a + b) + c: the three-region sums of the Mutual Cross-region Coupler, cls_wise_former.py:549-552 */
int cwf_bcast3(const float* x, float* y, int64_t n, void* stream);                 /* y[g][i] = x[i], g < 3: adjoint of the three-region sums */
int cwf_stats_channel_sum(const double* stats, float* out, int N, int C, void* stream);   /* out[c] = sum_n stats[n][c][0]: ConvTranspose bias gradient */
int cwf_channel_scale(const float* x, int x_ldc, const float* s, float* y, int y_ldc, int N, int64_t V, int C, void* stream);
int cwf_copy_strided(const float* x, int x_ldc, float* y, int y_ldc, int64_t nvox, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Launch plans: the captured training step (train_no_amp.py:181-239: forward, five losses, backward, gradient reduces) re-issued
 * as a plain launch list.  The step is static (fixed patch size, device-side top-k, device-resident dropout counters); the host
 * captures it once with HIP stream capture and hands the hipGraph_t over.  cwf_plan_create orders the graph's nodes
 * topologically and assigns them to streams along the capture's chains (main stream; weight-gradient side stream, low priority);
 * cwf_plan_run issues one plain launch per node plus an event pair per cross-stream edge -- hipGraphLaunch is not used (it costs
 * the host ~44 us per node on ROCm 7.2, more than an eager launch).  The graph must outlive the plan (argument blocks are read
 * from its nodes).  Unsupported node kinds (host nodes, child graphs, memcpy nodes) make cwf_plan_create return
 * CWF_E_TOOLARGE; the caller then replays the graph the ordinary way.
 * ---------------------------------------------------------------------------------------------- */
int cwf_plan_create(void* hip_graph, void** plan_out);
const char* cwf_plan_last_error(void);   /* which node made the last cwf_plan_create return CWF_E_TOOLARGE */
/* info8 = {nodes, kernel nodes, markers, streams used, cross-stream events, nodes on stream 0, on stream 1, on streams 2+} */
int cwf_plan_info(void* plan, int* info8);
/* Issues nodes [start, ...) on main_stream (chain 0) and the plan's own side streams until the list ends or a marker has been
 * processed; *next = position to continue from (= node count when finished), *marker_id = the marker's id or -1 when finished.
 * A marker's dependencies are enqueued as waits on comm_stream: work the caller puts on comm_stream after the call (the
 * data-parallel all-reduce of the gradient slice the marker closes) runs behind them.  On finish main_stream waits for the side
 * streams.                                                                                                                       */
int cwf_plan_run(void* plan, void* main_stream, void* comm_stream, int start, int* next, int* marker_id);
int cwf_plan_destroy(void* plan);
/* a no-op kernel carrying `id`: launched (under capture) on the communication stream to mark a cut point of the step */
int cwf_plan_marker(int id, void* stream);

/* The scheduling rules of cwf_plan_create on plain arrays; no HIP call, works without a GPU (cwf_plan_create calls the same code).
 * Nodes are named by creation index (the order the host issued the work in).  kind[n]: CWF_PLAN_*; cls[n]: CWF_PLAN_CLASS_* of a
 * kernel node, 0 for every other kind (cwf_plan_create derives it from the kernel's name: weight-gradient chain = SIDE, to_bf16
 * conversions = CONVERSION); edge_from / edge_to[n_edges]: the graph's edges.  Out: order[n] = creation index per plan position
 * (topological, smallest creation index first); stream[n] per position: 0 = the caller's stream, 1 = the side stream (SIDE nodes,
 * and a CONVERSION all of whose successors are on it), -1 = a marker (the communication stream); record[n]: an event is recorded
 * behind this position; wait_off[n + 1] / wait[2 n]: position i waits for the events of positions wait[wait_off[i] ..
 * wait_off[i + 1]), each earlier, on another stream and recorded.  One wait per source stream at most, none where the node's own
 * stream already waited for that position or a later one of the same source; a node behind a marker takes over the marker's waits.
 * CWF_E_BADARG: n <= 0, a null array, a kind or class out of range, a class on a node that is no kernel, an edge that names no
 * node, a cycle. */
#define CWF_PLAN_KERNEL 0
#define CWF_PLAN_MEMSET 1
#define CWF_PLAN_EMPTY  3
#define CWF_PLAN_MARKER 4
#define CWF_PLAN_CLASS_MAIN       0
#define CWF_PLAN_CLASS_SIDE       1
#define CWF_PLAN_CLASS_CONVERSION 2
int cwf_plan_schedule(int n, const int* kind, const int* cls, int n_edges, const int* edge_from, const int* edge_to,
                      int* order, int* stream, int* wait_off, int* wait, int* record);
/* Reading a built plan (nothing is launched).  counts3 = {positions, waits in all, edges of the graph}.  cwf_plan_describe fills,
 * per plan position: kind (CWF_PLAN_*), stream (0, 1, -1 for a marker), marker_id (-1 for any other kind), record, creation (index
 * in the graph's node list), wait_off[positions + 1] / wait[waits] as above; and the graph's edges as position pairs in
 * edge_from / edge_to[edges].  Any array may be NULL (wait_off with wait, edge_from with edge_to: both or neither).
 * cwf_plan_kernel_name copies the name hipKernelNameRefByPtr gave for the kernel at `position` into buf (at most cap - 1 characters
 * and a NUL; buf may be NULL with cap 0) and returns its full length: 0 for a memset, empty or marker node. */
int cwf_plan_counts(void* plan, int* counts3);
int cwf_plan_describe(void* plan, int* kind, int* stream, int* marker_id, int* record, int* creation, int* wait_off, int* wait,
                      int* edge_from, int* edge_to);
int cwf_plan_kernel_name(void* plan, int position, char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif
