// Declarations shared by the split-bf16 conv kernels (conv_bf16.hip: tap-table kernel, conv16 / conv16s, pointwise streams;
// conv_ws.hip: weight-stationary kernel for the 32/64/128-channel 3x3x3 layers; conv_wsp.hip: its wave-specialised split-bf16 forward; conv_wsd.hip: the wave-specialised single-bf16 kernel of the small deep layers).
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct ConvArgsB {
  ConvGeom g;
  const float* x; const uint4* wpk; const float* bias; float* y;
  const float* in_scale; const float* in_shift; float in_slope;
  const float* residual; int r_ldc; const float* out_scale; double* stats;
  // 16 unused bytes: without them every later field moves and hipcc schedules conv16s_kernel / convws_kernel differently; they keep
  // the compiled kernels byte-for-byte as measured
  unsigned long long unused_[2];
  // "norm-backward" statistics (data-gradient launches whose output g feeds the backward of y = act(IN(x))): with nb_x set,
  // stats receives per (n, channel)  S1 = sum g*act'(h), S2 = sum g*act'(h)*h,  h = nb_x*nb_scale + nb_shift  -- what
  // cwf_in_bwd_stats would compute in a separate pass over g and x (norm.hip) -- instead of (sum y, sum y^2).
  const float* nb_x; int nb_ldc; const float* nb_scale; const float* nb_shift; float nb_slope;
  // channel-grouped launches (cwf_conv with groups: the three sub-regions' supervision-head convs as one launch): group q reads
  // input channels [q*x_goff, q*x_goff + Cin) and writes output channels [q*y_goff, q*y_goff + Cout) of the same voxel rows, with its
  // own packed weights and bias; blockIdx.z = (group * N + n) * ncls + class.  groups == 0: an ordinary launch.
  int groups, x_goff, y_goff;
  const uint4* wpk_g[3]; const float* bias_g[3];
  // conv16s / convws, IN16 instantiations: the input as a bf16 image [N][D][H][W][Cin] (16-byte granules) and the 16-byte zero page of
  // their loaders
  const uint4* x16; const uint4* zero16;
  // pointwise stream kernel (1x1x1 forward): the output also as a bf16 image [N][V][Cout] (the operand image of a consuming layer's weight
  // gradient, see cwf_conv_args.y16): one extra 8-byte store per lane
  unsigned short* y16;
};

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {          // one v_cvt_pk_bf16_f32
  const f32x2_t f = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2_t));
}
__device__ __forceinline__ float bf16_round(float a) { return (float)(__bf16)a; }
// split two floats into packed bf16 hi and lo (lo = bf16(v - hi)):  cvt_pk, shl/and, 2 sub, cvt_pk
__device__ __forceinline__ void split_bf16(float a, float b, unsigned& hi, unsigned& lo) {
  hi = pack_bf16(a, b);
  const float ha = __builtin_bit_cast(float, hi << 16), hb = __builtin_bit_cast(float, hi & 0xffff0000u);
  lo = pack_bf16(a - ha, b - hb);
}
// branch-free (Leaky)ReLU / identity for slope in [0,1]: max(v, slope*v)
__device__ __forceinline__ float act01(float v, float slope) { return fmaxf(v, v * slope); }


// The extent choose_cfg tiles (per output-parity class) and the class count of a launch: the output extent, or for the eight-class
// launches (ConvTranspose forward, stride-2 data gradient) the extent of one class.  Shared by the fp32 (conv_mfma.hip) and the
// split-bf16 (conv_bf16.hip) tap-table launches and their configuration queries.
static inline int cfg_extent(int op, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int cd[3]) {
  cd[0] = Do; cd[1] = Ho; cd[2] = Wo;
  if (op == CWF_CONVT2) { cd[0] = Di; cd[1] = Hi; cd[2] = Wi; return 8; }
  if (op == CWF_CONV3_S2_DGRAD) { cd[0] = (Do + 1) / 2; cd[1] = (Ho + 1) / 2; cd[2] = (Wo + 1) / 2; return 8; }
  return 1;
}

// conv_ws.hip: launches the weight-stationary kernel when the layer is one it takes (returns 1, status in *rc); 0 = not eligible.
int cwf_try_conv_ws(int op, int x3, ConvArgsB& a, hipStream_t st, int* rc);
// conv_ws.hip: 1 if its bf16-image instantiation takes a single-bf16 launch of these dimensions (the eligibility code of the dispatch)
int cwf_ws_takes_x16(int op, int N, int D, int H, int W, int Cin, int Cout);
// conv_ws.hip: 1 while cwf_debug_ws_x3 sends split-bf16 launches to the weight-stationary kernel
int cwf_ws_takes_x3();
// conv_wsp.hip: the wave-specialised split-bf16 forward of the 32-256-channel 3x3x3 layers (same contract as cwf_try_conv_ws; cfg_mt /
// cfg_wm: the tap-table configuration the launch would otherwise take, whose statistics partials it reproduces)
int cwf_try_conv_wsp(int op, int x3, int cfg_mt, int cfg_wm, ConvArgsB& a, hipStream_t st, int* rc);
// conv_wsd.hip: the wave-specialised weight-in-LDS single-bf16 kernel of the small 128 / 256-channel 3x3x3 layers (the data gradients at
// 16^3); same contract as cwf_try_conv_wsp
int cwf_try_conv_wsd(int op, int x3, int cfg_mt, int cfg_wm, ConvArgsB& a, hipStream_t st, int* rc);

// Host launchers behind the routers cwf_conv (conv_bf16.hip) and cwf_wgrad (wgrad_bf16.hip), which have checked the route.
int conv_fp32_launch(const cwf_conv_args& d, hipStream_t st);        // conv_mfma.hip: the fp32 tap-table kernel
int conv_stem_launch(const cwf_conv_args& d, hipStream_t st);        // conv_stem.hip: 4 -> 16 channels from the raw weight w_raw
int conv_s2c16_launch(const cwf_conv_args& d, hipStream_t st);       // conv_s2.hip: stride 2, 16 -> 32 channels from w_raw
int wgrad_fp32_launch(const cwf_wgrad_args& d, int* nsplit_used, hipStream_t st);   // wgrad_mfma.hip: the fp32 slab kernel
