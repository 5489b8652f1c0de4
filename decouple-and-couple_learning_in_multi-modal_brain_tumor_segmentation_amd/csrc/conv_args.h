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

// branch-free (Leaky)ReLU / identity for slope in [0,1]: max(v, slope*v)
__device__ __forceinline__ float act01(float v, float slope) { return fmaxf(v, v * slope); }

// ---- The 4x4x16 output tile of conv_ws / conv_wsp / conv_wsd and its halo, staged as an LDS image [voxel][16 channels] of bf16 by 256
// loader threads: thread tg holds channel quad tg & 3 of the voxels (tg >> 2) + HALO_DV i, i < HALO_SLOTS.
constexpr int HALO_D = 6, HALO_H = 6, HALO_W = 18;
constexpr int HALO_NVOX = HALO_D * HALO_H * HALO_W;                  // 648 halo voxels
constexpr int HALO_DV = 256 / 4;                                     // voxels between two staging slots of a thread
constexpr int HALO_SLOTS = (HALO_NVOX + HALO_DV - 1) / HALO_DV;      // 11 (the last one only for tg >> 2 < 8)
// byte offset in the image of the voxel that tap t = (kd * 3 + kh) * 3 + kw reads for output voxel 0
__host__ __device__ constexpr int halo_tap_bytes(int t) { return (((t / 9) * HALO_H + (t / 3) % 3) * HALO_W + t % 3) * 32; }

// One step of a loader thread's halo slot walk over the tile whose halo starts at voxel (id0, ih0, iw0) of its sample.  (iw, row) is
// the slot's voxel as (v % HALO_W, v / HALO_W), row = idd * HALO_H + ih, from ((tg >> 2) % HALO_W, (tg >> 2) / HALO_W) for slot 0; the step
// moves it on to the next slot.  Returns whether the voxel lies in the volume; boff: the byte offset of its channel quad q in the sample's
// fp32 tensor (ldc4 = 4 x_ldc bytes per voxel), clamped to voxel 0 outside the volume so that the caller's load can be unconditional.
__device__ __forceinline__ bool halo_slot_next(const ConvGeom& g, int id0, int ih0, int iw0, unsigned ldc4, int q, int& iw, int& row, unsigned& boff) {
  const int idd = (row * 43) >> 8, ih = row - idd * HALO_H;                   // row / 6 for row < 48
  const int gd = id0 + idd, gh = ih0 + ih, gw = iw0 + iw;
  const bool ok = (row < HALO_D * HALO_H) & ((unsigned)gd < (unsigned)g.Di) & ((unsigned)gh < (unsigned)g.Hi) & ((unsigned)gw < (unsigned)g.Wi);
  iw += HALO_DV % HALO_W; row += HALO_DV / HALO_W;                            // HALO_DV voxels on: 3 rows + 10
  if (iw >= HALO_W) { iw -= HALO_W; ++row; }
  const unsigned lin = (unsigned)((gd * g.Hi + gh) * g.Wi + gw) * ldc4 + (unsigned)q * 16u;
  boff = ok ? lin : (unsigned)q * 16u;
  return ok;
}

// sample and tile coordinates of tile index `tile` (tiles_per_n = g.tiles_d * g.tiles_h * g.tiles_w)
__device__ __forceinline__ void tile_pos(const ConvGeom& g, int tiles_per_n, int tile, int& n, int& td, int& th, int& tw) {
  n = tile / tiles_per_n;
  int bx = tile - n * tiles_per_n;
  tw = bx % g.tiles_w; bx /= g.tiles_w;
  th = bx % g.tiles_h; td = bx / g.tiles_h;
}

// Row epilogue of conv_bf16 (interior fast path) / conv_ws / conv_wsp / conv_wsd: the byte offset of a lane's element -- voxel vi of the
// row, channel c0 -- in a tensor of ldc floats per voxel, as an opaque copy (keeps the zero-extension at the access: saddr form).
__device__ __forceinline__ unsigned epi_lane_off(int vi, int ldc, int c0) {
  unsigned o = (unsigned)(vi * ldc + c0) * 4u;
  asm volatile("" : "+v"(o));
  return o;
}
// What one stored output element v adds to the sums of the row epilogue of conv_bf16 (interior fast path) / conv_ws / conv_wsp / conv_wsd:
// the InstanceNorm sums of v (stat_sums), or the norm-backward sums of gn = v act'(h), h = x * nsc + nsh (nb_sums; ConvArgsB::nb_x).
__device__ __forceinline__ void stat_sums(float v, float& s1, float& s2) { s1 += v; s2 = fmaf(v, v, s2); }
__device__ __forceinline__ void nb_sums(float v, float x, float nsc, float nsh, float nb_slope, float& s1, float& s2) {
  const float h = fmaf(x, nsc, nsh);
  const float gn = v * (h > 0.f ? 1.f : nb_slope);
  s1 += gn; s2 = fmaf(gn, h, s2);
}

// The statistics fold of conv_wsp / conv_wsd: a wave's fp32 partials (per lane, over the voxels the tap-table kernel would have summed)
// go through that kernel's two shuffles into the float64 sums, and start again from zero.
template <int NT>
__device__ __forceinline__ void fold_stats(float (&s1)[NT], float (&s2)[NT], double (&d1)[NT], double (&d2)[NT]) {
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    float u1 = s1[j], u2 = s2[j];
    u1 += __shfl_xor(u1, 16, 64); u1 += __shfl_xor(u1, 32, 64);
    u2 += __shfl_xor(u2, 16, 64); u2 += __shfl_xor(u2, 32, 64);
    d1[j] += (double)u1; d2[j] += (double)u2;
    s1[j] = 0.f; s2[j] = 0.f;
  }
}


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
