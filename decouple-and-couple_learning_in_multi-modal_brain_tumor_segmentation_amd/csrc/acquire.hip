// N3 -- the acquisition stage of the batch preparer (utils/data.py: bias field, contrast, low-resolution simulation; statement:
// include/cwf_hip.h cwf_augment_acquisition).  It runs on the prepared crop x [B][4][C0][C1][C2], after a prepare kernel of prep.hip
// and before the intensity stage of intensity.hip.
//
// Every kernel: one 256-thread workgroup per (tile, channel, sample), the tile 32 x 8 x 32 voxels.  A thread owns the column
// (p1, p2) = (b1 + tid / 32, b2 + tid % 32) of the tile and walks its 32 voxels along axis 0, eight loads in flight: a half wave
// reads and writes 128 contiguous bytes.  A workgroup whose channel has nothing to do in a launch returns at once.
//   bias field: the spline is separable and a thread's axis-1 and axis-2 weights do not change along its column, so the thread folds
//     axes 2 and 1 over the whole control grid once -- the channel's grid (at most 512 floats) is staged in LDS, B[i0] = sum_j1 w1 *
//     (sum_j2 w2 * grid[i0][..][..]) for the G0 planes goes to the thread's own LDS column -- and a voxel then costs four products
//     with the axis-0 weights of its row (a table of the tile's 32 rows).  These are the statement's products and sums in its order.
//   acq_stats_kernel (channels with contrast): x * m in registers; the workgroup's float64 sum, minimum and maximum go to ws as
//     three doubles per tile.  Every sum is taken in a fixed order (a thread's column, the wave's butterfly, the four waves).
//   acq_point_kernel: every workgroup of a channel re-reduces that channel's partials (a few hundred triples, from L2) in one fixed
//     order, so all of them hold the same mean, then stores bias and contrast: into dst, or in place into src where the channel's
//     lowres bit is set (the gather reads it from there).  It also carries the plain copies of an out-of-place call.
//   acq_gather_kernel (channels with lowres): the lattice tap indices and fractions of the tile's 32 + 8 + 32 coordinates go to an LDS
//     table; a voxel gathers its eight taps from src (served by the vector cache and L2) and stores one dword to dst.
// No store is wider than a dword, so any 4-byte-aligned buffer with any sample stride takes the same path.
// This file is compiled with -ffp-contract=off.
#include "common.h"
#include <algorithm>
#include <cmath>

#define ACQ_MAXS 8                          // samples per launch
#define ACQ_T0 CWF_ACQUIRE_T0
#define ACQ_T1 CWF_ACQUIRE_T1
#define ACQ_T2 CWF_ACQUIRE_T2
#define ACQ_GMAX 8
#define ACQ_U 8                             // voxels of a column in flight
static_assert(ACQ_T1 * ACQ_T2 == 256 && ACQ_T2 == 32, "one column per thread, a tile row per half wave");
static_assert(ACQ_T0 % ACQ_U == 0, "whole rounds of a column");

struct AcqArgs {
  cwf_acquire_sample s[ACQ_MAXS];
  float k[ACQ_MAXS][3];                     // float(G_d - 3) / float(C_d - 1) of the sample's grid (0 when C_d == 1), divided on the host
  float r[ACQ_MAXS][4][3];                  // float(n_d) / float(C_d) of the channel's lattice, divided on the host
  float* src;
  float* dst;
  double* ws;                               // partials of this launch's first sample
  int64_t src_bs, dst_bs;                   // sample strides (elements)
  int C0, C1, C2, tiles, inplace;
};
static_assert(sizeof(AcqArgs) <= 4096, "the samples travel by value in the kernel-argument block");

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct AcqField {
  float cg[ACQ_GMAX * ACQ_GMAX * ACQ_GMAX]; // the channel's control grid
  float B[ACQ_GMAX][256];                   // thread tid's axes 2 and 1 folded, per control plane i0
  f32x4 w0[ACQ_T0];                         // axis-0 weights and control planes of the tile's rows
  i32x4 i0[ACQ_T0];
};

// ((w0*a + w1*b) + w2*c) + w3*d
__device__ __forceinline__ float acq_sum4(f32x4 w, float a, float b, float c, float d) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[0], a), __fmul_rn(w[1], b)), __fmul_rn(w[2], c)), __fmul_rn(w[3], d));
}

// weights and clamped control indices (times stride) of the crop index p along an axis of G control points: prep.hip's ela_axis
// without the flip
__device__ __forceinline__ void acq_axis(int p, int G, float k, int stride, f32x4& w, i32x4& ix) {
  const float g = __fadd_rn(__fmul_rn((float)p, k), 1.f);
  const float fl = floorf(g);
  const float t = __fsub_rn(g, fl), s = __fsub_rn(1.f, t), h = 0.16666667163372040f;
  w[0] = __fmul_rn(__fmul_rn(__fmul_rn(s, s), s), h);
  w[1] = __fmul_rn(__fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(3.f, t), 6.f), t), t), 4.f), h);
  w[2] = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(-3.f, t), 3.f), t), 3.f), t), 1.f), h);
  w[3] = __fmul_rn(__fmul_rn(__fmul_rn(t, t), t), h);
  const int i = (int)fl;                                      // 1 <= g <= G - 2 + one rounding: i is in [1, G - 2]
#pragma unroll
  for (int j = 0; j < 4; ++j) ix[j] = min(max(i - 1 + j, 0), G - 1) * stride;
}

// the field of channel c of sample S over the tile at (b0, b1, b2): after it, acq_field(F, j0) is m at the thread's voxel of row j0
__device__ __forceinline__ void acq_field_setup(AcqField& F, const cwf_acquire_sample& S, const float (&k)[3], int c, int b0, int b1,
                                                int b2, int C0, int C1, int C2, int tid) {
  const int G0 = S.G0, G1 = S.G1, G2 = S.G2, n = G0 * G1 * G2;  // <= 512 (checked on the host)
  const float* grid = S.bias[c];
  for (int i = tid; i < n; i += 256) F.cg[i] = grid[i];
  if (tid < ACQ_T0) {
    f32x4 w = {0.f, 0.f, 0.f, 0.f};
    i32x4 ix = {0, 0, 0, 0};
    if (b0 + tid < C0) acq_axis(b0 + tid, G0, k[0], 1, w, ix);
    F.w0[tid] = w;
    F.i0[tid] = ix;
  }
  __syncthreads();
  const int p1 = min(b1 + (tid >> 5), C1 - 1), p2 = min(b2 + (tid & 31), C2 - 1);   // (a column outside the crop is never stored)
  f32x4 w1, w2;
  i32x4 i1, i2;
  acq_axis(p1, G1, k[1], G2, w1, i1);
  acq_axis(p2, G2, k[2], 1, w2, i2);
#pragma unroll 1
  for (int g0 = 0; g0 < G0; ++g0) {
    float r[4];
#pragma unroll
    for (int j1 = 0; j1 < 4; ++j1) {
      const float* row = F.cg + g0 * G1 * G2 + i1[j1];
      r[j1] = acq_sum4(w2, row[i2[0]], row[i2[1]], row[i2[2]], row[i2[3]]);
    }
    F.B[g0][tid] = acq_sum4(w1, r[0], r[1], r[2], r[3]);
  }
  // (a thread reads back only its own column of B, and w0 / i0 were written before the barrier above)
}

__device__ __forceinline__ float acq_field(const AcqField& F, int j0, int tid) {
  const i32x4 ix = F.i0[j0];
  return acq_sum4(F.w0[j0], F.B[ix[0]][tid], F.B[ix[1]][tid], F.B[ix[2]][tid], F.B[ix[3]][tid]);
}

// sum (in a fixed order), minimum and maximum over the workgroup; valid in every thread
__device__ __forceinline__ void acq_block_reduce(double& s, float& mn, float& mx, double (&rs)[4], float (&rm)[2][4]) {
  s = wave_sum_d(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rm[0][threadIdx.x >> 6] = mn;
    rm[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  s = ((rs[0] + rs[1]) + rs[2]) + rs[3];
  mn = fminf(fminf(rm[0][0], rm[0][1]), fminf(rm[0][2], rm[0][3]));
  mx = fmaxf(fmaxf(rm[1][0], rm[1][1]), fmaxf(rm[1][2], rm[1][3]));
}

struct AcqTile {
  int b0, b1, b2;
};
__device__ __forceinline__ AcqTile acq_tile(int t, int C1, int C2) {
  const int n2 = (C2 + ACQ_T2 - 1) / ACQ_T2, n1 = (C1 + ACQ_T1 - 1) / ACQ_T1;
  return AcqTile{(t / (n2 * n1)) * ACQ_T0, ((t / n2) % n1) * ACQ_T1, (t % n2) * ACQ_T2};
}

__global__ __launch_bounds__(256) void acq_stats_kernel(const AcqArgs a) {
  __shared__ AcqField F;
  __shared__ double rs[4];
  __shared__ float rm[2][4];
  const cwf_acquire_sample& S = a.s[blockIdx.z];
  const int c = blockIdx.y, tid = threadIdx.x;
  if (!((S.contrast_mask >> c) & 1)) return;                  // (uniform over the workgroup)
  const bool bias = (S.bias_mask >> c) & 1;
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const AcqTile T = acq_tile(blockIdx.x, C1, C2);
  const int64_t V = (int64_t)C0 * C1 * C2;
  const float* src = a.src + (int64_t)blockIdx.z * a.src_bs + c * V;
  if (bias) acq_field_setup(F, S, a.k[blockIdx.z], c, T.b0, T.b1, T.b2, C0, C1, C2, tid);
  const int p1 = T.b1 + (tid >> 5), p2 = T.b2 + (tid & 31);
  const bool col = p1 < C1 && p2 < C2;
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll 1
  for (int j = 0; j < ACQ_T0; j += ACQ_U) {
    float y[ACQ_U];
#pragma unroll
    for (int u = 0; u < ACQ_U; ++u) {
      const int p0 = T.b0 + j + u;
      y[u] = (col && p0 < C0) ? src[((int64_t)p0 * C1 + p1) * C2 + p2] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < ACQ_U; ++u) {
      if (!(col && T.b0 + j + u < C0)) continue;
      const float v = bias ? __fmul_rn(y[u], acq_field(F, j + u, tid)) : y[u];
      s += (double)v;
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  acq_block_reduce(s, mn, mx, rs, rm);
  if (tid == 0) {
    double* part = a.ws + (((int64_t)blockIdx.z * 4 + c) * a.tiles + blockIdx.x) * 3;
    part[0] = s;
    part[1] = (double)mn;
    part[2] = (double)mx;
  }
}

__global__ __launch_bounds__(256) void acq_point_kernel(const AcqArgs a) {
  __shared__ AcqField F;
  __shared__ double rs[4];
  __shared__ float rm[2][4];
  const cwf_acquire_sample& S = a.s[blockIdx.z];
  const int c = blockIdx.y, tid = threadIdx.x;
  const bool bias = (S.bias_mask >> c) & 1, low = (S.lowres_mask >> c) & 1;
  bool con = (S.contrast_mask >> c) & 1;
  if (!bias && !con && (a.inplace || low)) return;            // (uniform over the workgroup)
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const AcqTile T = acq_tile(blockIdx.x, C1, C2);
  const int64_t V = (int64_t)C0 * C1 * C2;
  const float* src = a.src + (int64_t)blockIdx.z * a.src_bs + c * V;
  float* dst = low ? a.src + (int64_t)blockIdx.z * a.src_bs + c * V : a.dst + (int64_t)blockIdx.z * a.dst_bs + c * V;
  float mean = 0.f, mn = INFINITY, mx = -INFINITY;
  if (con) {
    const double* part = a.ws + ((int64_t)blockIdx.z * 4 + c) * a.tiles * 3;
    double s = 0.0;
    for (int i = tid; i < a.tiles; i += 256) {
      s += part[3 * i];
      mn = fminf(mn, (float)part[3 * i + 1]);
      mx = fmaxf(mx, (float)part[3 * i + 2]);
    }
    acq_block_reduce(s, mn, mx, rs, rm);
    mean = (float)(s / (double)V);
    con = isfinite(mean);
  }
  if (!bias && !con && (a.inplace || low)) return;            // a mean that is not finite: the channel stays as it is
  if (bias) acq_field_setup(F, S, a.k[blockIdx.z], c, T.b0, T.b1, T.b2, C0, C1, C2, tid);
  const float f = S.factor[c];
  const int p1 = T.b1 + (tid >> 5), p2 = T.b2 + (tid & 31);
  if (!(p1 < C1 && p2 < C2)) return;                          // (no barrier follows)
#pragma unroll 1
  for (int j = 0; j < ACQ_T0; j += ACQ_U) {
    float y[ACQ_U];
#pragma unroll
    for (int u = 0; u < ACQ_U; ++u) {
      const int p0 = T.b0 + j + u;
      y[u] = p0 < C0 ? src[((int64_t)p0 * C1 + p1) * C2 + p2] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < ACQ_U; ++u) {
      const int p0 = T.b0 + j + u;
      if (p0 >= C0) continue;
      float v = y[u];
      if (bias) v = __fmul_rn(v, acq_field(F, j + u, tid));
      if (con) v = fminf(fmaxf(__fadd_rn(__fmul_rn(__fsub_rn(v, mean), f), mean), mn), mx);
      dst[((int64_t)p0 * C1 + p1) * C2 + p2] = v;
    }
  }
}

// one coordinate of the interpolation back from a lattice of n points to C voxels: the two crop indices the taps read, and t
struct AcqTap {
  int lo, hi;
  float t;
};
__device__ __forceinline__ AcqTap acq_tap(int p, int C, int n, float r) {
  float u = __fsub_rn(__fmul_rn(__fadd_rn((float)p, 0.5f), r), 0.5f);
  u = fminf(fmaxf(u, 0.f), (float)(n - 1));
  const int k = max(min((int)floorf(u), n - 2), 0), k1 = min(k + 1, n - 1);
  AcqTap o;
  o.t = __fsub_rn(u, (float)k);
  o.lo = min((int)(((int64_t)(2 * k + 1) * C) / (2 * n)), C - 1);      // (always < C: the clamp costs nothing and cannot act)
  o.hi = min((int)(((int64_t)(2 * k1 + 1) * C) / (2 * n)), C - 1);
  return o;
}

__device__ __forceinline__ float acq_lerp(float a, float b, float t) { return __fadd_rn(a, __fmul_rn(t, __fsub_rn(b, a))); }

__global__ __launch_bounds__(256) void acq_gather_kernel(const AcqArgs a) {
  __shared__ AcqTap tap0[ACQ_T0];
  const cwf_acquire_sample& S = a.s[blockIdx.z];
  const int c = blockIdx.y, tid = threadIdx.x;
  if (!((S.lowres_mask >> c) & 1)) return;                    // (uniform over the workgroup)
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const AcqTile T = acq_tile(blockIdx.x, C1, C2);
  const int64_t V = (int64_t)C0 * C1 * C2;
  const float* src = a.src + (int64_t)blockIdx.z * a.src_bs + c * V;
  float* dst = a.dst + (int64_t)blockIdx.z * a.dst_bs + c * V;
  const int* n = S.lattice[c];
  const float* r = a.r[blockIdx.z][c];
  if (tid < ACQ_T0) tap0[tid] = acq_tap(min(T.b0 + tid, C0 - 1), C0, n[0], r[0]);
  __syncthreads();
  const int p1 = T.b1 + (tid >> 5), p2 = T.b2 + (tid & 31);
  if (!(p1 < C1 && p2 < C2)) return;                          // (no barrier follows)
  const AcqTap t1 = acq_tap(p1, C1, n[1], r[1]), t2 = acq_tap(p2, C2, n[2], r[2]);
  const int64_t o00 = (int64_t)t1.lo * C2 + t2.lo, o01 = (int64_t)t1.lo * C2 + t2.hi, o10 = (int64_t)t1.hi * C2 + t2.lo,
                o11 = (int64_t)t1.hi * C2 + t2.hi;
  const int64_t plane = (int64_t)C1 * C2;
#pragma unroll 2
  for (int j = 0; j < ACQ_T0; ++j) {
    const int p0 = T.b0 + j;
    if (p0 >= C0) break;
    const AcqTap t0 = tap0[j];
    const float* lo = src + t0.lo * plane;
    const float* hi = src + t0.hi * plane;
    const float l0 = acq_lerp(acq_lerp(lo[o00], lo[o01], t2.t), acq_lerp(lo[o10], lo[o11], t2.t), t1.t);
    const float l1 = acq_lerp(acq_lerp(hi[o00], hi[o01], t2.t), acq_lerp(hi[o10], hi[o11], t2.t), t1.t);
    dst[((int64_t)p0 * C1 + p1) * C2 + p2] = acq_lerp(l0, l1, t0.t);
  }
}

extern "C" int cwf_augment_acquisition(const struct cwf_acquire_sample* h_samples, int B, int C0, int C1, int C2, float* src,
                                       int64_t src_bstride, float* dst, int64_t dst_bstride, double* ws, int64_t ws_doubles,
                                       void* stream) {
  if (!h_samples || B <= 0 || C0 <= 0 || C1 <= 0 || C2 <= 0 || !src || !dst) return CWF_E_BADARG;
  const int64_t V = (int64_t)C0 * C1 * C2;
  if (V >= (int64_t(1) << 31)) return CWF_E_TOOLARGE;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)ws & 7)) return CWF_E_BADARG;
  if (src_bstride < 4 * V || dst_bstride < 4 * V) return CWF_E_BADARG;
  const int C[3] = {C0, C1, C2};
  bool any_contrast = false, any_lowres = false;
  for (int b = 0; b < B; ++b) {
    const cwf_acquire_sample& s = h_samples[b];
    if (s.bias_mask < 0 || s.bias_mask > 15 || s.contrast_mask < 0 || s.contrast_mask > 15 || s.lowres_mask < 0 || s.lowres_mask > 15)
      return CWF_E_BADARG;
    const int G[3] = {s.G0, s.G1, s.G2};
    for (int d = 0; d < 3; ++d)
      if (s.bias_mask && (G[d] < 4 || G[d] > ACQ_GMAX)) return CWF_E_BADARG;
    for (int c = 0; c < 4; ++c) {
      if (((s.bias_mask >> c) & 1) && (!s.bias[c] || ((uintptr_t)s.bias[c] & 3))) return CWF_E_BADARG;
      if (((s.contrast_mask >> c) & 1) && !(std::isfinite(s.factor[c]) && s.factor[c] > 0.f)) return CWF_E_BADARG;
      for (int d = 0; d < 3; ++d)
        if (((s.lowres_mask >> c) & 1) && (s.lattice[c][d] < 1 || s.lattice[c][d] > C[d])) return CWF_E_BADARG;
    }
    any_contrast = any_contrast || s.contrast_mask;
    any_lowres = any_lowres || s.lowres_mask;
  }
  const int64_t tiles = (int64_t)cdiv(C0, ACQ_T0) * cdiv(C1, ACQ_T1) * cdiv(C2, ACQ_T2);
  if (any_contrast && (!ws || ws_doubles < 12 * (int64_t)B * tiles)) return CWF_E_BADARG;
  const bool inplace = dst == src && dst_bstride == src_bstride;
  if (!inplace || any_lowres) {                               // the buffers must be disjoint
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + 4 * (uintptr_t)((B - 1) * src_bstride + 4 * V);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + 4 * (uintptr_t)((B - 1) * dst_bstride + 4 * V);
    if (s0 < d1 && d0 < s1) return CWF_E_BADARG;
  }
  AcqArgs a;
  a.src_bs = src_bstride; a.dst_bs = dst_bstride;
  a.C0 = C0; a.C1 = C1; a.C2 = C2; a.tiles = (int)tiles; a.inplace = inplace;
  hipStream_t st = cwf_stream(stream);
  for (int b0 = 0; b0 < B; b0 += ACQ_MAXS) {
    const int nb = std::min(ACQ_MAXS, B - b0);
    bool stats = false, point = false, gather = false;        // some channel for each of the three kernels
    for (int i = 0; i < ACQ_MAXS; ++i) {
      a.s[i] = i < nb ? h_samples[b0 + i] : cwf_acquire_sample{};
      cwf_acquire_sample& s = a.s[i];
      if (!s.bias_mask) s.G0 = s.G1 = s.G2 = 0;
      const int G[3] = {s.G0, s.G1, s.G2};
      for (int d = 0; d < 3; ++d) {
        a.k[i][d] = (s.bias_mask && C[d] > 1) ? (float)(G[d] - 3) / (float)(C[d] - 1) : 0.f;
        for (int c = 0; c < 4; ++c) a.r[i][c][d] = ((s.lowres_mask >> c) & 1) ? (float)s.lattice[c][d] / (float)C[d] : 0.f;
      }
      if (i >= nb) continue;
      stats = stats || s.contrast_mask;
      point = point || ((s.bias_mask | s.contrast_mask) || (!inplace && (15 & ~s.lowres_mask)));
      gather = gather || s.lowres_mask;
    }
    a.src = src + (int64_t)b0 * src_bstride;
    a.dst = dst + (int64_t)b0 * dst_bstride;
    a.ws = ws ? ws + 12 * (int64_t)b0 * tiles : nullptr;
    const dim3 grid((unsigned)tiles, 4, (unsigned)nb);
    if (stats) {
      hipLaunchKernelGGL(acq_stats_kernel, grid, dim3(256), 0, st, a);
      CWF_LAUNCH_CHECK();
    }
    if (point) {
      hipLaunchKernelGGL(acq_point_kernel, grid, dim3(256), 0, st, a);
      CWF_LAUNCH_CHECK();
    }
    if (gather) {
      hipLaunchKernelGGL(acq_gather_kernel, grid, dim3(256), 0, st, a);
      CWF_LAUNCH_CHECK();
    }
  }
  return 0;
}
