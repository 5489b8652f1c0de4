// N3 -- the intensity stage of the batch preparer (utils/data.py: Gaussian blur, additive noise, gamma; statement:
// include/cwf_hip.h cwf_augment_intensity).  It runs after a prepare kernel of prep.hip on the prepared crop x [B][4][C0][C1][C2].
//
// int_stage_kernel<BLUR>: one 256-thread workgroup per (tile, channel, sample); the two instantiations share a launch's channels
// between them (a workgroup whose channel belongs to the other one returns at once), so that the channels without a blur do not
// carry the blur's LDS and run at full occupancy.
//   blurred channel: the tile of 10 x 10 x 32 output voxels plus its 3-voxel halo, 16 x 16 x 38 voxels read with clamped (replicate)
//     indices, is staged in LDS (rows padded to 39 words: 39,936 B, so four workgroups share a CU's 160 KiB).  The three passes run
//     in place.  A thread owns a whole line of the pass's axis -- it reads the line into registers and writes the results over the
//     line's head -- so a pass needs no second buffer and only the barriers between passes.  Axis 2: 16 x 16 = 256 rows, one per
//     thread (row stride 39 words: the 32 lanes of an LDS lane group fall on 32 banks).  Axis 1: 16 x 32 = 512 columns, two per
//     thread; axis 0: 10 x 32 = 320 columns (lanes along axis 2: conflict-free), whose ten results get the noise and go to global
//     memory with one dword store per lane, 128 B per tile row.  The channel is read once (plus the halo, from L2) and written once.
//     A pass of a line at a clamped index equals the pass of the line it is clamped to, so clamping the staged indices gives the
//     replicate border of every pass.
//   other channels: the tile's voxels are copied (or left alone when the stage runs in place), with the noise where it is on, four
//     loads in flight per thread.
//   Where gamma is on the workgroup also writes the minimum and maximum of what it stored to ws (fminf / fmaxf ignore NaN; min and
//   max do not depend on the order they are taken in).
// int_gamma_kernel: every workgroup of a channel reduces that channel's partials (at most a few hundred pairs, from L2) and maps
//   its share of the voxels in place.
// No store is wider than a dword, so any 4-byte-aligned x with any sample stride takes the same path.
// This file is compiled with -ffp-contract=off.
#include "common.h"

#define INT_MAXS 8                          // samples per launch
#define INT_R 3                             // blur radius
#define INT_T0 CWF_INTENSITY_T0
#define INT_T1 CWF_INTENSITY_T1
#define INT_T2 CWF_INTENSITY_T2
#define INT_H0 (INT_T0 + 2 * INT_R)
#define INT_H1 (INT_T1 + 2 * INT_R)
#define INT_H2 (INT_T2 + 2 * INT_R)
#define INT_ROW (INT_H2 + 1)                // odd row stride (words)
#define INT_FILL 19                         // halo voxels a thread fetches before it writes them to LDS
#define INT_GAMMA_BLOCKS 256                // workgroups per channel of the gamma launch, at most
static_assert(INT_H0 * INT_H1 == 256, "axis-2 pass: one halo row per thread");
static_assert((INT_H0 * INT_T2) % 256 == 0 && INT_T2 == 32, "axis-1 pass: whole rounds of columns, a tile row per half wave");
static_assert(INT_H0 * INT_H1 * INT_ROW * 4 <= 40960, "four workgroups per CU");
static_assert((INT_H0 * INT_H1 * INT_H2) % (256 * INT_FILL) == 0, "the fill: whole rounds");

struct IntArgs {
  cwf_intensity_sample s[INT_MAXS];
  const float* src;
  float* dst;
  float* ws;                                // partials of this launch's first sample
  int64_t src_bs, dst_bs;                   // sample strides (elements)
  int C0, C1, C2, tiles, inplace;
};
static_assert(sizeof(IntArgs) <= 4096, "the samples travel by value in the kernel-argument block");

// (((((w0*a0 + w1*a1) + w2*a2) + w3*a3) + w4*a4) + w5*a5) + w6*a6
__device__ __forceinline__ float int_tap7(const float (&w)[7], const float* a) {
  float y = __fadd_rn(__fmul_rn(w[0], a[0]), __fmul_rn(w[1], a[1]));
#pragma unroll
  for (int j = 2; j < 7; ++j) y = __fadd_rn(y, __fmul_rn(w[j], a[j]));
  return y;
}

// utils.synthetic._splitmix64
__device__ __forceinline__ uint64_t int_splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// x + float(s) * amp, s the sum of the four 16-bit fields of the hash of element ctr, centred
__device__ __forceinline__ float int_noise(float x, uint64_t key, uint64_t ctr, float amp) {
  const uint64_t h = int_splitmix64(key + ctr);
  const int s = (int)(h & 0xFFFFu) + (int)((h >> 16) & 0xFFFFu) + (int)((h >> 32) & 0xFFFFu) + (int)(h >> 48) - 131070;
  return __fadd_rn(x, __fmul_rn((float)s, amp));
}

__device__ __forceinline__ int int_clamp(int p, int C) { return min(max(p, 0), C - 1); }

// minimum and maximum over the workgroup; the result is valid in every thread
__device__ __forceinline__ void int_block_minmax(float& mn, float& mx, float (&red)[2][4]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mn;
    red[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
}

template <bool BLUR>
__global__ __launch_bounds__(256) void int_stage_kernel(const IntArgs a) {
  __shared__ float red[2][4];
  const cwf_intensity_sample& S = a.s[blockIdx.z];
  const int c = blockIdx.y, tid = threadIdx.x;
  const bool blur = (S.blur >> c) & 1, noise = (S.noise >> c) & 1, gam = (S.gam >> c) & 1;
  if (blur != BLUR || (!blur && !noise && !gam && a.inplace)) return;       // (uniform over the workgroup)
  const int C0 = a.C0, C1 = a.C1, C2 = a.C2;
  const int n2 = (C2 + INT_T2 - 1) / INT_T2, n1 = (C1 + INT_T1 - 1) / INT_T1;
  const int t = blockIdx.x;
  const int b2 = (t % n2) * INT_T2, b1 = ((t / n2) % n1) * INT_T1, b0 = (t / (n2 * n1)) * INT_T0;
  const int64_t V = (int64_t)C0 * C1 * C2;
  const float* src = a.src + (int64_t)blockIdx.z * a.src_bs + c * V;
  float* dst = a.dst + (int64_t)blockIdx.z * a.dst_bs + c * V;
  const float amp = S.amp[c];
  const uint64_t key = S.key, cV = (uint64_t)(c * V);
  float mn = INFINITY, mx = -INFINITY;

  if constexpr (BLUR) {
    __shared__ float A[INT_H0][INT_H1][INT_ROW];
    float w[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) w[j] = S.taps[c][j];
    // the halo tile, every index clamped into the crop: 38 voxels per thread, fetched 19 at a time before any is written to LDS
    // (one load in flight per thread left the fill waiting out 38 memory latencies in turn)
#pragma unroll 1
    for (int i0 = tid; i0 < INT_H0 * INT_H1 * INT_H2; i0 += 256 * INT_FILL) {
      float v[INT_FILL];
#pragma unroll
      for (int k = 0; k < INT_FILL; ++k) {
        const int i = i0 + 256 * k;
        const int h2 = i % INT_H2, h1 = (i / INT_H2) % INT_H1, h0 = i / (INT_H2 * INT_H1);
        const int p0 = int_clamp(b0 + h0 - INT_R, C0), p1 = int_clamp(b1 + h1 - INT_R, C1), p2 = int_clamp(b2 + h2 - INT_R, C2);
        v[k] = src[((int64_t)p0 * C1 + p1) * C2 + p2];
      }
#pragma unroll
      for (int k = 0; k < INT_FILL; ++k) {
        const int i = i0 + 256 * k;
        A[i / (INT_H2 * INT_H1)][(i / INT_H2) % INT_H1][i % INT_H2] = v[k];
      }
    }
    __syncthreads();
    {   // axis 2: row tid
      float* row = &A[tid / INT_H1][tid % INT_H1][0];
      float v[INT_H2];
#pragma unroll
      for (int j = 0; j < INT_H2; ++j) v[j] = row[j];
#pragma unroll
      for (int j = 0; j < INT_T2; ++j) row[j] = int_tap7(w, v + j);
    }
    __syncthreads();
    // axis 1: column (h0, p2)
#pragma unroll 1
    for (int k = 0; k < INT_H0 * INT_T2 / 256; ++k) {
      const int q = tid + 256 * k, e = q % INT_T2, h0 = q / INT_T2;
      float v[INT_H1];
#pragma unroll
      for (int j = 0; j < INT_H1; ++j) v[j] = A[h0][j][e];
#pragma unroll
      for (int j = 0; j < INT_T1; ++j) A[h0][j][e] = int_tap7(w, v + j);
    }
    __syncthreads();
    // axis 0: column (p1, p2); noise; store
#pragma unroll 1
    for (int q = tid; q < INT_T1 * INT_T2; q += 256) {
      const int e = q % INT_T2, j1 = q / INT_T2;
      const int p1 = b1 + j1, p2 = b2 + e;
      if (p1 >= C1 || p2 >= C2) continue;
      float v[INT_H0];
#pragma unroll
      for (int j = 0; j < INT_H0; ++j) v[j] = A[j][j1][e];
#pragma unroll
      for (int j = 0; j < INT_T0; ++j) {
        const int p0 = b0 + j;
        if (p0 >= C0) break;
        const int64_t at = ((int64_t)p0 * C1 + p1) * C2 + p2;
        float y = int_tap7(w, v + j);
        if (noise) y = int_noise(y, key, cV + (uint64_t)at, amp);
        dst[at] = y;
        mn = fminf(mn, y);
        mx = fmaxf(mx, y);
      }
    }
  } else {
    const bool store = noise || !a.inplace;
#pragma unroll 1
    for (int i0 = tid; i0 < INT_T0 * INT_T1 * INT_T2; i0 += 1024) {
      int64_t at[4];
      float y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + 256 * k;
        const int p2 = b2 + i % INT_T2, p1 = b1 + (i / INT_T2) % INT_T1, p0 = b0 + i / (INT_T2 * INT_T1);
        at[k] = (i < INT_T0 * INT_T1 * INT_T2 && p0 < C0 && p1 < C1 && p2 < C2) ? ((int64_t)p0 * C1 + p1) * C2 + p2 : -1;
        y[k] = at[k] >= 0 ? src[at[k]] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (at[k] < 0) continue;
        if (noise) y[k] = int_noise(y[k], key, cV + (uint64_t)at[k], amp);
        if (store) dst[at[k]] = y[k];
        mn = fminf(mn, y[k]);
        mx = fmaxf(mx, y[k]);
      }
    }
  }
  if (gam) {
    int_block_minmax(mn, mx, red);
    if (tid == 0) {
      float* part = a.ws + (((int64_t)blockIdx.z * 4 + c) * a.tiles + t) * 2;
      part[0] = mn;
      part[1] = mx;
    }
  }
}

__global__ __launch_bounds__(256) void int_gamma_kernel(const IntArgs a) {
  __shared__ float red[2][4];
  const cwf_intensity_sample& S = a.s[blockIdx.z];
  const int c = blockIdx.y;
  if (!((S.gam >> c) & 1)) return;
  const float* part = a.ws + ((int64_t)blockIdx.z * 4 + c) * a.tiles * 2;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < a.tiles; i += 256) {
    mn = fminf(mn, part[2 * i]);
    mx = fmaxf(mx, part[2 * i + 1]);
  }
  int_block_minmax(mn, mx, red);
  const float r = __fsub_rn(mx, mn);
  if (!(isfinite(r) && r > 0.f)) return;
  const float g = S.gamma[c];
  const int64_t V = (int64_t)a.C0 * a.C1 * a.C2;
  float* x = a.dst + (int64_t)blockIdx.z * a.dst_bs + c * V;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const float u = __fsub_rn(x[v], mn) / r;
    x[v] = __fadd_rn(__fmul_rn(powf(u, g), r), mn);
  }
}

extern "C" int cwf_augment_intensity(const struct cwf_intensity_sample* h_samples, int B, int C0, int C1, int C2, const float* src,
                                     int64_t src_bstride, float* dst, int64_t dst_bstride, float* ws, int64_t ws_floats,
                                     void* stream) {
  if (!h_samples || B <= 0 || C0 <= 0 || C1 <= 0 || C2 <= 0 || !src || !dst) return CWF_E_BADARG;
  const int64_t V = (int64_t)C0 * C1 * C2;
  if (V >= (int64_t(1) << 31)) return CWF_E_TOOLARGE;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)ws & 3)) return CWF_E_BADARG;
  if (src_bstride < 4 * V || dst_bstride < 4 * V) return CWF_E_BADARG;
  bool any_blur = false, any_gamma = false;
  for (int b = 0; b < B; ++b) {
    const cwf_intensity_sample& s = h_samples[b];
    if (s.blur < 0 || s.blur > 15 || s.noise < 0 || s.noise > 15 || s.gam < 0 || s.gam > 15) return CWF_E_BADARG;
    for (int c = 0; c < 4; ++c) {
      for (int j = 0; j < 7; ++j)
        if (!std::isfinite(s.taps[c][j])) return CWF_E_BADARG;
      if (!std::isfinite(s.amp[c]) || s.amp[c] < 0.f) return CWF_E_BADARG;
      if (((s.gam >> c) & 1) && !(std::isfinite(s.gamma[c]) && s.gamma[c] > 0.f)) return CWF_E_BADARG;
    }
    any_blur = any_blur || s.blur;
    any_gamma = any_gamma || s.gam;
  }
  const int64_t tiles = (int64_t)cdiv(C0, INT_T0) * cdiv(C1, INT_T1) * cdiv(C2, INT_T2);
  if (any_gamma && (!ws || ws_floats < 8 * (int64_t)B * tiles)) return CWF_E_BADARG;
  const bool inplace = (const float*)dst == src && dst_bstride == src_bstride;
  if (!inplace || any_blur) {                                 // the buffers must be disjoint
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + 4 * (uintptr_t)((B - 1) * src_bstride + 4 * V);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + 4 * (uintptr_t)((B - 1) * dst_bstride + 4 * V);
    if (s0 < d1 && d0 < s1) return CWF_E_BADARG;
  }
  IntArgs a;
  a.src_bs = src_bstride; a.dst_bs = dst_bstride;
  a.C0 = C0; a.C1 = C1; a.C2 = C2; a.tiles = (int)tiles; a.inplace = inplace;
  const int gblocks = (int)std::min<int64_t>(cdiv64(V, 256 * 8), INT_GAMMA_BLOCKS);
  hipStream_t st = cwf_stream(stream);
  for (int b0 = 0; b0 < B; b0 += INT_MAXS) {
    const int nb = std::min(INT_MAXS, B - b0);
    bool blur = false, point = false, gam = false;            // some channel for int_stage_kernel<true>, for <false>, for gamma
    for (int i = 0; i < INT_MAXS; ++i) {
      a.s[i] = i < nb ? h_samples[b0 + i] : cwf_intensity_sample{};
      if (i >= nb) continue;
      blur = blur || a.s[i].blur;
      point = point || ((inplace ? a.s[i].noise | a.s[i].gam : 15) & ~a.s[i].blur);
      gam = gam || a.s[i].gam;
    }
    a.src = src + (int64_t)b0 * src_bstride;
    a.dst = dst + (int64_t)b0 * dst_bstride;
    a.ws = ws ? ws + 8 * (int64_t)b0 * tiles : nullptr;
    if (blur) {
      hipLaunchKernelGGL(int_stage_kernel<true>, dim3((unsigned)tiles, 4, (unsigned)nb), dim3(256), 0, st, a);
      CWF_LAUNCH_CHECK();
    }
    if (point) {
      hipLaunchKernelGGL(int_stage_kernel<false>, dim3((unsigned)tiles, 4, (unsigned)nb), dim3(256), 0, st, a);
      CWF_LAUNCH_CHECK();
    }
    if (gam) {
      hipLaunchKernelGGL(int_gamma_kernel, dim3((unsigned)gblocks, 4, (unsigned)nb), dim3(256), 0, st, a);
      CWF_LAUNCH_CHECK();
    }
  }
  return 0;
}
