// N5 -- sliding-window inference over volumes of any size (predict_overlap.sliding_window_inference): cut the windows of a chunk
// out of the NCDHW volume into the model's channels-last input (cwf_window_gather), add the importance-weighted window outputs into
// a channels-last fp32 accumulator (cwf_window_blend), divide by the per-voxel weight sum into NCDHW (cwf_window_finalize).
// cwf_window_gather_box / cwf_window_finalize_box lay the grid over a sub-box of the volume (sliding_window_inference(crop_nonzero=True)):
// the gather reads the whole volume at box.lo + the box coordinate, the finalize visits every voxel of the whole volume and writes the
// background one-hot outside the box; the plain entry points are these with the box the whole volume.
// One thread per voxel, 16 bytes (4 classes) per voxel access.  Built with -ffp-contract=off: every weight product, product with a
// probability and addition is rounded on its own, as tests/sliding_window_ref.py's bound counts them.
#include "common.h"

// wt(l0, l1, l2) = fp32(fp32(g0[l0] * g1[l1]) * g2[l2]); g = g0[r0] g1[r1] g2[r2] back to back
__device__ __forceinline__ float window_weight(const float* __restrict__ g, const cwf_window_grid& gr, int l0, int l1, int l2) {
  return (g[l0] * g[gr.r[0] + l1]) * g[gr.r[0] + gr.r[1] + l2];
}

// blockIdx.y = j * B + b (window w0 + j, sample b); x over the window's r0 * r1 * r2 voxels.  The grid is laid over the box bx of the
// volume x: window coordinates a are box coordinates, bx.lo + a the voxel read.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ x, float* __restrict__ win, const cwf_window_grid gr,
                                                            const cwf_window_box bx, int w0, int nvw) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nvw) return;
  const int jb = blockIdx.y;
  const int b = jb % gr.B, w = w0 + jb / gr.B;
  const int i2 = w % gr.n[2], i1 = (w / gr.n[2]) % gr.n[1], i0 = w / (gr.n[2] * gr.n[1]);
  const int l2 = l % gr.r[2], l1 = (l / gr.r[2]) % gr.r[1], l0 = l / (gr.r[2] * gr.r[1]);
  const int a0 = gr.start[0][i0] + l0, a1 = gr.start[1][i1] + l1, a2 = gr.start[2][i2] + l2;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if ((unsigned)a0 < (unsigned)gr.S[0] && (unsigned)a1 < (unsigned)gr.S[1] && (unsigned)a2 < (unsigned)gr.S[2]) {
    const int64_t plane = (int64_t)bx.full[0] * bx.full[1] * bx.full[2];
    const float* src = x + (int64_t)b * 4 * plane + ((int64_t)(bx.lo[0] + a0) * bx.full[1] + (bx.lo[1] + a1)) * bx.full[2] + (bx.lo[2] + a2);
    v[0] = src[0]; v[1] = src[plane]; v[2] = src[2 * plane]; v[3] = src[3 * plane];
  }
  *reinterpret_cast<f32x4*>(win + ((int64_t)jb * nvw + l) * 4) = v;
}

// blockIdx.y = b; x over the S0 * S1 * S2 voxels.  Windows are visited in window order (i0, i1, i2 nested, axis 0 slowest).
__global__ __launch_bounds__(256) void window_blend_kernel(const float* __restrict__ probs, const float* __restrict__ g, float* __restrict__ acc,
                                                           const cwf_window_grid gr, int w0, int count, int accumulate, int nv) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int b = blockIdx.y;
  const int a2 = v % gr.S[2], a1 = (v / gr.S[2]) % gr.S[1], a0 = v / (gr.S[2] * gr.S[1]);
  f32x4* dst = reinterpret_cast<f32x4*>(acc) + (int64_t)b * nv + v;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (accumulate) s = *dst;
  const int64_t nvw = (int64_t)gr.r[0] * gr.r[1] * gr.r[2];
  for (int i0 = 0; i0 < gr.n[0]; ++i0) {
    const int l0 = a0 - gr.start[0][i0];
    if ((unsigned)l0 >= (unsigned)gr.r[0]) continue;
    for (int i1 = 0; i1 < gr.n[1]; ++i1) {
      const int l1 = a1 - gr.start[1][i1];
      if ((unsigned)l1 >= (unsigned)gr.r[1]) continue;
      for (int i2 = 0; i2 < gr.n[2]; ++i2) {
        const int l2 = a2 - gr.start[2][i2];
        if ((unsigned)l2 >= (unsigned)gr.r[2]) continue;
        const int j = (i0 * gr.n[1] + i1) * gr.n[2] + i2 - w0;
        if ((unsigned)j >= (unsigned)count) continue;
        const float wt = window_weight(g, gr, l0, l1, l2);
        const f32x4 p = *reinterpret_cast<const f32x4*>(probs + (((int64_t)j * gr.B + b) * nvw + ((int64_t)l0 * gr.r[1] + l1) * gr.r[2] + l2) * 4);
        s[0] = s[0] + wt * p[0]; s[1] = s[1] + wt * p[1]; s[2] = s[2] + wt * p[2]; s[3] = s[3] + wt * p[3];
      }
    }
  }
  *dst = s;
}

// blockIdx.y = b; x over the nf voxels of the whole volume; acc holds the nv voxels of the box bx
__global__ __launch_bounds__(256) void window_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ g, float* __restrict__ y,
                                                              const cwf_window_grid gr, const cwf_window_box bx, int nv, int nf) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int b = blockIdx.y;
  const int a2 = f % bx.full[2] - bx.lo[2], a1 = (f / bx.full[2]) % bx.full[1] - bx.lo[1], a0 = f / (bx.full[2] * bx.full[1]) - bx.lo[0];
  float* dst = y + (int64_t)b * 4 * nf + f;
  if ((unsigned)a0 >= (unsigned)gr.S[0] || (unsigned)a1 >= (unsigned)gr.S[1] || (unsigned)a2 >= (unsigned)gr.S[2]) {   // outside the box
    dst[0] = 1.f; dst[nf] = 0.f; dst[2 * (int64_t)nf] = 0.f; dst[3 * (int64_t)nf] = 0.f;
    return;
  }
  float ws = 0.f;
  for (int i0 = 0; i0 < gr.n[0]; ++i0) {
    const int l0 = a0 - gr.start[0][i0];
    if ((unsigned)l0 >= (unsigned)gr.r[0]) continue;
    for (int i1 = 0; i1 < gr.n[1]; ++i1) {
      const int l1 = a1 - gr.start[1][i1];
      if ((unsigned)l1 >= (unsigned)gr.r[1]) continue;
      for (int i2 = 0; i2 < gr.n[2]; ++i2) {
        const int l2 = a2 - gr.start[2][i2];
        if ((unsigned)l2 >= (unsigned)gr.r[2]) continue;
        ws = ws + window_weight(g, gr, l0, l1, l2);
      }
    }
  }
  const f32x4 s = reinterpret_cast<const f32x4*>(acc)[(int64_t)b * nv + ((int64_t)a0 * gr.S[1] + a1) * gr.S[2] + a2];
  dst[0] = s[0] / ws; dst[nf] = s[1] / ws; dst[2 * (int64_t)nf] = s[2] / ws; dst[3 * (int64_t)nf] = s[3] / ws;
}

// A grid every kernel here can index: positive sizes, 1..CWF_WINDOW_MAX_STARTS windows per axis that each overlap the volume, and
// voxel counts (volume, window) below 2^31.
static int check_grid(const cwf_window_grid* g) {
  if (!g || g->B <= 0) return CWF_E_BADARG;
  int64_t nv = 1, nvw = 1;
  for (int a = 0; a < 3; ++a) {
    if (g->S[a] <= 0 || g->r[a] <= 0 || g->n[a] <= 0 || g->n[a] > CWF_WINDOW_MAX_STARTS) return CWF_E_BADARG;
    for (int i = 0; i < g->n[a]; ++i)
      if (g->start[a][i] <= -g->r[a] || g->start[a][i] >= g->S[a]) return CWF_E_BADARG;      // entirely outside the volume
    nv *= g->S[a]; nvw *= g->r[a];
  }
  if (nv >= ((int64_t)1 << 31) || nvw >= ((int64_t)1 << 31)) return CWF_E_TOOLARGE;
  return 0;
}

static int check_chunk(const cwf_window_grid* g, int w0, int count) {
  const int64_t nw = (int64_t)g->n[0] * g->n[1] * g->n[2];
  if (w0 < 0 || count <= 0 || w0 + (int64_t)count > nw) return CWF_E_BADARG;
  return 0;
}

// A box the grid's volume fits: inside a whole volume of positive extents and fewer than 2^31 voxels (after check_grid).
static int check_box(const cwf_window_grid* g, const cwf_window_box* bx) {
  if (!bx) return CWF_E_BADARG;
  int64_t nf = 1;
  for (int a = 0; a < 3; ++a) {
    if (bx->full[a] <= 0 || bx->lo[a] < 0 || (int64_t)bx->lo[a] + g->S[a] > bx->full[a]) return CWF_E_BADARG;
    nf *= bx->full[a];
  }
  if (nf >= ((int64_t)1 << 31)) return CWF_E_TOOLARGE;
  return 0;
}

// the box that is the grid's whole volume (a null grid is refused by check_grid before the box is looked at)
static cwf_window_box whole_box(const cwf_window_grid* g) {
  cwf_window_box bx = {};
  for (int a = 0; g && a < 3; ++a) bx.full[a] = g->S[a];
  return bx;
}

extern "C" int cwf_window_gather_box(const float* x, float* windows, const cwf_window_grid* grid, const cwf_window_box* box, int w0, int count,
                                     void* stream) {
  if (!x || !windows || ((uintptr_t)windows & 15) || ((uintptr_t)x & 3)) return CWF_E_BADARG;
  int rc = check_grid(grid);
  if (rc || (rc = check_chunk(grid, w0, count)) || (rc = check_box(grid, box))) return rc;
  if ((int64_t)count * grid->B > 65535) return CWF_E_TOOLARGE;
  const int nvw = grid->r[0] * grid->r[1] * grid->r[2];
  hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)cdiv(nvw, 256), (unsigned)(count * grid->B)), dim3(256), 0, cwf_stream(stream),
                     x, windows, *grid, *box, w0, nvw);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_window_gather(const float* x, float* windows, const cwf_window_grid* grid, int w0, int count, void* stream) {
  const cwf_window_box bx = whole_box(grid);
  return cwf_window_gather_box(x, windows, grid, &bx, w0, count, stream);
}

extern "C" int cwf_window_blend(const float* probs, const float* weights, float* acc, const cwf_window_grid* grid, int w0, int count,
                                int accumulate, void* stream) {
  if (!probs || !weights || !acc || ((uintptr_t)probs & 15) || ((uintptr_t)acc & 15) || ((uintptr_t)weights & 3)) return CWF_E_BADARG;
  int rc = check_grid(grid);
  if (rc || (rc = check_chunk(grid, w0, count))) return rc;
  if (grid->B > 65535) return CWF_E_TOOLARGE;
  const int nv = grid->S[0] * grid->S[1] * grid->S[2];
  hipLaunchKernelGGL(window_blend_kernel, dim3((unsigned)cdiv(nv, 256), (unsigned)grid->B), dim3(256), 0, cwf_stream(stream),
                     probs, weights, acc, *grid, w0, count, accumulate ? 1 : 0, nv);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_window_finalize_box(const float* acc, const float* weights, float* y, const cwf_window_grid* grid, const cwf_window_box* box,
                                       void* stream) {
  if (!acc || !weights || !y || ((uintptr_t)acc & 15) || ((uintptr_t)weights & 3) || ((uintptr_t)y & 3)) return CWF_E_BADARG;
  int rc = check_grid(grid);
  if (rc || (rc = check_box(grid, box))) return rc;
  if (grid->B > 65535) return CWF_E_TOOLARGE;
  const int nv = grid->S[0] * grid->S[1] * grid->S[2], nf = box->full[0] * box->full[1] * box->full[2];
  hipLaunchKernelGGL(window_finalize_kernel, dim3((unsigned)cdiv(nf, 256), (unsigned)grid->B), dim3(256), 0, cwf_stream(stream),
                     acc, weights, y, *grid, *box, nv, nf);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_window_finalize(const float* acc, const float* weights, float* y, const cwf_window_grid* grid, void* stream) {
  const cwf_window_box bx = whole_box(grid);
  return cwf_window_finalize_box(acc, weights, y, grid, &bx, stream);
}
