// N7 -- lesion-wise Dice and HD95 of region-bit masks (the BraTS 2023 ranking metrics; predict_overlap.lesionwise_metrics states the
// definition).  For every sample b and region r of a prediction and a ground truth:
//   pred_cc  = 26-neighbour components of pred                                  (cwf_components)
//   gt_dil   = gt dilated `dilation` times with the 18-neighbour footprint      (cwf_dilate_bits; all regions of a byte at once)
//   dil_cc   = 26-neighbour components of gt_dil; lesion g = gt & (dil_cc == g) (cwf_components)
// and then, all integer:
//   lw_clear_kernel   the touch words of the components that exist are zeroed (not the whole [cap] extent)
//   lw_touch_kernel   one pass over the voxels: touch[p] |= 1 << (g - 1) for every voxel of predicted component p inside dilated
//                     component g (a 64-bit word per predicted component -- hence the cap of 64 lesions), and per lesion gt_vol and
//                     inter = |pred & lesion| (a voxel of gt & pred always lies in a touching component); counts are summed per wave,
//                     then per workgroup in LDS, one global atomic per workgroup and lesion
//   lw_comp_kernel    one pass over the predicted components: pred_vol and the number of touching components per lesion from the
//                     components' sizes and touch words; components whose word is zero are the false positives
//   lw_pack_kernel    per region and group of eight lesions: byte a = the touch bits of the voxel's component for the group, byte b =
//                     the lesion's own bit, so that cwf_hausdorff (R = 8) scores eight (pred_g, lesion g) pairs per call
//   lw_final_kernel   one workgroup per (sample, region): per-lesion Dice and HD95, the sums in increasing lesion order in float64
// Every accumulation is an integer add or a bitwise OR, so no output depends on the order in which atomics land.  No kernel waits on
// another workgroup.  The host reads the lesion counts back once (B * R ints) to size the HD95 calls.  This file is compiled with
// -ffp-contract=off: the aggregate is formed operation by operation as the float64 restatement forms it.
//
// cwf_lesionwise_ex adds the lesion-wise normalised surface Dice at T <= 4 tolerances: it calls cwf_surface_metrics where
// cwf_lesionwise calls cwf_hausdorff (same masks, eight lesions per call), takes nsd_g of (pred_g, lesion g) from it -- 0 for a lesion
// nothing touches -- and lw_final_kernel forms lw_nsd[t] = (sum over kept lesions of nsd_g[t]) / (kept + FP) in increasing g, 1 if
// kept + FP == 0, as it forms lw_dice.  Every nsd_g is a ratio of two integers, so lw_nsd does not depend on the order of atomics either.
#include <algorithm>
#include <vector>
#include "common.h"

#define LW_MAX 64             // lesions per (sample, region) on the device: one bit of a touch word each
#define LW_MAX_TAU 4          // tolerances of cwf_lesionwise_ex (cwf_surface_metrics' limit)

// out = in dilated once; one thread per voxel, one sample per blockIdx.y.  Out-of-volume voxels are unset.
__global__ __launch_bounds__(256) void lw_dilate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int D0, int D1, int D2,
                                                        int conn) {
  const int64_t plane = (int64_t)D1 * D2, V = (int64_t)D0 * plane;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const uint8_t* s = in + (int64_t)blockIdx.y * V;
  const int i2 = (int)(v % D2);
  const int64_t t = v / D2;
  const int i1 = (int)(t % D1), i0 = (int)(t / D1);
  unsigned m = 0;
#pragma unroll
  for (int d0 = -1; d0 <= 1; ++d0)
#pragma unroll
    for (int d1 = -1; d1 <= 1; ++d1) {
      const int nz = (d0 != 0) + (d1 != 0);
      if (nz > conn) continue;
      const int j0 = i0 + d0, j1 = i1 + d1;
      if (j0 < 0 || j0 >= D0 || j1 < 0 || j1 >= D1) continue;
      const uint8_t* row = s + (int64_t)j0 * plane + (int64_t)j1 * D2;
      m |= row[i2];
      if (nz + 1 <= conn) {
        if (i2 > 0) m |= row[i2 - 1];
        if (i2 + 1 < D2) m |= row[i2 + 1];
      }
    }
  out[(int64_t)blockIdx.y * V + v] = (uint8_t)m;
}

extern "C" int cwf_dilate_bits(const uint8_t* bits, uint8_t* out, int B, int D0, int D1, int D2, int connectivity, int iterations, void* ws,
                               int64_t ws_bytes, void* stream) {
  if (B <= 0 || B > 65535 || D0 <= 0 || D1 <= 0 || D2 <= 0) return CWF_E_BADARG;
  const int64_t V = (int64_t)D0 * D1 * D2;
  if (V >= ((int64_t)1 << 31)) return CWF_E_TOOLARGE;
  if (!bits || !out || bits == out || connectivity < 1 || connectivity > 3 || iterations < 0 || iterations > 8) return CWF_E_BADARG;
  if (iterations >= 2 && (!ws || ws == (void*)bits || ws == (void*)out)) return CWF_E_BADARG;
  if (iterations >= 2 && ws_bytes < (int64_t)B * V) return CWF_E_TOOLARGE;
  hipStream_t st = cwf_stream(stream);
  if (iterations == 0) {
    if (hipMemcpyAsync(out, bits, (size_t)B * V, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipErrorInvalidValue;
    return 0;
  }
  const uint8_t* src = bits;
  for (int i = 0; i < iterations; ++i) {                        // ping-pong so that the last pass lands in out
    uint8_t* dst = ((iterations - 1 - i) & 1) ? (uint8_t*)ws : out;
    hipLaunchKernelGGL(lw_dilate_kernel, dim3((unsigned)cdiv64(V, 256), B), dim3(256), 0, st, src, dst, D0, D1, D2, connectivity);
    CWF_LAUNCH_CHECK();
    src = dst;
  }
  return 0;
}

// acc[b][r][LW_MAX][4] = gt_vol, pred_vol, inter, touching components; this pass adds gt_vol and inter.  One (sample, region) per
// blockIdx.y; the trip count is the same for every lane (ballots).  An entry with more than LW_MAX lesions is left alone.
__global__ __launch_bounds__(256) void lw_touch_kernel(const uint8_t* __restrict__ gt, const int* __restrict__ plab, const int* __restrict__ dlab,
                                                       const int* __restrict__ dcount, unsigned long long* __restrict__ touch,
                                                       unsigned long long* __restrict__ acc, int R, int64_t V, int64_t cap) {
  __shared__ unsigned int h[LW_MAX * 2];
  const int br = blockIdx.y, b = br / R, r = br % R;
  if (dcount[br] > LW_MAX) return;                              // the whole grid row leaves
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < LW_MAX * 2) h[tid] = 0;
  __syncthreads();
  const uint8_t* gs = gt + (int64_t)b * V;
  const int* pl = plab + (int64_t)br * V;
  const int* dl = dlab + (int64_t)br * V;
  unsigned long long* tw = touch + (int64_t)br * cap;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < V; base += (int64_t)gridDim.x * 256) {
    const int64_t v = base + tid;
    const int g = v < V ? dl[v] : 0;                            // 1..LW_MAX inside a dilated component
    const int p = g > 0 ? pl[v] : 0;
    const bool ing = g > 0 && ((gs[v] >> r) & 1);
    const bool hit = g > 0 && p > 0;
    const unsigned long long mh = __ballot(hit);
    if (mh) {                                                   // wave-uniform; lanes that repeat the first lane's (p, g) stay out
      const int first = __ffsll((long long)mh) - 1;
      const int p0 = __shfl(p, first, 64), g0 = __shfl(g, first, 64);
      if (hit && (lane == first || p != p0 || g != g0)) {
        const unsigned long long bit = 1ull << (g - 1);
        if (!(__hip_atomic_load(tw + p - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(tw + p - 1, bit);
      }
    }
    const unsigned long long mg = __ballot(ing);
    if (mg) {
      const int first = __ffsll((long long)mg) - 1;
      const int g0 = __shfl(g, first, 64);
      const bool same = ing && g == g0;
      const unsigned long long ms = __ballot(same), mi = __ballot(same && p > 0);
      if (lane == first) {
        atomicAdd(&h[(g0 - 1) * 2], (unsigned)__popcll(ms));
        if (mi) atomicAdd(&h[(g0 - 1) * 2 + 1], (unsigned)__popcll(mi));
      } else if (ing && !same) {
        atomicAdd(&h[(g - 1) * 2], 1u);
        if (p > 0) atomicAdd(&h[(g - 1) * 2 + 1], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < LW_MAX * 2 && h[tid]) atomicAdd(acc + ((int64_t)br * LW_MAX + (tid >> 1)) * 4 + ((tid & 1) ? 2 : 0), (unsigned long long)h[tid]);
}

// touch words of the P components that exist <- 0 (the region held the second labelling's sizes); the words past P are never read
__global__ __launch_bounds__(256) void lw_clear_kernel(unsigned long long* __restrict__ touch, const int* __restrict__ pcount, int64_t cap) {
  const int64_t P = pcount[blockIdx.y];
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P && p < cap; p += (int64_t)gridDim.x * 256) touch[(int64_t)blockIdx.y * cap + p] = 0;
}

// pred_vol and the touching-component count per lesion, and the false positives fp[b][r], from the touch words and sizes of the
// P predicted components.  The sizes of distinct components add up to at most V < 2^31, so the LDS counters are 32-bit.
__global__ __launch_bounds__(256) void lw_comp_kernel(const unsigned long long* __restrict__ touch, const int* __restrict__ psizes,
                                                      const int* __restrict__ pcount, const int* __restrict__ dcount,
                                                      unsigned long long* __restrict__ acc, unsigned long long* __restrict__ fp, int64_t cap) {
  __shared__ unsigned int h[LW_MAX * 2];
  const int br = blockIdx.y, tid = threadIdx.x;
  if (dcount[br] > LW_MAX) return;
  if (tid < LW_MAX * 2) h[tid] = 0;
  __syncthreads();
  const int64_t P = pcount[br];
  int nfp = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + tid; p < P && p < cap; p += (int64_t)gridDim.x * 256) {
    unsigned long long t = touch[(int64_t)br * cap + p];
    const unsigned sz = (unsigned)psizes[(int64_t)br * cap + p];
    nfp += t == 0;
    while (t) {
      const int g = __ffsll((long long)t) - 1;
      t &= t - 1;
      atomicAdd(&h[g * 2], sz);
      atomicAdd(&h[g * 2 + 1], 1u);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nfp += __shfl_xor(nfp, o, 64);
  if ((tid & 63) == 0 && nfp) atomicAdd(fp + br, (unsigned long long)nfp);
  __syncthreads();
  if (tid < LW_MAX * 2 && h[tid]) atomicAdd(acc + ((int64_t)br * LW_MAX + (tid >> 1)) * 4 + ((tid & 1) ? 3 : 1), (unsigned long long)h[tid]);
}

// Lesions 8 k + 1 .. 8 k + 8 of region r as region-bit bytes for cwf_hausdorff: pa = pred_g, pb = lesion g.  One sample per blockIdx.y.
__global__ __launch_bounds__(256) void lw_pack_kernel(const uint8_t* __restrict__ gt, const int* __restrict__ plab, const int* __restrict__ dlab,
                                                      const int* __restrict__ dcount, const unsigned long long* __restrict__ touch,
                                                      uint8_t* __restrict__ pa, uint8_t* __restrict__ pb, int R, int r, int k, int64_t V,
                                                      int64_t cap) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const int b = blockIdx.y, br = b * R + r;
  unsigned a = 0, c = 0;
  if (dcount[br] <= LW_MAX) {
    const int p = plab[(int64_t)br * V + v];
    if (p > 0) a = (unsigned)(touch[(int64_t)br * cap + p - 1] >> (8 * k)) & 255u;
    const int j = dlab[(int64_t)br * V + v] - 1 - 8 * k;
    if (j >= 0 && j < 8 && ((gt[(int64_t)b * V + v] >> r) & 1)) c = 1u << j;
  }
  pa[(int64_t)b * V + v] = (uint8_t)a;
  pb[(int64_t)b * V + v] = (uint8_t)c;
}

struct LwFinal {
  int R, B, maxg[8];          // maxg[r]: the largest lesion count of region r over the samples within the cap (sizes the HD95 calls)
  long long min_lesion;
  double penalty;
};

// One workgroup of LW_MAX threads per (sample, region).  hd95 of lesion g = 8 k + j was written by the call for (r, k) at
// hdt[(r * 8 + k) * B * 8 + b * Rk + j], Rk = min(8, maxg[r] - 8 k) regions in that call; its nsd, with T > 0, at
// nsdt[((r * 8 + k) * B * 8 + b * Rk + j) * T + t].  With T == 0 nsdt, lesion_nsd and lw_nsd are not touched.
__global__ __launch_bounds__(LW_MAX) void lw_final_kernel(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ fp,
                                                          const int* __restrict__ pcount, const int* __restrict__ dcount,
                                                          const double* __restrict__ hdt, LwFinal a, double* __restrict__ summary,
                                                          int64_t* __restrict__ counts, int* __restrict__ overflow, int64_t* __restrict__ table,
                                                          double* __restrict__ lesion_hd95, const double* __restrict__ nsdt, int T,
                                                          double* __restrict__ lesion_nsd, double* __restrict__ lw_nsd) {
  __shared__ double sd[LW_MAX], sh[LW_MAX], sn[LW_MAX_TAU][LW_MAX];
  __shared__ int keep[LW_MAX], miss[LW_MAX];
  const int br = blockIdx.x, b = br / a.R, r = br % a.R, g = threadIdx.x;
  const int G = dcount[br];
  if (G > LW_MAX) {
    if (g == 0) overflow[br] = 1;
    return;
  }
  const unsigned long long* t = acc + ((int64_t)br * LW_MAX + g) * 4;
  const long long gv = (long long)t[0], pv = (long long)t[1], in = (long long)t[2], nt = (long long)t[3];
  double dice = 0.0, hd = 0.0, ns[LW_MAX_TAU] = {0.0, 0.0, 0.0, 0.0};
  if (g < G) {
    if (nt == 0) {
      hd = a.penalty;
    } else {
      const int k = g >> 3, j = g & 7, rk = min(8, a.maxg[r] - 8 * k);
      dice = (double)(2 * in) / (double)(pv + gv);
      hd = hdt[((int64_t)r * 8 + k) * a.B * 8 + (int64_t)b * rk + j];
      for (int t = 0; t < T; ++t) ns[t] = nsdt[(((int64_t)r * 8 + k) * a.B * 8 + (int64_t)b * rk + j) * T + t];
    }
  }
  sd[g] = dice; sh[g] = hd;
  for (int t = 0; t < T; ++t) {
    sn[t][g] = ns[t];
    lesion_nsd[((int64_t)br * LW_MAX + g) * T + t] = ns[t];
  }
  keep[g] = g < G && gv > a.min_lesion;
  miss[g] = g < G && gv > a.min_lesion && nt == 0;
  int64_t* row = table + ((int64_t)br * LW_MAX + g) * 4;
  row[0] = g < G ? gv : 0; row[1] = g < G ? pv : 0; row[2] = g < G ? in : 0; row[3] = g < G ? nt : 0;
  lesion_hd95[(int64_t)br * LW_MAX + g] = hd;
  __syncthreads();
  if (g != 0) return;
  const long long nfp = (long long)fp[br], P = pcount[br];
  double sdice = 0.0, shd = 0.0;
  long long kept = 0, fn = 0;
  for (int i = 0; i < G; ++i)
    if (keep[i]) { sdice += sd[i]; shd += sh[i]; ++kept; fn += miss[i]; }
  const long long n = kept + nfp;
  summary[br * 2 + 0] = n ? sdice / (double)n : 1.0;
  summary[br * 2 + 1] = n ? (shd + (double)nfp * a.penalty) / (double)n : 0.0;
  for (int t = 0; t < T; ++t) {
    double snsd = 0.0;
    for (int i = 0; i < G; ++i)
      if (keep[i]) snsd += sn[t][i];
    lw_nsd[br * T + t] = n ? snsd / (double)n : 1.0;
  }
  int64_t* c = counts + (int64_t)br * 6;
  c[0] = G; c[1] = kept; c[2] = P - nfp; c[3] = nfp; c[4] = fn; c[5] = P;
  overflow[br] = 0;
}

static inline int64_t lw_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Workspace layout: gt_dil [B][V] | dilation ping-pong [B][V] | pred labels, dilated labels [B][R][V] ints each | pred sizes
// [B][R][cap] ints | touch [B][R][cap] uint64 (first the sizes output of the second labelling, which nothing reads) | pred count, dilated
// count [B][R], largest [B][R][2] ints | acc [B][R][64][4], fp [B][R] uint64 | packed a, b [B][V] | hd95 per call [R][8][B][8], hd
// scratch [B][8] doubles, counts scratch [B][8][4] int64 | the workspace of cwf_components or of cwf_hausdorff, whichever is larger
// (they are used one after the other on one stream).  cwf_lesionwise_ex: nsd per call [R][8][B][8][4] and asd [B][8][2], assd [B][8],
// within [B][8][4][2] scratch go before the last block, which then holds cwf_surface_metrics' workspace in cwf_hausdorff's place.
struct LwLayout { int64_t dil, tmp, plab, dlab, psizes, touch, pcount, dcount, largest, acc, fp, pa, pb, hdt, hds, hdc, nsdt, asd, assd, within, sub, sub_bytes, total; };
static int lw_layout(int B, int R, int D0, int D1, int D2, bool ex, LwLayout& L) {
  const int64_t cc = cwf_components_workspace(B, R, D0, D1, D2);
  if (cc < 0) return (int)cc;
  const int64_t hd = ex ? cwf_surface_metrics_workspace(B, 8, D0, D1, D2) : cwf_hausdorff_workspace(B, 8, D0, D1, D2);
  if (hd < 0) return (int)hd;
  const int64_t V = (int64_t)D0 * D1 * D2, cap = (V + 1) / 2, BR = (int64_t)B * R;
  L.dil = 0;
  L.tmp = lw_align(L.dil + B * V);
  L.plab = lw_align(L.tmp + B * V);
  L.dlab = lw_align(L.plab + BR * V * 4);
  L.psizes = lw_align(L.dlab + BR * V * 4);
  L.touch = lw_align(L.psizes + BR * cap * 4);
  L.pcount = lw_align(L.touch + BR * cap * 8);
  L.dcount = lw_align(L.pcount + BR * 4);
  L.largest = lw_align(L.dcount + BR * 4);
  L.acc = lw_align(L.largest + BR * 8);
  L.fp = lw_align(L.acc + BR * LW_MAX * 4 * 8);
  L.pa = lw_align(L.fp + BR * 8);
  L.pb = lw_align(L.pa + B * V);
  L.hdt = lw_align(L.pb + B * V);
  L.hds = lw_align(L.hdt + (int64_t)R * 8 * B * 8 * 8);
  L.hdc = lw_align(L.hds + (int64_t)B * 8 * 8);
  L.nsdt = lw_align(L.hdc + (int64_t)B * 8 * 4 * 8);
  L.asd = L.assd = L.within = L.sub = L.nsdt;
  if (ex) {
    L.asd = lw_align(L.nsdt + (int64_t)R * 8 * B * 8 * LW_MAX_TAU * 8);
    L.assd = lw_align(L.asd + (int64_t)B * 8 * 2 * 8);
    L.within = lw_align(L.assd + (int64_t)B * 8 * 8);
    L.sub = lw_align(L.within + (int64_t)B * 8 * LW_MAX_TAU * 2 * 8);
  }
  L.sub_bytes = std::max(cc, hd);
  L.total = lw_align(L.sub + L.sub_bytes);
  return 0;
}

extern "C" int64_t cwf_lesionwise_workspace(int B, int R, int D0, int D1, int D2) {
  LwLayout L;
  const int rc = lw_layout(B, R, D0, D1, D2, false, L);
  return rc ? rc : L.total;
}

extern "C" int64_t cwf_lesionwise_ex_workspace(int B, int R, int D0, int D1, int D2) {
  LwLayout L;
  const int rc = lw_layout(B, R, D0, D1, D2, true, L);
  return rc ? rc : L.total;
}

// cwf_lesionwise (ex == false: the workspace of cwf_lesionwise_workspace, cwf_hausdorff per group of lesions, T == 0) and
// cwf_lesionwise_ex (the workspace of cwf_lesionwise_ex_workspace, cwf_surface_metrics per group)
static int lw_run(const uint8_t* pred, const uint8_t* gt, int B, int R, int D0, int D1, int D2, int dilation, int64_t min_lesion_voxels,
                  double penalty, bool ex, const double* tau, int T, double* summary, int64_t* counts, int32_t* overflow, int64_t* table,
                  double* lesion_hd95, double* lesion_nsd, double* lw_nsd, void* ws, int64_t ws_bytes, void* stream) {
  LwLayout L;
  int rc = lw_layout(B, R, D0, D1, D2, ex, L);
  if (rc) return rc;
  if (!pred || !gt || !summary || !counts || !overflow || !table || !lesion_hd95 || !ws) return CWF_E_BADARG;
  if (ex) {
    if (T < 0 || T > LW_MAX_TAU || (T > 0 && (!tau || !lesion_nsd || !lw_nsd))) return CWF_E_BADARG;
    for (int t = 0; t < T; ++t)
      if (!(tau[t] >= 0.0)) return CWF_E_BADARG;
  }
  if (dilation < 0 || dilation > 8 || min_lesion_voxels < 0 || !(penalty >= 0.0 && penalty < 1e300)) return CWF_E_BADARG;
  if (ws_bytes < L.total) return CWF_E_TOOLARGE;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  uint8_t* w = (uint8_t*)ws;
  const int64_t V = (int64_t)D0 * D1 * D2, cap = (V + 1) / 2;
  const int BR = B * R;
  uint8_t* dil = w + L.dil;
  int* plab = (int*)(w + L.plab);
  int* dlab = (int*)(w + L.dlab);
  int* psizes = (int*)(w + L.psizes);
  unsigned long long* touch = (unsigned long long*)(w + L.touch);
  int* pcount = (int*)(w + L.pcount);
  int* dcount = (int*)(w + L.dcount);
  int* largest = (int*)(w + L.largest);
  unsigned long long* acc = (unsigned long long*)(w + L.acc);
  unsigned long long* fp = (unsigned long long*)(w + L.fp);
  uint8_t* pa = w + L.pa;
  uint8_t* pb = w + L.pb;
  double* hdt = (double*)(w + L.hdt);
  double* hds = (double*)(w + L.hds);
  int64_t* hdc = (int64_t*)(w + L.hdc);
  double* nsdt = (double*)(w + L.nsdt);
  void* sub = w + L.sub;

  rc = cwf_dilate_bits(gt, dil, B, D0, D1, D2, 2, dilation, w + L.tmp, (int64_t)B * V, stream);
  if (rc) return rc;
  rc = cwf_components(pred, B, R, D0, D1, D2, 3, plab, psizes, pcount, largest, sub, L.sub_bytes, stream);
  if (rc) return rc;
  rc = cwf_components(dil, B, R, D0, D1, D2, 3, dlab, (int*)touch, dcount, largest, sub, L.sub_bytes, stream);
  if (rc) return rc;
  if (hipMemsetAsync(acc, 0, (size_t)(L.pa - L.acc), st) != hipSuccess) return (int)hipErrorInvalidValue;        // acc and fp
  if (hipMemsetAsync(hdt, 0, (size_t)(L.hds - L.hdt), st) != hipSuccess) return (int)hipErrorInvalidValue;
  const unsigned gc = (unsigned)std::min<int64_t>(cdiv64(cap, 256), 256);
  hipLaunchKernelGGL(lw_clear_kernel, dim3(gc, BR), dim3(256), 0, st, touch, (const int*)pcount, cap);
  CWF_LAUNCH_CHECK();
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(V, 256), 1024);
  hipLaunchKernelGGL(lw_touch_kernel, dim3(gx, BR), dim3(256), 0, st, gt, (const int*)plab, (const int*)dlab, (const int*)dcount, touch, acc, R,
                     V, cap);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(lw_comp_kernel, dim3(gc, BR), dim3(256), 0, st, (const unsigned long long*)touch, (const int*)psizes, (const int*)pcount,
                     (const int*)dcount, acc, fp, cap);
  CWF_LAUNCH_CHECK();

  // the one readback: lesion counts, to launch only the HD95 calls that hold a lesion
  std::vector<int> hcount((size_t)BR);
  if (hipMemcpyAsync(hcount.data(), dcount, (size_t)BR * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return (int)hipErrorInvalidValue;
  if (hipStreamSynchronize(st) != hipSuccess) return (int)hipErrorUnknown;
  LwFinal fa;
  fa.R = R; fa.B = B; fa.min_lesion = (long long)min_lesion_voxels; fa.penalty = penalty;
  for (int r = 0; r < 8; ++r) fa.maxg[r] = 0;
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < R; ++r) {
      const int g = hcount[(size_t)b * R + r];
      if (g <= LW_MAX) fa.maxg[r] = std::max(fa.maxg[r], g);
    }
  for (int r = 0; r < R; ++r)
    for (int k = 0; 8 * k < fa.maxg[r]; ++k) {
      const int rk = std::min(8, fa.maxg[r] - 8 * k);
      hipLaunchKernelGGL(lw_pack_kernel, dim3((unsigned)cdiv64(V, 256), B), dim3(256), 0, st, gt, (const int*)plab, (const int*)dlab,
                         (const int*)dcount, (const unsigned long long*)touch, pa, pb, R, r, k, V, cap);
      CWF_LAUNCH_CHECK();
      const int64_t o = ((int64_t)r * 8 + k) * B * 8;
      if (ex)
        rc = cwf_surface_metrics(pa, pb, B, rk, D0, D1, D2, 1.0, 1.0, 1.0, 1, 0, tau, T, hds, hdt + o, (double*)(w + L.asd), (double*)(w + L.assd),
                                 (int64_t*)(w + L.within), nsdt + o * T, hdc, sub, L.sub_bytes, stream);
      else
        rc = cwf_hausdorff(pa, pb, B, rk, D0, D1, D2, 1.0, 1.0, 1.0, 1, 0, hds, hdt + o, hdc, sub, L.sub_bytes, stream);
      if (rc) return rc;
    }
  hipLaunchKernelGGL(lw_final_kernel, dim3(BR), dim3(LW_MAX), 0, st, (const unsigned long long*)acc, (const unsigned long long*)fp,
                     (const int*)pcount, (const int*)dcount, (const double*)hdt, fa, summary, counts, overflow, table, lesion_hd95,
                     (const double*)nsdt, T, lesion_nsd, lw_nsd);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_lesionwise(const uint8_t* pred, const uint8_t* gt, int B, int R, int D0, int D1, int D2, int dilation,
                              int64_t min_lesion_voxels, double penalty, double* summary, int64_t* counts, int32_t* overflow, int64_t* table,
                              double* lesion_hd95, void* ws, int64_t ws_bytes, void* stream) {
  return lw_run(pred, gt, B, R, D0, D1, D2, dilation, min_lesion_voxels, penalty, false, nullptr, 0, summary, counts, overflow, table,
                lesion_hd95, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int cwf_lesionwise_ex(const uint8_t* pred, const uint8_t* gt, int B, int R, int D0, int D1, int D2, int dilation,
                                 int64_t min_lesion_voxels, double penalty, const double* tau, int T, double* summary, int64_t* counts,
                                 int32_t* overflow, int64_t* table, double* lesion_hd95, double* lesion_nsd, double* lw_nsd, void* ws,
                                 int64_t ws_bytes, void* stream) {
  return lw_run(pred, gt, B, R, D0, D1, D2, dilation, min_lesion_voxels, penalty, true, tau, T, summary, counts, overflow, table, lesion_hd95,
                lesion_nsd, lw_nsd, ws, ws_bytes, stream);
}
