// L2 -- boundary loss (Kervadec et al., MIDL 2019): dense exact Euclidean signed distance maps of label maps, and the fused loss
// mean(phi * p) with its analytic backward.  The float statement (restated in tests/boundary_ref.py):
//   label   int64 [N, D0, D1, D2].  Region r is a class bitmask posmask_r: voxel v is in G_r iff 0 <= label < 32 and
//           (posmask_r >> label) & 1.  1 <= R <= 8 regions per call, 1 <= D_d <= 512 per axis (3 * 511^2 fits int32 with room to spare).
//   q_r(v)  unit spacing: for v outside G_r the exact integer squared Euclidean distance to the nearest voxel of G_r, for v inside G_r
//           that to the nearest voxel of the volume outside G_r.
//   phi_r(v) = float32(sqrt((double)q)) outside, float32(1.0 - sqrt((double)q)) inside, formed in float64 and rounded once: the
//           (edt(~G) * ~G - (edt(G) - 1) * G).astype(float32) of the common one_hot2dist.  (1.0f - sqrtf(q) in float32 is another value.)
//           A (sample, region) whose G_r is empty or fills the volume has no opposite voxel: every q is "infinite" and phi_r = +0 there.
//   prob    float32 [N, V, C] channels-last, V = D0 D1 D2.  p_r = float32 sum of p_c over c in r, in increasing c.
//   loss    S = sum_{n, r, v} (double)phi_r (double)p_r;  loss = float32((double)w / (N R V) * S), w read from device memory.
//   bwd     k = float32((double)w / (N R V));  s_c(n, v) = float32 sum of phi_r over r containing c, in increasing r;
//           dprob[n, v, c] = (gscale * k) * s_c, each product rounded on its own; a class in no region gets +0.
// This file is compiled with -ffp-contract=off.
//
// The transform is separable and runs on integers.  Both feature sets share ONE signed field: at every voxel exactly one of "squared
// distance to the nearest inside voxel" and "to the nearest outside voxel" is zero, so a voxel stores the non-zero one, negated when the
// voxel is inside (it is >= 1, or the INF marker when the lines seen so far hold no opposite voxel).  An axis pass gives the target t
//   min over the voxels u of its line of  (u on t's side ? stored(u) : 0) + (t - u)^2
// which is the minimum over every opposite voxel of the sub-volume the passes so far span.  Three kernels per call:
//   bd_axis2_kernel  the contiguous axis: one wave per line reads the labels ONCE for all R regions, ballots the membership bits into
//                    64-bit words and finds the nearest opposite bit on either side by clz / ffs; int16 signed distance (not squared)
//   bd_axis1_kernel  a workgroup owns (whole axis 1) x 64 contiguous voxels of one (sample, region, i0): the line values are staged in
//                    LDS and every target searches outward, stopping at the first offset whose own square reaches the best value
//                    found (the early exit of hd_edt_gather_kernel); int32 signed squared distance
//   bd_axis0_kernel  the same over (whole axis 0) x 64 contiguous voxels of the (axis 1, axis 2) plane, then the square root in
//                    float64, the sign and the float32 store of phi [N, R, D0, D1, D2]
// Both strided passes run 1024-thread workgroups (16 waves share a slab's targets) and bound each column's search by the span of
// positions that can contribute (bd_spans_*, bd_search).  Their static LDS stays at zero: the 160 KiB dynamic limit leaves no room
// for any.  The workspace is fully rewritten by every call, so nothing is zeroed; no kernel waits on another workgroup; there is no
// host synchronisation and no read-back.
#include <algorithm>
#include "common.h"

#define BD_MAX_EXT 512
#define BD_MAX_R 8
#define BD_INF16 0x4000          // |value| >= this after the axis-2 pass: the line holds no opposite voxel
#define BD_INF32 0x40000000      // |value| >= this after the axis-1 / axis-0 pass: no opposite voxel so far
#define BD_SLAB_THREADS 1024     // a slab workgroup: 16 waves, wave w takes the targets w, w + 16, ... of each of its 64 columns
#define BD_SPAN_BYTES (6 * 64 * 4)   // LDS behind the staged lines of a slab: six spans per column

struct BdMasks { uint32_t m[BD_MAX_R]; };

__device__ __forceinline__ bool bd_in(int64_t lab, uint32_t mask) { return lab >= 0 && lab < 32 && ((mask >> (int)lab) & 1u) != 0u; }

// One wave per axis-(0, 1) line of the whole batch, four lines per workgroup.
__global__ __launch_bounds__(256) void bd_axis2_kernel(const int64_t* __restrict__ label, BdMasks mk, int R, int D2, int64_t nlines,
                                                       int64_t lines_per_sample, int64_t V, int16_t* __restrict__ out16) {
  __shared__ unsigned long long words[4][BD_MAX_R][BD_MAX_EXT / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t line = (int64_t)blockIdx.x * 4 + wave;
  const bool valid = line < nlines;
  const int nch = (D2 + 63) >> 6;
  if (valid) {
    const int64_t* src = label + line * D2;
    for (int c = 0; c < nch; ++c) {
      const int x = c * 64 + lane;
      const int64_t lab = x < D2 ? src[x] : -1;
      for (int r = 0; r < R; ++r) {
        const unsigned long long b = __ballot(bd_in(lab, mk.m[r]));
        if (lane == 0) words[wave][r][c] = b;
      }
    }
  }
  __syncthreads();
  if (!valid) return;
  const int64_t n = line / lines_per_sample, lin = line - n * lines_per_sample;
  const unsigned long long tail = (D2 & 63) ? ((1ull << (D2 & 63)) - 1ull) : ~0ull;      // voxels of the last word that exist
  for (int r = 0; r < R; ++r) {
    int16_t* dst = out16 + ((n * R + r) * V + lin * D2);
    const unsigned long long* w = words[wave][r];
    for (int c = 0; c < nch; ++c) {
      const int x = c * 64 + lane;
      const bool in = ((w[c] >> lane) & 1ull) != 0ull;
      const unsigned long long flip = in ? ~0ull : 0ull;
      int d = BD_INF16;
      for (int j = c; j >= 0; --j) {                 // nearest opposite voxel below x
        unsigned long long o = (w[j] ^ flip) & (j == nch - 1 ? tail : ~0ull);
        if (j == c) o &= lane ? (~0ull >> (64 - lane)) : 0ull;
        if (o) { d = x - (j * 64 + 63 - __clzll((long long)o)); break; }
      }
      for (int j = c; j < nch; ++j) {                // and above
        unsigned long long o = (w[j] ^ flip) & (j == nch - 1 ? tail : ~0ull);
        if (j == c) o &= lane < 63 ? (~0ull << (lane + 1)) : 0ull;
        if (o) { d = min(d, j * 64 + __ffsll((long long)o) - 1 - x); break; }
      }
      if (x < D2) dst[x] = (int16_t)(in ? -d : d);
    }
  }
}

// Per column of a slab, the spans of line positions a search can gain from, six rows of 64 ints in LDS behind the staged lines:
// rows 0 / 1 the first / last position holding a finite value, rows 2 / 3 those of an inside voxel, rows 4 / 5 of an outside voxel
// (first = E, last = -1 when there is none).  A target only has to visit [first, last] of (finite values) u (voxels of the other
// side): a same-side voxel without a finite value contributes nothing.  With a small region in a large volume that span is the
// region's extent, where the plain outward search walks the whole way from the target to it; a column without a span (the region is
// empty or full over it so far) is not searched at all.
struct BdSpans { int lofin, hifin, loin, hiin, loout, hiout; };

__device__ __forceinline__ void bd_spans_init(int* rng, int E) {
  for (int i = threadIdx.x; i < 6 * 64; i += BD_SLAB_THREADS) rng[i] = ((i >> 6) & 1) ? -1 : E;
}
__device__ __forceinline__ void bd_spans_note(BdSpans& s, int i, bool finite, bool in) {
  if (finite) { s.lofin = min(s.lofin, i); s.hifin = i; }
  if (in) { s.loin = min(s.loin, i); s.hiin = i; } else { s.loout = min(s.loout, i); s.hiout = i; }
}
__device__ __forceinline__ void bd_spans_merge(int* rng, int x, const BdSpans& s) {
  atomicMin(&rng[0 * 64 + x], s.lofin); atomicMax(&rng[1 * 64 + x], s.hifin);
  atomicMin(&rng[2 * 64 + x], s.loin);  atomicMax(&rng[3 * 64 + x], s.hiin);
  atomicMin(&rng[4 * 64 + x], s.loout); atomicMax(&rng[5 * 64 + x], s.hiout);
}
__device__ __forceinline__ BdSpans bd_spans_load(const int* rng, int x) {
  return BdSpans{rng[0 * 64 + x], rng[1 * 64 + x], rng[2 * 64 + x], rng[3 * 64 + x], rng[4 * 64 + x], rng[5 * 64 + x]};
}

// what the staged value v of a line voxel offers a target on side `in` at squared offset kk (SQUARE: v is an axis-2 distance)
template <bool SQUARE>
__device__ __forceinline__ int bd_cand(int v, bool in, int kk) {
  const int va = v < 0 ? -v : v;
  if ((v < 0) != in) return kk;
  if (SQUARE) return va >= BD_INF16 ? BD_INF32 : va * va + kk;
  return va >= BD_INF32 ? BD_INF32 : va + kk;
}

// The minimum for the target at position i of one column (col[p * 64] = staged value at position p), starting from its own value
// `best`, over the span [lo, hi].  A target outside the span walks it in one direction, four positions per trip (positions past the
// far end are clamped to it: a repeated candidate changes nothing) with one exit test per trip; a target inside it searches outward
// on both sides.  Either way the walk stops at the first offset whose own square reaches the best value found.
template <bool SQUARE, typename T>
__device__ __forceinline__ int bd_search(const T* __restrict__ col, int i, bool in, int best, int lo, int hi) {
  if (lo > hi) return best;
  if (i < lo || i > hi) {
    const int dir = i < lo ? 1 : -1;
    for (int u = i < lo ? lo : hi; u >= lo && u <= hi; u += 4 * dir) {
      const int k = dir * (u - i);
      if (k * k >= best) break;
      int p[4], v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { p[j] = min(max(u + dir * j, lo), hi); v[j] = (int)col[p[j] * 64]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int kj = p[j] - i; best = min(best, bd_cand<SQUARE>(v[j], in, kj * kj)); }
    }
    return best;
  }
  const int k1 = max(i - lo, hi - i);
  for (int k = 1; k <= k1; ++k) {
    const int kk = k * k;
    if (kk >= best) break;
    const int p0 = i - k, p1 = i + k;
    if (p0 >= lo) best = min(best, bd_cand<SQUARE>((int)col[p0 * 64], in, kk));
    if (p1 <= hi) best = min(best, bd_cand<SQUARE>((int)col[p1 * 64], in, kk));
  }
  return best;
}

// One workgroup per (sample * region, i0, 64-voxel chunk of axis 2); LDS: [D1][64] int16 + the spans.
__global__ __launch_bounds__(BD_SLAB_THREADS) void bd_axis1_kernel(const int16_t* __restrict__ in16, int32_t* __restrict__ out32, int D0, int D1, int D2,
                                                       int nxc, int64_t V) {
  extern __shared__ int16_t bd_s16[];
  int* rng = reinterpret_cast<int*>(bd_s16 + D1 * 64);
  const int64_t bid = blockIdx.x;
  const int xc = (int)(bid % nxc);
  const int64_t t = bid / nxc;
  const int i0 = (int)(t % D0);
  const int64_t nr = t / D0;
  const int x = threadIdx.x & 63, row0 = threadIdx.x >> 6;
  const bool xok = xc * 64 + x < D2;
  const int64_t base = nr * V + (int64_t)i0 * D1 * D2 + xc * 64 + x;
  bd_spans_init(rng, D1);
  __syncthreads();
  BdSpans mine = {D1, -1, D1, -1, D1, -1};
  if (xok) {
    for (int i1 = row0; i1 < D1; i1 += BD_SLAB_THREADS / 64) {
      const int v = (int)in16[base + (int64_t)i1 * D2];
      bd_s16[i1 * 64 + x] = (int16_t)v;
      bd_spans_note(mine, i1, v < BD_INF16 && v > -BD_INF16, v < 0);
    }
    bd_spans_merge(rng, x, mine);
  }
  __syncthreads();
  if (!xok) return;
  const BdSpans sp = bd_spans_load(rng, x);
  for (int i1 = row0; i1 < D1; i1 += BD_SLAB_THREADS / 64) {
    const int v = bd_s16[i1 * 64 + x];
    const bool in = v < 0;
    const int a = in ? -v : v;
    int best = a >= BD_INF16 ? BD_INF32 : a * a;
    best = bd_search<true>(bd_s16 + x, i1, in, best, min(sp.lofin, in ? sp.loout : sp.loin), max(sp.hifin, in ? sp.hiout : sp.hiin));
    out32[base + (int64_t)i1 * D2] = in ? -best : best;
  }
}

// One workgroup per (sample * region, 64-voxel chunk of the (axis 1, axis 2) plane); LDS: [D0][64] int32 + the spans.
__global__ __launch_bounds__(BD_SLAB_THREADS) void bd_axis0_kernel(const int32_t* __restrict__ in32, float* __restrict__ phi, int D0, int64_t plane, int npc,
                                                       int64_t V) {
  extern __shared__ int32_t bd_s32[];
  int* rng = bd_s32 + D0 * 64;
  const int64_t bid = blockIdx.x;
  const int pc = (int)(bid % npc);
  const int64_t nr = bid / npc;
  const int x = threadIdx.x & 63, row0 = threadIdx.x >> 6;
  const bool xok = (int64_t)pc * 64 + x < plane;
  const int64_t base = nr * V + (int64_t)pc * 64 + x;
  bd_spans_init(rng, D0);
  __syncthreads();
  BdSpans mine = {D0, -1, D0, -1, D0, -1};
  if (xok) {
    for (int i0 = row0; i0 < D0; i0 += BD_SLAB_THREADS / 64) {
      const int v = in32[base + (int64_t)i0 * plane];
      bd_s32[i0 * 64 + x] = v;
      bd_spans_note(mine, i0, v < BD_INF32 && v > -BD_INF32, v < 0);
    }
    bd_spans_merge(rng, x, mine);
  }
  __syncthreads();
  if (!xok) return;
  const BdSpans sp = bd_spans_load(rng, x);
  for (int i0 = row0; i0 < D0; i0 += BD_SLAB_THREADS / 64) {
    const int v = bd_s32[i0 * 64 + x];
    const bool in = v < 0;
    int best = in ? -v : v;
    best = bd_search<false>(bd_s32 + x, i0, in, best, min(sp.lofin, in ? sp.loout : sp.loin), max(sp.hifin, in ? sp.hiout : sp.hiin));
    float o = 0.f;                                   // no opposite voxel in the volume: the region is empty or full
    if (best < BD_INF32) {
      const double d = sqrt((double)best);
      o = in ? (float)(1.0 - d) : (float)d;
    }
    phi[base + (int64_t)i0 * plane] = o;
  }
}

// S += sum over this workgroup's voxels of (double)phi_r * (double)p_r: float64 partials per thread, one atomic per workgroup.
template <bool C4>
__global__ __launch_bounds__(256) void bd_sums_kernel(const float* __restrict__ prob, const float* __restrict__ phi, BdMasks mk, int R, int C,
                                                      int64_t V, int64_t total, double* __restrict__ sum) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t gv = (int64_t)blockIdx.x * 256 + threadIdx.x; gv < total; gv += (int64_t)gridDim.x * 256) {
    const int64_t n = gv / V, v = gv - n * V;
    float p4[4] = {0.f, 0.f, 0.f, 0.f};
    if (C4) { const float4 q = *reinterpret_cast<const float4*>(prob + gv * 4); p4[0] = q.x; p4[1] = q.y; p4[2] = q.z; p4[3] = q.w; }
    for (int r = 0; r < R; ++r) {
      const uint32_t m = mk.m[r];
      float pr = 0.f;
      if (C4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) if ((m >> c) & 1u) pr += p4[c];
      } else {
        for (int c = 0; c < C; ++c) if ((m >> c) & 1u) pr += prob[gv * C + c];
      }
      acc += (double)phi[(n * R + r) * V + v] * (double)pr;
    }
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomic_add_f64(sum, (red[0] + red[1]) + (red[2] + red[3]));
}

// single thread: loss[0] = float32((double)w / (N R V) * S), coef[0] = k = float32((double)w / (N R V))
__global__ void bd_finalize_kernel(const double* __restrict__ sum, const float* __restrict__ weight, float* __restrict__ loss,
                                   float* __restrict__ coef, double nrv) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double k = (double)weight[0] / nrv;
  loss[0] = (float)(k * sum[0]);
  coef[0] = (float)k;
}

// (gscale k) * s_c of one class: s_c adds the phi of the regions that hold class c in increasing r; +0 for a class in no region
__device__ __forceinline__ float bd_class_grad(const BdMasks& mk, const float (&f)[BD_MAX_R], int R, int c, float gk) {
  float s = 0.f;
  bool has = false;
#pragma unroll
  for (int r = 0; r < BD_MAX_R; ++r)
    if (r < R && ((mk.m[r] >> c) & 1u)) { s = has ? s + f[r] : f[r]; has = true; }
  return has ? gk * s : 0.f;
}

template <bool C4>
__global__ __launch_bounds__(256) void bd_bwd_kernel(const float* __restrict__ phi, BdMasks mk, const float* __restrict__ coef,
                                                     const float* __restrict__ gscale, float* __restrict__ dprob, int R, int C, int64_t V,
                                                     int64_t total) {
  const int64_t gv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gv >= total) return;
  const int64_t n = gv / V, v = gv - n * V;
  const float gk = gscale[0] * coef[0];
  float f[BD_MAX_R];
#pragma unroll
  for (int r = 0; r < BD_MAX_R; ++r) f[r] = r < R ? phi[(n * R + r) * V + v] : 0.f;
  if (C4) {
    *reinterpret_cast<float4*>(dprob + gv * 4) = make_float4(bd_class_grad(mk, f, R, 0, gk), bd_class_grad(mk, f, R, 1, gk),
                                                             bd_class_grad(mk, f, R, 2, gk), bd_class_grad(mk, f, R, 3, gk));
  } else {
    for (int c = 0; c < C; ++c) dprob[gv * C + c] = bd_class_grad(mk, f, R, c, gk);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t bd_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static int bd_check(int B, int R, int D0, int D1, int D2) {
  if (B <= 0 || R < 1 || R > BD_MAX_R) return CWF_E_BADARG;
  if (D0 < 1 || D1 < 1 || D2 < 1 || D0 > BD_MAX_EXT || D1 > BD_MAX_EXT || D2 > BD_MAX_EXT) return CWF_E_BADARG;
  const int64_t V = (int64_t)D0 * D1 * D2;
  // the largest launch is one workgroup per (sample, region, i0, 64-voxel chunk): keep every grid inside 2^31 - 1
  if ((int64_t)B * R * cdiv64(V, 64) > 0x7fffffffll || (int64_t)B * R * D0 * D1 > 0x7fffffffll) return CWF_E_TOOLARGE;
  return 0;
}

static int bd_masks(const uint32_t* posmasks, int R, BdMasks& mk) {
  if (!posmasks || R < 1 || R > BD_MAX_R) return CWF_E_BADARG;
  for (int r = 0; r < BD_MAX_R; ++r) mk.m[r] = r < R ? posmasks[r] : 0u;
  return 0;
}

extern "C" int64_t cwf_signed_distance_workspace(int B, int R, int D0, int D1, int D2) {
  const int rc = bd_check(B, R, D0, D1, D2);
  if (rc) return rc;
  const int64_t nrv = (int64_t)B * R * D0 * D1 * D2;
  return bd_align(nrv * 2) + bd_align(nrv * 4);
}

extern "C" int cwf_signed_distance(const int64_t* label, const uint32_t* posmasks, float* phi, int B, int R, int D0, int D1, int D2, void* ws,
                                   void* stream) {
  int rc = bd_check(B, R, D0, D1, D2);
  if (rc) return rc;
  if (!label || !phi || !ws) return CWF_E_BADARG;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  BdMasks mk;
  if ((rc = bd_masks(posmasks, R, mk))) return rc;
  hipStream_t st = cwf_stream(stream);
  const int64_t plane = (int64_t)D1 * D2, V = (int64_t)D0 * plane, nrv = (int64_t)B * R * V;
  int16_t* f16 = (int16_t*)ws;
  int32_t* f32 = (int32_t*)((uint8_t*)ws + bd_align(nrv * 2));
  const int64_t nlines = (int64_t)B * D0 * D1;
  hipLaunchKernelGGL(bd_axis2_kernel, dim3((unsigned)cdiv64(nlines, 4)), dim3(256), 0, st, label, mk, R, D2, nlines, (int64_t)D0 * D1, V, f16);
  CWF_LAUNCH_CHECK();
  const int nxc = cdiv(D2, 64);
  CWF_MAX_LDS_ONCE(bd_axis1_kernel);
  hipLaunchKernelGGL(bd_axis1_kernel, dim3((unsigned)((int64_t)B * R * D0 * nxc)), dim3(BD_SLAB_THREADS), (size_t)D1 * 64 * sizeof(int16_t) + BD_SPAN_BYTES, st, f16, f32,
                     D0, D1, D2, nxc, V);
  CWF_LAUNCH_CHECK();
  const int npc = (int)cdiv64(plane, 64);
  CWF_MAX_LDS_ONCE(bd_axis0_kernel);
  hipLaunchKernelGGL(bd_axis0_kernel, dim3((unsigned)((int64_t)B * R * npc)), dim3(BD_SLAB_THREADS), (size_t)D0 * 64 * sizeof(int32_t) + BD_SPAN_BYTES, st, f32, phi, D0,
                     plane, npc, V);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_boundary_sums(const float* prob, const float* phi, const uint32_t* posmasks, double* sum, int N, int R, int64_t V, int C,
                                 void* stream) {
  if (!prob || !phi || !sum || N <= 0 || V <= 0 || C < 1 || C > 32) return CWF_E_BADARG;
  BdMasks mk;
  const int rc = bd_masks(posmasks, R, mk);
  if (rc) return rc;
  const int64_t total = (int64_t)N * V;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv64(total, 256), 2048));
  if (C == 4) hipLaunchKernelGGL(bd_sums_kernel<true>, grid, dim3(256), 0, cwf_stream(stream), prob, phi, mk, R, C, V, total, sum);
  else hipLaunchKernelGGL(bd_sums_kernel<false>, grid, dim3(256), 0, cwf_stream(stream), prob, phi, mk, R, C, V, total, sum);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_boundary_finalize(const double* sum, const float* weight, float* loss, float* coef, int N, int R, int64_t V, void* stream) {
  if (!sum || !weight || !loss || !coef || N <= 0 || R < 1 || R > BD_MAX_R || V <= 0) return CWF_E_BADARG;
  hipLaunchKernelGGL(bd_finalize_kernel, dim3(1), dim3(64), 0, cwf_stream(stream), sum, weight, loss, coef, (double)N * (double)R * (double)V);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_boundary_bwd(const float* phi, const uint32_t* posmasks, const float* coef, const float* gscale, float* dprob, int N, int R,
                                int64_t V, int C, void* stream) {
  if (!phi || !coef || !gscale || !dprob || N <= 0 || V <= 0 || C < 1 || C > 32) return CWF_E_BADARG;
  BdMasks mk;
  const int rc = bd_masks(posmasks, R, mk);
  if (rc) return rc;
  const int64_t total = (int64_t)N * V;
  if (cdiv64(total, 256) > 0x7fffffffll) return CWF_E_TOOLARGE;
  const dim3 grid((unsigned)cdiv64(total, 256));
  if (C == 4) hipLaunchKernelGGL(bd_bwd_kernel<true>, grid, dim3(256), 0, cwf_stream(stream), phi, mk, coef, gscale, dprob, R, C, V, total);
  else hipLaunchKernelGGL(bd_bwd_kernel<false>, grid, dim3(256), 0, cwf_stream(stream), phi, mk, coef, gscale, dprob, R, C, V, total);
  CWF_LAUNCH_CHECK();
  return 0;
}
