// N1 -- Hausdorff distance and HD95 of binary masks on the device (the `medpy.metric.binary` hd / hd95 that the reference's
// utils/hausdorff.py and utils/tools.softmax_hd_dice call).  For a pair of masks A, B:
//   border(M)  = M & ~erosion(M) under the 6/18/26-neighbour footprint, out-of-volume voxels counting as unset (every mask voxel on a
//                face of the volume is a border voxel); in all-border mode border(M) = M (medpy on [1, D0, D1, D2] arrays)
//   sd(A, B)   = Euclidean distance, in spacing units, from every voxel of border(A) to the nearest voxel of border(B)
//   hd         = max over sd(A, B) u sd(B, A);  hd95 = numpy's linear 95th percentile of the union of both directions.
// Masks are bytes of region bits (bit r = the voxel is in region r, R <= 8), so one set of launches serves WT / TC / ET at once.
//
// Three kernels per (sample, region) after one border pass over the whole batch:
//   hd_border_kernel      border bytes of A and B and the counts |A|, |B|, |dA|, |dB| (wave ballots, one atomic per workgroup)
//   hd_edt_axis0_kernel   squared distance along axis 0 to the nearest border voxel, (s0 * d0)^2 or +inf, for both transforms
//   hd_edt_gather_kernel  one wave per axis-(0, 1) line holding at least one voxel of the OTHER map's border: the axis-1 pass
//                         min_p g(p) + (s1 (q - p))^2 for the line, staged in LDS, then the axis-2 pass evaluated only at those voxels;
//                         the squared distances are appended to one compact array per (sample, region), the max taken on the way
//   hd_radix_kernel       eight 8-bit digit passes of a radix select over the uint64 bit patterns of the compacted squared distances
//                         (non-negative doubles order like their bit patterns) for the two ranks numpy's percentile interpolates
//                         between; a ninth single-workgroup launch takes sqrt and numpy's lerp.
// Every term is formed as (s * d)^2 and summed in axis order 0, 1, 2, exactly as scipy's distance_transform_edt, and the minimum
// commutes with the monotone rounding of each addition, so the result is the correctly rounded minimum over all border voxels: with unit
// spacing every value is an exact integer.  This file is compiled with -ffp-contract=off (no fused multiply-adds).
//
// N8 -- normalised surface Dice and average surface distance (cwf_surface_metrics), on the same border / EDT / gather / select kernels.
// With q the float64 squared distance above and d(p) = sqrt(q), correctly rounded, for p in dA (to dB) and for p in dB (to dA):
//   within[t][0] = |{p in dA : d(p) <= tau_t}|, within[t][1] the same over dB          (a float64 <= on d)
//   nsd[t]       = (within[t][0] + within[t][1]) / (|dA| + |dB|)                        (one float64 division of two exact integers)
//   asd[0]       = mean of d over dA, asd[1] = mean of d over dB (medpy asd(A, B), asd(B, A));  assd = (asd[0] + asd[1]) / 2 (medpy assd)
//   either mask empty: every float output of that (sample, region) is NaN and within is 0, as for hd / hd95.
// This is the voxel-border NSD (MONAI's compute_surface_dice without sub-voxel handling), not the area-weighted surface-element form of
// DeepMind's surface-distance; with unit spacing every tau < 1 counts coincident border voxels only (d is 0 or >= 1).
// The compact array is filled through an atomic cursor and mixes both directions, so neither output is taken from it.  The surface
// variant of hd_edt_gather_kernel (one wave per line) instead leaves, per line and direction, the sum of d and the T counts in a slot
// of their own: lane l adds its voxels l, l + 64, ... in increasing order, the 64 lane sums go through a fixed xor butterfly, and a line
// without a gather voxel writes zeros.  hd_surface_final_kernel then adds the D0 * D1 slots of a direction with 512 threads, thread i
// taking slots i, i + 512, ... in increasing order, and a fixed binary tree over the 512 partial sums.  Every addition has fixed
// operands whatever order workgroups run or atomics land in, and the shape depends on D0, D1, D2 alone, so asd is bit-identical from
// run to run and from batch to batch; the counts are integers.
#include <algorithm>
#include "common.h"

#define HD_MAX_D2 4096        // axis-2 extent staged in LDS by hd_edt_gather_kernel (at most 32 KiB of doubles)

struct HdSmall {              // per (sample, region) scratch, zeroed by cwf_hausdorff
  unsigned long long cursor;  // entries in the compact array (|dA| + |dB| once the gather pass is done)
  unsigned long long hdmax;   // max squared distance, as its bit pattern
  unsigned long long state[9][2][2];    // radix select: (prefix, remaining rank) of the two target ranks before pass p
  unsigned int hist[8][2][256];         // digit histograms of pass p for the two target ranks
};

#define HD_MAX_TAU 4          // tolerances per cwf_surface_metrics call

struct HdSurface {            // what the surface variant of the gather pass adds; passed by value
  double tau[HD_MAX_TAU];
  int T;
  double* lsum;               // [2][D0 * D1]: per direction and line, the sum of d over the line's gather voxels
  unsigned int* lcnt;         // [2][D0 * D1][HD_MAX_TAU]: the line's voxels with d <= tau[t]
};

__device__ __forceinline__ double hd_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// labels (int64) -> region bits of tools.softmax_output_dice: bit 0 WT (label > 0), bit 1 TC (label 1 or 3), bit 2 ET (label 3)
__global__ void hd_region_bits_kernel(const int64_t* __restrict__ labels, uint8_t* __restrict__ bits, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t l = labels[i];
  bits[i] = (uint8_t)((l > 0 ? 1 : 0) | (l == 1 || l == 3 ? 2 : 0) | (l == 3 ? 4 : 0));
}

// One sample per blockIdx.y; grid-stride over its voxels with a trip count that is the same for every lane (the ballots need them all).
__global__ __launch_bounds__(256) void hd_border_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ ba,
                                                        uint8_t* __restrict__ bb, unsigned long long* __restrict__ counts, int R, int D0, int D1,
                                                        int D2, int conn, int all_border) {
  __shared__ unsigned long long red[32];
  const int s = blockIdx.y;
  const int64_t plane = (int64_t)D1 * D2, V = (int64_t)D0 * plane;
  const uint8_t* as = a + s * V;
  const uint8_t* bs = b + s * V;
  if (threadIdx.x < 32) red[threadIdx.x] = 0;
  unsigned long long acc[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) acc[j] = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < V; base += (int64_t)gridDim.x * 256) {
    const int64_t v = base + threadIdx.x;
    const bool valid = v < V;
    const unsigned ma = valid ? as[v] : 0u, mb = valid ? bs[v] : 0u;
    unsigned ea = 0, eb = 0;                       // eroded masks (all-border mode: nothing survives erosion)
    if (!all_border && (ma | mb)) {
      ea = ma; eb = mb;
      const int i2 = (int)(v % D2);
      const int64_t t = v / D2;
      const int i1 = (int)(t % D1), i0 = (int)(t / D1);
      for (int d0 = -1; d0 <= 1; ++d0)
        for (int d1 = -1; d1 <= 1; ++d1)
          for (int d2 = -1; d2 <= 1; ++d2) {
            const int nz = (d0 != 0) + (d1 != 0) + (d2 != 0);
            if (nz == 0 || nz > conn) continue;
            const int j0 = i0 + d0, j1 = i1 + d1, j2 = i2 + d2;
            if (j0 < 0 || j0 >= D0 || j1 < 0 || j1 >= D1 || j2 < 0 || j2 >= D2) { ea = 0; eb = 0; continue; }
            const int64_t o = (int64_t)j0 * plane + (int64_t)j1 * D2 + j2;
            ea &= as[o]; eb &= bs[o];
          }
    }
    const unsigned bda = ma & ~ea, bdb = mb & ~eb;
    if (valid) { ba[s * V + v] = (uint8_t)bda; bb[s * V + v] = (uint8_t)bdb; }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (r >= R) break;
      acc[r * 4 + 0] += __popcll(__ballot((ma >> r) & 1u));
      acc[r * 4 + 1] += __popcll(__ballot((mb >> r) & 1u));
      acc[r * 4 + 2] += __popcll(__ballot((bda >> r) & 1u));
      acc[r * 4 + 3] += __popcll(__ballot((bdb >> r) & 1u));
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if (j < 4 * R && acc[j]) atomicAdd(&red[j], acc[j]);
  }
  __syncthreads();
  if (threadIdx.x < 4 * R && red[threadIdx.x]) atomicAdd(counts + (int64_t)s * R * 4 + threadIdx.x, red[threadIdx.x]);
}

// One thread per axis-0 column (i1, i2) of one sample and transform t (blockIdx.y): t = 0 is the transform of dB, t = 1 that of dA.
// g[t][v] = (s0 * d0)^2, d0 = distance along axis 0 to the nearest border voxel of the column, +inf if there is none.  Columns
// that hold a border voxel widen range[t][*][i2] (encoded so that zero means empty: lo = D1 - enc_lo, hi = enc_hi - 1), which bounds
// the axis-1 search of the gather pass.
__global__ __launch_bounds__(256) void hd_edt_axis0_kernel(const uint8_t* __restrict__ ba, const uint8_t* __restrict__ bb, int r, int D0, int D1,
                                                           int D2, double s0, double* __restrict__ g, int* __restrict__ range) {
  const int64_t plane = (int64_t)D1 * D2, V = (int64_t)D0 * plane;
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= plane) return;
  const int t = blockIdx.y;
  const uint8_t* src = t == 0 ? bb : ba;
  double* gt = g + (int64_t)t * V;
  const double inf = hd_inf();
  int last = -1;
#pragma unroll 8
  for (int i0 = 0; i0 < D0; ++i0) {
    const int64_t v = i0 * plane + col;
    if ((src[v] >> r) & 1) last = i0;
    gt[v] = last >= 0 ? (double)(i0 - last) : inf;
  }
  if (last < 0) return;                            // no border voxel in the column: +inf throughout, already written
  int next = -1;
#pragma unroll 8
  for (int i0 = D0 - 1; i0 >= 0; --i0) {
    const int64_t v = i0 * plane + col;
    if ((src[v] >> r) & 1) next = i0;
    const double d = next >= 0 ? fmin(gt[v], (double)(next - i0)) : gt[v];
    const double e = s0 * d;
    gt[v] = e * e;
  }
  const int i1 = (int)(col / D2), i2 = (int)(col % D2);
  atomicMax(range + (t * 2 + 0) * D2 + i2, D1 - i1);
  atomicMax(range + (t * 2 + 1) * D2 + i2, i1 + 1);
}

// One 64-lane workgroup per axis-(0, 1) line (i0, i1) and transform t (blockIdx.y): t = 0 gathers the transform of dB at the voxels of
// dA, t = 1 that of dA at dB.  Lines without a gather voxel leave at once.  Both minimum passes search outward from q and stop at the
// first offset k whose own term (s k)^2 already reaches the best value found: every farther candidate is at least that large, as the
// rounding of s * k, of its square and of g + (s k)^2 is monotone and g >= 0.
// SURF: also the line's slot of sv.lsum / sv.lcnt (see the header); without it sv is not touched and the code is what it was.
template <bool SURF>
__global__ __launch_bounds__(64) void hd_edt_gather_kernel(const uint8_t* __restrict__ ba, const uint8_t* __restrict__ bb, int r, int D0, int D1,
                                                           int D2, double s1, double s2, const double* __restrict__ g, const int* __restrict__ range,
                                                           double* __restrict__ compact, int64_t cap, HdSmall* __restrict__ sm, HdSurface sv) {
  extern __shared__ double line[];                 // [D2]
  const int t = blockIdx.y;
  const int64_t plane = (int64_t)D1 * D2, V = (int64_t)D0 * plane;
  const int64_t lidx = blockIdx.x;                 // i0 * D1 + i1
  if (lidx >= (int64_t)D0 * D1) return;
  const int i0 = (int)(lidx / D1), i1 = (int)(lidx % D1);
  const uint8_t* gm = (t == 0 ? ba : bb) + lidx * D2;       // the voxels this transform is gathered at
  const double* gt = g + (int64_t)t * V + (int64_t)i0 * plane;
  const int* rlo = range + (t * 2 + 0) * D2;
  const int* rhi = range + (t * 2 + 1) * D2;
  const int lane = threadIdx.x;
  bool any = false;
  for (int i2 = lane; i2 < D2; i2 += 64) any |= ((gm[i2] >> r) & 1) != 0;
  if (!__any(any)) {
    if constexpr (SURF) {
      if (lane == 0) sv.lsum[(int64_t)t * D0 * D1 + lidx] = 0.0;
      if (lane < HD_MAX_TAU) sv.lcnt[((int64_t)t * D0 * D1 + lidx) * HD_MAX_TAU + lane] = 0u;
    }
    return;
  }
  const double inf = hd_inf();
  // axis 1: g1(i0, i1, i2) = min_p g0(i0, p, i2) + (s1 (i1 - p))^2 over the columns p in [lo, hi] that hold a border voxel
  for (int i2 = lane; i2 < D2; i2 += 64) {
    const int lo = D1 - rlo[i2], hi = rhi[i2] - 1;
    double best = inf;
    if (lo <= hi) {
      const int k0 = max(0, max(lo - i1, i1 - hi)), k1 = max(i1 - lo, hi - i1);
      for (int k = k0; k <= k1; ++k) {
        const double d = s1 * (double)k;
        const double tk = d * d;
        if (tk >= best) break;
        const int p0 = i1 - k, p1 = i1 + k;
        if (p0 >= lo && p0 <= hi) best = fmin(best, gt[(int64_t)p0 * D2 + i2] + tk);
        if (k > 0 && p1 >= lo && p1 <= hi) best = fmin(best, gt[(int64_t)p1 * D2 + i2] + tk);
      }
    }
    line[i2] = best;
  }
  __syncthreads();
  // axis 2 at the gather voxels, appended to the compact array
  unsigned long long mx = 0;
  double dsum = 0.0;                               // SURF: this lane's sum of d and counts of d <= tau[t]
  unsigned int dcnt[HD_MAX_TAU] = {0u, 0u, 0u, 0u};
  for (int base = 0; base < D2; base += 64) {
    const int q = base + lane;
    const bool on = q < D2 && ((gm[q] >> r) & 1);
    double best = 0.0;
    if (on) {
      best = line[q];
      for (int k = 1; k < D2; ++k) {
        const double d = s2 * (double)k;
        const double tk = d * d;
        if (tk >= best) break;
        const int p0 = q - k, p1 = q + k;
        if (p0 < 0 && p1 >= D2) break;
        if (p0 >= 0) best = fmin(best, line[p0] + tk);
        if (p1 < D2) best = fmin(best, line[p1] + tk);
      }
    }
    const unsigned long long m = __ballot(on);
    unsigned long long slot = 0;
    if (lane == 0 && m) slot = atomicAdd(&sm->cursor, (unsigned long long)__popcll(m));
    slot = __shfl(slot, 0, 64) + __popcll(m & ((1ull << lane) - 1ull));
    if (on && slot < (unsigned long long)cap) {
      compact[slot] = best;
      const unsigned long long bits = (unsigned long long)__double_as_longlong(best);
      mx = bits > mx ? bits : mx;
    }
    if constexpr (SURF) {
      if (on) {
        const double d = sqrt(best);
        dsum += d;
#pragma unroll
        for (int j = 0; j < HD_MAX_TAU; ++j) dcnt[j] += (j < sv.T && d <= sv.tau[j]) ? 1u : 0u;
      }
    }
  }
  if constexpr (SURF) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      dsum += __shfl_xor(dsum, o, 64);
#pragma unroll
      for (int j = 0; j < HD_MAX_TAU; ++j) dcnt[j] += __shfl_xor(dcnt[j], o, 64);
    }
    if (lane == 0) {
      sv.lsum[(int64_t)t * D0 * D1 + lidx] = dsum;
#pragma unroll
      for (int j = 0; j < HD_MAX_TAU; ++j) sv.lcnt[((int64_t)t * D0 * D1 + lidx) * HD_MAX_TAU + j] = dcnt[j];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(mx, o, 64);
    mx = y > mx ? y : mx;
  }
  if (lane == 0 && mx) atomicMax(&sm->hdmax, mx);
}

// State of the radix select before pass `pass` (0..8) into LDS: pass 0 from n, pass p from the state and histogram of pass p - 1.
// Ranks lo = floor(v), hi = min(lo + 1, n - 1) of v = (n - 1) * 0.95 (numpy's linear percentile).  256 threads.
__device__ void hd_radix_state(const HdSmall* sm, int pass, unsigned long long n, unsigned long long* pref, unsigned long long* kk,
                               unsigned int (*scan)[256]) {
  const int tid = threadIdx.x;
  if (pass == 0) {
    if (tid == 0) {
      const double v = (double)(n - 1) * 0.95;
      const unsigned long long lo = (unsigned long long)floor(v);
      pref[0] = 0; pref[1] = 0;
      kk[0] = lo; kk[1] = lo + 1 < n - 1 ? lo + 1 : n - 1;
    }
    __syncthreads();
    return;
  }
  const int shift = 56 - 8 * (pass - 1);
  unsigned int h[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { h[t] = sm->hist[pass - 1][t][tid]; scan[t][tid] = h[t]; }
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    unsigned int add[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) add[t] = tid >= off ? scan[t][tid - off] : 0u;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) scan[t][tid] += add[t];
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const unsigned long long incl = scan[t][tid], excl = incl - h[t];
    const unsigned long long k = sm->state[pass - 1][t][1];
    if (excl <= k && k < incl) {
      pref[t] = sm->state[pass - 1][t][0] | ((unsigned long long)tid << shift);
      kk[t] = k - excl;
    }
  }
  __syncthreads();
}

// Passes 0..7: digit histograms of the keys that share the two targets' prefixes.  Pass 8 (one workgroup): the two order statistics,
// sqrt, numpy's lerp, and hd; NaN for both when either mask is empty.
__global__ __launch_bounds__(256) void hd_radix_kernel(const unsigned long long* __restrict__ keys, int64_t cap, HdSmall* __restrict__ sm, int pass,
                                                       const unsigned long long* __restrict__ counts, double* __restrict__ hd,
                                                       double* __restrict__ hd95) {
  __shared__ unsigned int lh[2][256];
  __shared__ unsigned int scan[2][256];
  __shared__ unsigned long long pref[2], kk[2];
  const int tid = threadIdx.x;
  const unsigned long long n0 = sm->cursor;
  const unsigned long long n = n0 < (unsigned long long)cap ? n0 : (unsigned long long)cap;
  if (pass == 8) {
    const bool empty = counts[0] == 0 || counts[1] == 0 || n < 2;
    if (empty) {
      if (tid == 0) { *hd = __longlong_as_double(0x7ff8000000000000ll); *hd95 = *hd; }
      return;
    }
    hd_radix_state(sm, 8, n, pref, kk, scan);
    if (tid == 0) {
      const double v = (double)(n - 1) * 0.95;
      const double gm = v - floor(v);
      const double a = sqrt(__longlong_as_double((long long)pref[0]));
      const double b = sqrt(__longlong_as_double((long long)pref[1]));
      const double diff = b - a;
      *hd95 = gm >= 0.5 ? b - diff * (1.0 - gm) : a + diff * gm;
      *hd = sqrt(__longlong_as_double((long long)sm->hdmax));
    }
    return;
  }
  if (n == 0) return;
  hd_radix_state(sm, pass, n, pref, kk, scan);
  if (blockIdx.x == 0 && tid < 2) { sm->state[pass][tid][0] = pref[tid]; sm->state[pass][tid][1] = kk[tid]; }
  lh[0][tid] = 0; lh[1][tid] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const unsigned long long hmask = pass == 0 ? 0ull : (~0ull << (shift + 8));
  const unsigned long long p0 = pref[0], p1 = pref[1];
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + tid; i < n; i += (unsigned long long)gridDim.x * 256) {
    const unsigned long long key = keys[i];
    const unsigned int d = (unsigned int)(key >> shift) & 255u;
    if ((key & hmask) == p0) atomicAdd(&lh[0][d], 1u);
    if ((key & hmask) == p1) atomicAdd(&lh[1][d], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2; ++t)
    if (lh[t][tid]) atomicAdd(&sm->hist[pass][t][tid], lh[t][tid]);
}

// cwf_surface_metrics zeroes counts and the HdSmall / range part of the workspace with this kernel, not with memset nodes: in a captured
// graph the runtime's node for the small memset of counts was seen to write a wrong pattern from the second replay on.  n0, n1: 8-byte words.
__global__ __launch_bounds__(256) void hd_zero_kernel(unsigned long long* __restrict__ p0, int64_t n0, unsigned long long* __restrict__ p1,
                                                      int64_t n1) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n0 + n1; i += (int64_t)gridDim.x * 256) {
    if (i < n0) p0[i] = 0ull;
    else p1[i - n0] = 0ull;
  }
}

// One workgroup of 1024 threads per (sample, region), after the gather pass: threads 0..511 add the line slots of direction 0 (dA to
// dB), threads 512..1023 those of direction 1, thread i taking slots i, i + 512, ... in increasing order; then a binary tree over the
// 512 partial sums of each half.  The operands of every addition are fixed by L = D0 * D1 alone.  c = |dA|, |dB|.
__global__ __launch_bounds__(1024) void hd_surface_final_kernel(HdSurface sv, int64_t L, const unsigned long long* __restrict__ c,
                                                                double* __restrict__ asd, double* __restrict__ assd,
                                                                long long* __restrict__ within, double* __restrict__ nsd) {
  __shared__ double ss[1024];
  __shared__ unsigned long long sc[HD_MAX_TAU][1024];
  const int tid = threadIdx.x, dir = tid >> 9, i = tid & 511;
  const double* ls = sv.lsum + (int64_t)dir * L;
  const uint4* lc = reinterpret_cast<const uint4*>(sv.lcnt) + (int64_t)dir * L;
  double a = 0.0;
  unsigned long long n[HD_MAX_TAU] = {0ull, 0ull, 0ull, 0ull};
  for (int64_t l = i; l < L; l += 512) {
    a += ls[l];
    if (sv.T > 0) {
      const uint4 k = lc[l];
      n[0] += k.x; n[1] += k.y; n[2] += k.z; n[3] += k.w;
    }
  }
  ss[tid] = a;
#pragma unroll
  for (int j = 0; j < HD_MAX_TAU; ++j) sc[j][tid] = n[j];
  __syncthreads();
  for (int o = 256; o > 0; o >>= 1) {
    if (i < o) {
      ss[tid] += ss[tid + o];
#pragma unroll
      for (int j = 0; j < HD_MAX_TAU; ++j) sc[j][tid] += sc[j][tid + o];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const unsigned long long na = c[0], nb = c[1];
  const bool empty = na == 0 || nb == 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double a0 = empty ? nan : ss[0] / (double)na, a1 = empty ? nan : ss[512] / (double)nb;
  asd[0] = a0; asd[1] = a1;
  *assd = empty ? nan : (a0 + a1) / 2.0;
  for (int j = 0; j < sv.T; ++j) {
    const unsigned long long w0 = empty ? 0ull : sc[j][0], w1 = empty ? 0ull : sc[j][512];
    within[j * 2 + 0] = (long long)w0; within[j * 2 + 1] = (long long)w1;
    nsd[j] = empty ? nan : (double)(w0 + w1) / (double)(na + nb);
  }
}

static inline int64_t hd_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Workspace layout: border bytes [2][B][V] | g [2][V] doubles | compact [2V] doubles | HdSmall [B][R] | range [B][R][4][D2] ints
// cwf_surface_metrics appends: line sums [2][D0 D1] doubles | line counts [2][D0 D1][HD_MAX_TAU] uints
struct HdLayout { int64_t border, g, compact, small, range, total, lsum, lcnt, total_surface; };
static int hd_layout(int B, int R, int D0, int D1, int D2, HdLayout& L) {
  if (B <= 0 || R <= 0 || R > 8 || D0 <= 0 || D1 <= 0 || D2 <= 0) return CWF_E_BADARG;
  if (D2 > HD_MAX_D2) return CWF_E_TOOLARGE;
  const int64_t V = (int64_t)D0 * D1 * D2;
  if (V >= ((int64_t)1 << 31) || (int64_t)D0 * D1 >= ((int64_t)1 << 31)) return CWF_E_TOOLARGE;
  L.border = 0;
  L.g = hd_align(L.border + 2 * (int64_t)B * V);
  L.compact = hd_align(L.g + 2 * V * 8);
  L.small = hd_align(L.compact + 2 * V * 8);
  L.range = hd_align(L.small + (int64_t)B * R * (int64_t)sizeof(HdSmall));
  L.total = hd_align(L.range + (int64_t)B * R * 4 * D2 * 4);
  L.lsum = L.total;
  L.lcnt = hd_align(L.lsum + 2 * (int64_t)D0 * D1 * 8);
  L.total_surface = hd_align(L.lcnt + 2 * (int64_t)D0 * D1 * HD_MAX_TAU * 4);
  return 0;
}

extern "C" int64_t cwf_hausdorff_workspace(int B, int R, int D0, int D1, int D2) {
  HdLayout L;
  const int rc = hd_layout(B, R, D0, D1, D2, L);
  return rc ? rc : L.total;
}

extern "C" int64_t cwf_surface_metrics_workspace(int B, int R, int D0, int D1, int D2) {
  HdLayout L;
  const int rc = hd_layout(B, R, D0, D1, D2, L);
  return rc ? rc : L.total_surface;
}

extern "C" int cwf_region_bits(const int64_t* labels, uint8_t* bits, int64_t n, void* stream) {
  if (!labels || !bits || n <= 0) return CWF_E_BADARG;
  hipLaunchKernelGGL(hd_region_bits_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, cwf_stream(stream), labels, bits, n);
  CWF_LAUNCH_CHECK();
  return 0;
}

// The launches of cwf_hausdorff; with surf, the surface variant of the gather pass and one more launch per (sample, region).
static int hd_run(const uint8_t* a, const uint8_t* b, int B, int R, int D0, int D1, int D2, double s0, double s1, double s2, int connectivity,
                  int all_border, double* hd, double* hd95, int64_t* counts, void* ws, int64_t ws_bytes, void* stream, bool surf,
                  const double* tau, int T, double* asd, double* assd, int64_t* within, double* nsd) {
  HdLayout L;
  const int rc = hd_layout(B, R, D0, D1, D2, L);
  if (rc) return rc;
  if (!a || !b || !hd || !hd95 || !counts || !ws || connectivity < 1 || connectivity > 3) return CWF_E_BADARG;
  if (!(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s0 < 1e300 && s1 < 1e300 && s2 < 1e300)) return CWF_E_BADARG;
  HdSurface sv = {};
  if (surf) {
    if (T < 0 || T > HD_MAX_TAU || !asd || !assd || (T > 0 && (!tau || !within || !nsd))) return CWF_E_BADARG;
    for (int j = 0; j < T; ++j) {
      if (!(tau[j] >= 0.0)) return CWF_E_BADARG;               // negative or NaN; +inf counts every border voxel
      sv.tau[j] = tau[j];
    }
    sv.T = T;
  }
  if (ws_bytes < (surf ? L.total_surface : L.total)) return CWF_E_TOOLARGE;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  uint8_t* w = (uint8_t*)ws;
  const int64_t V = (int64_t)D0 * D1 * D2, plane = (int64_t)D1 * D2, lines = (int64_t)D0 * D1;
  uint8_t* ba = w + L.border;
  uint8_t* bb = ba + (int64_t)B * V;
  double* g = (double*)(w + L.g);
  double* compact = (double*)(w + L.compact);
  HdSmall* small = (HdSmall*)(w + L.small);
  int* range = (int*)(w + L.range);
  if (surf) { sv.lsum = (double*)(w + L.lsum); sv.lcnt = (unsigned int*)(w + L.lcnt); }
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (surf) {
    const int64_t n0 = (int64_t)B * R * 4, n1 = (L.total - L.small) / 8;               // L.small and L.total are multiples of 256
    hipLaunchKernelGGL(hd_zero_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(n0 + n1, 256), 1024)), dim3(256), 0, st, cnt, n0,
                       reinterpret_cast<unsigned long long*>(w + L.small), n1);
    CWF_LAUNCH_CHECK();
  } else {
    if (hipMemsetAsync(counts, 0, (size_t)B * R * 4 * sizeof(int64_t), st) != hipSuccess) return (int)hipErrorInvalidValue;
    if (hipMemsetAsync(w + L.small, 0, (size_t)(L.total - L.small), st) != hipSuccess) return (int)hipErrorInvalidValue;
  }
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(V, 256), 1024);
  hipLaunchKernelGGL(hd_border_kernel, dim3(gx, B), dim3(256), 0, st, a, b, ba, bb, cnt, R, D0, D1, D2, connectivity, all_border);
  CWF_LAUNCH_CHECK();
  const int64_t cap = 2 * V;
  const unsigned gsel = (unsigned)std::min<int64_t>(cdiv64(cap, 256 * 16), 1024);
  for (int s = 0; s < B; ++s)
    for (int r = 0; r < R; ++r) {
      HdSmall* sm = small + (int64_t)s * R + r;
      int* rg = range + ((int64_t)s * R + r) * 4 * D2;
      hipLaunchKernelGGL(hd_edt_axis0_kernel, dim3((unsigned)cdiv64(plane, 256), 2), dim3(256), 0, st, ba + s * V, bb + s * V, r, D0, D1, D2, s0, g, rg);
      CWF_LAUNCH_CHECK();
      if (surf)
        hipLaunchKernelGGL(hd_edt_gather_kernel<true>, dim3((unsigned)lines, 2), dim3(64), (size_t)D2 * sizeof(double), st, ba + s * V, bb + s * V, r, D0, D1, D2,
                           s1, s2, (const double*)g, (const int*)rg, compact, cap, sm, sv);
      else
        hipLaunchKernelGGL(hd_edt_gather_kernel<false>, dim3((unsigned)lines, 2), dim3(64), (size_t)D2 * sizeof(double), st, ba + s * V, bb + s * V, r, D0, D1, D2,
                           s1, s2, (const double*)g, (const int*)rg, compact, cap, sm, sv);
      CWF_LAUNCH_CHECK();
      const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(compact);
      const unsigned long long* c = cnt + ((int64_t)s * R + r) * 4 + 2;          // |dA|, |dB|
      for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(hd_radix_kernel, dim3(gsel), dim3(256), 0, st, keys, cap, sm, pass, c, hd + s * R + r, hd95 + s * R + r);
        CWF_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(hd_radix_kernel, dim3(1), dim3(256), 0, st, keys, cap, sm, 8, c, hd + s * R + r, hd95 + s * R + r);
      CWF_LAUNCH_CHECK();
      if (surf) {
        const int64_t o = (int64_t)s * R + r;
        hipLaunchKernelGGL(hd_surface_final_kernel, dim3(1), dim3(1024), 0, st, sv, lines, c, asd + o * 2, assd + o,
                           reinterpret_cast<long long*>(within) + o * T * 2, nsd + o * T);
        CWF_LAUNCH_CHECK();
      }
    }
  return 0;
}

extern "C" int cwf_hausdorff(const uint8_t* a, const uint8_t* b, int B, int R, int D0, int D1, int D2, double s0, double s1, double s2,
                             int connectivity, int all_border, double* hd, double* hd95, int64_t* counts, void* ws, int64_t ws_bytes,
                             void* stream) {
  return hd_run(a, b, B, R, D0, D1, D2, s0, s1, s2, connectivity, all_border, hd, hd95, counts, ws, ws_bytes, stream, false, nullptr, 0,
                nullptr, nullptr, nullptr, nullptr);
}

extern "C" int cwf_surface_metrics(const uint8_t* a, const uint8_t* b, int B, int R, int D0, int D1, int D2, double s0, double s1, double s2,
                                   int connectivity, int all_border, const double* tau, int T, double* hd, double* hd95, double* asd,
                                   double* assd, int64_t* within, double* nsd, int64_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  return hd_run(a, b, B, R, D0, D1, D2, s0, s1, s2, connectivity, all_border, hd, hd95, counts, ws, ws_bytes, stream, true, tau, T, asd, assd,
                within, nsd);
}
