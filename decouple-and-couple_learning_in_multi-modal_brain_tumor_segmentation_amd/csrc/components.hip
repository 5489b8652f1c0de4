// N6 -- 3-D connected-component labelling of region-bit masks and the label-map post-processing policy built on it
// (predict_overlap.postprocess).  Block-based union-find on an int32 parent array that lives in the `labels` output itself:
//   parent[v] = -1 for background, otherwise the linear index of an earlier-or-equal voxel of the same component (parent[v] <= v), so
//   the root of a finished tree is the component's smallest linear index -- ranking the roots in index order is scipy's numbering.
//
//   cc_tile_kernel     one 16 x 16 x 32 tile per workgroup (32 KiB of LDS, five workgroups per CU): union-find in LDS over the
//                      backward half of the footprint, every voxel then written with its tile root's global index
//   cc_merge_kernel    voxels on tile faces: union with the backward neighbours that lie in another tile, on the global array
//   cc_flatten_kernel  parent[v] <- root; voxel counts added at the roots (one atomic per wave and root in the common case);
//                      roots per block of 2048 voxels counted
//   cc_scan_kernel     exclusive scan of the block counts, one workgroup per (sample, region) walking its own list; K
//   cc_rank_kernel     label of every root = block prefix + its rank in the block + 1; sizes scattered; the root's size slot is
//                      overwritten with its label; the largest component by a 64-bit max of size << 32 | ~label
//   cc_relabel_kernel  labels[v] <- label of parent[v]; largest unpacked
// A union is the lock-free "find both roots, atomicMin the larger root's parent to the smaller, retry from what was there" loop.
// A failed attempt strictly lowers the index it continues from, so every iteration makes progress whatever other threads do: no
// workgroup waits on another, nothing spins on a flag, no kernel needs a grid-wide barrier.  Links only ever join voxels of one
// component and every required link is eventually made, so the roots -- and with them every output -- do not depend on the order
// in which the atomics land.
#include <algorithm>
#include "common.h"

#define CC_T0 16
#define CC_T1 16
#define CC_T2 32
#define CC_TV (CC_T0 * CC_T1 * CC_T2)
#define CC_BLK 2048            // voxels per workgroup of the flatten / rank passes (256 threads x 8)

template <int SCOPE>
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

template <int SCOPE>
__device__ __forceinline__ int cc_find(const int* P, int x) {
  int p = cc_load<SCOPE>(P + x);
  while (p != x) { x = p; p = cc_load<SCOPE>(P + x); }
  return x;
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int* P, int a, int b) {
  for (;;) {
    a = cc_find<SCOPE>(P, a);
    b = cc_find<SCOPE>(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;          // a was still a root and now hangs under b
    a = old;                       // a had been linked meanwhile (old < a): join what it pointed to with b
  }
}

// is (d0, d1, d2) in the backward half of the connectivity-`conn` footprint (the neighbour's linear index is the smaller one)
__device__ __forceinline__ bool cc_backward(int d0, int d1, int d2, int conn) {
  const int nz = (d0 != 0) + (d1 != 0) + (d2 != 0);
  if (nz == 0 || nz > conn) return false;
  return d0 < 0 || (d0 == 0 && (d1 < 0 || (d1 == 0 && d2 < 0)));
}

__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ bits, int* __restrict__ parent, int R, int D0, int D1, int D2,
                                                      int nt1, int nt2, int conn) {
  __shared__ int lab[CC_TV];
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  const int tid = threadIdx.x;
  const int br = blockIdx.y, b = br / R, r = br % R;
  const int64_t V = (int64_t)D0 * D1 * D2;
  int t = blockIdx.x;
  const int o2 = (t % nt2) * CC_T2; t /= nt2;
  const int o1 = (t % nt1) * CC_T1;
  const int o0 = (t / nt1) * CC_T0;
  const uint8_t* bs = bits + (int64_t)b * V;
  int* P = parent + (int64_t)br * V;
  for (int li = tid; li < CC_TV; li += 256) {
    const int i2 = o2 + (li & (CC_T2 - 1)), i1 = o1 + ((li / CC_T2) & (CC_T1 - 1)), i0 = o0 + li / (CC_T2 * CC_T1);
    const bool inb = i0 < D0 && i1 < D1 && i2 < D2;
    const bool on = inb && ((bs[((int64_t)i0 * D1 + i1) * D2 + i2] >> r) & 1);
    lab[li] = on ? li : -1;
  }
  __syncthreads();
  for (int li = tid; li < CC_TV; li += 256) {
    if (cc_load<WG>(lab + li) < 0) continue;                  // background stays -1 throughout
    const int l2 = li & (CC_T2 - 1), l1 = (li / CC_T2) & (CC_T1 - 1), l0 = li / (CC_T2 * CC_T1);
#pragma unroll
    for (int d0 = -1; d0 <= 0; ++d0)
#pragma unroll
      for (int d1 = -1; d1 <= 1; ++d1)
#pragma unroll
        for (int d2 = -1; d2 <= 1; ++d2) {
          if (!cc_backward(d0, d1, d2, conn)) continue;
          const int m0 = l0 + d0, m1 = l1 + d1, m2 = l2 + d2;
          if (m0 < 0 || m1 < 0 || m1 >= CC_T1 || m2 < 0 || m2 >= CC_T2) continue;
          const int nl = (m0 * CC_T1 + m1) * CC_T2 + m2;
          if (cc_load<WG>(lab + nl) < 0) continue;
          cc_union<WG>(lab, li, nl);
        }
  }
  __syncthreads();
  for (int li = tid; li < CC_TV; li += 256) {                 // read-only on lab from here
    const int i2 = o2 + (li & (CC_T2 - 1)), i1 = o1 + ((li / CC_T2) & (CC_T1 - 1)), i0 = o0 + li / (CC_T2 * CC_T1);
    if (i0 >= D0 || i1 >= D1 || i2 >= D2) continue;
    int g = -1;
    if (lab[li] >= 0) {
      const int root = cc_find<WG>(lab, li);
      const int r2 = o2 + (root & (CC_T2 - 1)), r1 = o1 + ((root / CC_T2) & (CC_T1 - 1)), r0 = o0 + root / (CC_T2 * CC_T1);
      g = (int)(((int64_t)r0 * D1 + r1) * D2 + r2);
    }
    P[((int64_t)i0 * D1 + i1) * D2 + i2] = g;
  }
}

// One thread per voxel of one sample (blockIdx.y); all regions of the voxel's byte.
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* __restrict__ bits, int* __restrict__ parent, int R, int D0, int D1, int D2,
                                                       int conn) {
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  const int64_t V = (int64_t)D0 * D1 * D2;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const int b = blockIdx.y;
  const int i2 = (int)(v % D2);
  const int64_t q = v / D2;
  const int i1 = (int)(q % D1), i0 = (int)(q / D1);
  const int l0 = i0 & (CC_T0 - 1), l1 = i1 & (CC_T1 - 1), l2 = i2 & (CC_T2 - 1);
  if (l0 != 0 && l0 != CC_T0 - 1 && l1 != 0 && l1 != CC_T1 - 1 && l2 != 0 && l2 != CC_T2 - 1) return;
  const uint8_t* bs = bits + (int64_t)b * V;
  const unsigned m = bs[v];
  if (!m) return;
  for (int d0 = -1; d0 <= 0; ++d0)
    for (int d1 = -1; d1 <= 1; ++d1)
      for (int d2 = -1; d2 <= 1; ++d2) {
        if (!cc_backward(d0, d1, d2, conn)) continue;
        const int j0 = i0 + d0, j1 = i1 + d1, j2 = i2 + d2;
        if (j0 < 0 || j1 < 0 || j1 >= D1 || j2 < 0 || j2 >= D2) continue;
        if (j0 / CC_T0 == i0 / CC_T0 && j1 / CC_T1 == i1 / CC_T1 && j2 / CC_T2 == i2 / CC_T2) continue;     // the tile pass joined these
        const int64_t nv = ((int64_t)j0 * D1 + j1) * D2 + j2;
        const unsigned mn = m & bs[nv];
        for (int r = 0; r < R; ++r)
          if ((mn >> r) & 1u) cc_union<AG>(parent + ((int64_t)b * R + r) * V, (int)v, (int)nv);
      }
}

__device__ __forceinline__ int cc_block_sum(int x, int* red) {     // 256 threads; red[4]
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Every lane of a wave runs all eight rounds (the ballots and shuffles need them all).
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int* __restrict__ rsize, int* __restrict__ bsum, int64_t V,
                                                         int nblk) {
  __shared__ int red[4];
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  const int br = blockIdx.y, lane = threadIdx.x & 63;
  int* P = parent + (int64_t)br * V;
  int* S = rsize + (int64_t)br * V;
  int nroots = 0;
  for (int k = 0; k < CC_BLK / 256; ++k) {
    const int64_t v = (int64_t)blockIdx.x * CC_BLK + k * 256 + threadIdx.x;
    const int p = v < V ? cc_load<AG>(P + v) : -1;
    const bool on = p >= 0;
    int root = -1;
    if (on) {
      root = p == (int)v ? p : cc_find<AG>(P, p);
      if (root != p) __hip_atomic_store(P + v, root, __ATOMIC_RELAXED, AG);
      nroots += root == (int)v;
    }
    const unsigned long long mask = __ballot(on);
    if (mask) {                                               // wave-uniform
      const int first = __ffsll((long long)mask) - 1;
      const int r0 = __shfl(root, first, 64);
      const bool same = on && root == r0;
      const unsigned long long ms = __ballot(same);
      if (lane == first) atomicAdd(S + r0, (int)__popcll(ms));
      else if (on && !same) atomicAdd(S + root, 1);
    }
  }
  const int total = cc_block_sum(nroots, red);
  if (threadIdx.x == 0) bsum[(int64_t)br * nblk + blockIdx.x] = total;
}

// One workgroup per (sample, region): bsum <- its exclusive scan, count <- the total.  It walks its own list and waits on nobody.
__global__ __launch_bounds__(256) void cc_scan_kernel(int* __restrict__ bsum, int nblk, int* __restrict__ count) {
  __shared__ int sc[256];
  __shared__ int carry;
  const int tid = threadIdx.x;
  int* s = bsum + (int64_t)blockIdx.x * nblk;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + tid;
    const int x = i < nblk ? s[i] : 0;
    sc[tid] = x;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int add = tid >= off ? sc[tid - off] : 0;
      __syncthreads();
      sc[tid] += add;
      __syncthreads();
    }
    const int incl = sc[tid], c = carry;
    if (i < nblk) s[i] = c + incl - x;
    __syncthreads();
    if (tid == 255) carry = c + incl;
    __syncthreads();
  }
  if (tid == 0) count[blockIdx.x] = carry;
}

// Thread t owns voxels [8 t, 8 t + 8) of the block, so ranks follow the linear index.
__global__ __launch_bounds__(256) void cc_rank_kernel(const int* __restrict__ parent, int* __restrict__ rsize, const int* __restrict__ bsum,
                                                      int* __restrict__ sizes, unsigned long long* __restrict__ packed, int64_t V, int nblk,
                                                      int64_t cap) {
  __shared__ int wsum[4];
  __shared__ unsigned long long wbest[4];
  const int br = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* P = parent + (int64_t)br * V;
  int* S = rsize + (int64_t)br * V;
  const int64_t v0 = (int64_t)blockIdx.x * CC_BLK + (int64_t)tid * 8;
  unsigned flags = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t v = v0 + j;
    if (v < V && P[v] == (int)v) flags |= 1u << j;
  }
  const int c = __popc(flags);
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int lab = bsum[(int64_t)br * nblk + blockIdx.x] + incl - c;
  for (int w = 0; w < wave; ++w) lab += wsum[w];
  unsigned long long best = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (!((flags >> j) & 1u)) continue;
    const int64_t v = v0 + j;
    ++lab;                                                    // 1-based label of this root
    const int sz = S[v];
    if (lab - 1 < cap) sizes[(int64_t)br * cap + lab - 1] = sz;
    S[v] = lab;
    const unsigned long long key = ((unsigned long long)(unsigned)sz << 32) | (unsigned)~(unsigned)lab;
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(best, o, 64);
    best = y > best ? y : best;
  }
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
    if (best) atomicMax(packed + br, best);
  }
}

__global__ __launch_bounds__(256) void cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ rsize,
                                                         const unsigned long long* __restrict__ packed, int* __restrict__ largest, int64_t V) {
  const int br = blockIdx.y;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < V) {
    const int p = labels[(int64_t)br * V + v];                // flattened: the root, whose size slot now holds its label
    labels[(int64_t)br * V + v] = p >= 0 ? rsize[(int64_t)br * V + p] : 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long key = packed[br];
    const int sz = (int)(key >> 32);
    largest[br * 2 + 0] = sz ? (int)~(unsigned)key : 0;
    largest[br * 2 + 1] = sz;
  }
}

static inline int64_t cc_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Workspace layout: rsize [B][R][V] ints | bsum [B][R][nblk] ints | packed [B][R] uint64
struct CcLayout { int64_t rsize, bsum, packed, total; int nblk; };
static int cc_layout(int B, int R, int D0, int D1, int D2, CcLayout& L) {
  if (B <= 0 || R <= 0 || R > 8 || D0 <= 0 || D1 <= 0 || D2 <= 0) return CWF_E_BADARG;
  const int64_t V = (int64_t)D0 * D1 * D2;
  if (V >= ((int64_t)1 << 31) || (int64_t)B * R > 65535) return CWF_E_TOOLARGE;
  L.nblk = (int)cdiv64(V, CC_BLK);
  L.rsize = 0;
  L.bsum = cc_align(L.rsize + (int64_t)B * R * V * 4);
  L.packed = cc_align(L.bsum + (int64_t)B * R * L.nblk * 4);
  L.total = cc_align(L.packed + (int64_t)B * R * 8);
  return 0;
}

extern "C" int64_t cwf_components_workspace(int B, int R, int D0, int D1, int D2) {
  CcLayout L;
  const int rc = cc_layout(B, R, D0, D1, D2, L);
  return rc ? rc : L.total;
}

extern "C" int cwf_components(const uint8_t* bits, int B, int R, int D0, int D1, int D2, int connectivity, int32_t* labels, int32_t* sizes,
                              int32_t* count, int32_t* largest, void* ws, int64_t ws_bytes, void* stream) {
  CcLayout L;
  const int rc = cc_layout(B, R, D0, D1, D2, L);
  if (rc) return rc;
  if (!bits || !labels || !sizes || !count || !largest || !ws || connectivity < 1 || connectivity > 3) return CWF_E_BADARG;
  if (ws_bytes < L.total) return CWF_E_TOOLARGE;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  uint8_t* w = (uint8_t*)ws;
  const int64_t V = (int64_t)D0 * D1 * D2, cap = (V + 1) / 2;
  int* rsize = (int*)(w + L.rsize);
  int* bsum = (int*)(w + L.bsum);
  unsigned long long* packed = (unsigned long long*)(w + L.packed);
  const int BR = B * R;
  if (hipMemsetAsync(rsize, 0, (size_t)BR * V * 4, st) != hipSuccess) return (int)hipErrorInvalidValue;
  if (hipMemsetAsync(packed, 0, (size_t)BR * 8, st) != hipSuccess) return (int)hipErrorInvalidValue;
  if (hipMemsetAsync(sizes, 0, (size_t)BR * cap * 4, st) != hipSuccess) return (int)hipErrorInvalidValue;
  const int nt0 = cdiv(D0, CC_T0), nt1 = cdiv(D1, CC_T1), nt2 = cdiv(D2, CC_T2);
  const int64_t ntiles = (int64_t)nt0 * nt1 * nt2;               // < 2^31 as V is
  const unsigned gv = (unsigned)cdiv64(V, 256);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)ntiles, BR), dim3(256), 0, st, bits, labels, R, D0, D1, D2, nt1, nt2, connectivity);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_merge_kernel, dim3(gv, B), dim3(256), 0, st, bits, labels, R, D0, D1, D2, connectivity);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)L.nblk, BR), dim3(256), 0, st, labels, rsize, bsum, V, L.nblk);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_scan_kernel, dim3(BR), dim3(256), 0, st, bsum, L.nblk, count);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)L.nblk, BR), dim3(256), 0, st, (const int*)labels, rsize, (const int*)bsum, sizes, packed, V,
                     L.nblk, cap);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_relabel_kernel, dim3(gv, BR), dim3(256), 0, st, labels, (const int*)rsize, (const unsigned long long*)packed, largest, V);
  CWF_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ the post-processing policy
struct PpArgs {
  int R, wt, et, min_component, keep_largest, et_min_component, et_min_voxels, et_replace;
  int64_t V, cap;
};

// wave sums of up to four counters, one atomic per wave and non-zero counter
template <int N>
__device__ __forceinline__ void pp_wave_add(unsigned long long* acc, const int (&c)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    int x = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(acc + j, (unsigned long long)x);
  }
}

// Rules 1-3 per voxel, and per WT component (threads i < cap look at sizes[i] as well).  acc[b][4] = WT voxels removed, WT components
// removed, ET voxels relabelled by rule 3, ET voxels left for rule 4.  One sample per blockIdx.y; no early return (wave sums).
__global__ __launch_bounds__(256) void pp_rules_kernel(const int64_t* __restrict__ seg_in, int64_t* __restrict__ seg_out, const int* __restrict__ labels,
                                                       const int* __restrict__ sizes, const int* __restrict__ largest, PpArgs a,
                                                       unsigned long long* __restrict__ acc) {
  const int b = blockIdx.y;
  const int* lwt = labels + ((int64_t)b * a.R + a.wt) * a.V;
  const int* let = labels + ((int64_t)b * a.R + a.et) * a.V;
  const int* swt = sizes + ((int64_t)b * a.R + a.wt) * a.cap;
  const int* set = sizes + ((int64_t)b * a.R + a.et) * a.cap;
  const int keep = a.keep_largest ? largest[((int64_t)b * a.R + a.wt) * 2] : 0;
  int c[4] = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.V; i += (int64_t)gridDim.x * 256) {
    int64_t s = seg_in[(int64_t)b * a.V + i];
    if (s > 0 && (a.min_component > 0 || a.keep_largest)) {
      const int l = lwt[i];
      const bool gone = l <= 0 || (a.min_component > 0 && swt[l - 1] < a.min_component) || (a.keep_largest && l != keep);
      if (gone) { s = 0; ++c[0]; }
    }
    if (s == 3 && a.et_min_component > 0) {
      const int l = let[i];
      if (l > 0 && set[l - 1] < a.et_min_component) { s = a.et_replace; ++c[2]; }
    }
    c[3] += s == 3;
    seg_out[(int64_t)b * a.V + i] = s;
    if (i < a.cap && (a.min_component > 0 || a.keep_largest)) {
      const int sz = swt[i];                                  // component i + 1, 0 beyond the last
      c[1] += sz > 0 && ((a.min_component > 0 && sz < a.min_component) || (a.keep_largest && (int)i + 1 != keep));
    }
  }
  pp_wave_add<4>(acc + b * 4, c);
}

// Rule 4 from the device-side count, and the stats.  With et_min_voxels == 0 it is launched with one workgroup per sample.
__global__ __launch_bounds__(256) void pp_rule4_kernel(int64_t* __restrict__ seg_out, PpArgs a, const unsigned long long* __restrict__ acc,
                                                       int64_t* __restrict__ stats) {
  const int b = blockIdx.y;
  const unsigned long long left = acc[b * 4 + 3];
  const bool all = a.et_min_voxels > 0 && left < (unsigned long long)a.et_min_voxels;
  if (all)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.V; i += (int64_t)gridDim.x * 256)
      if (seg_out[(int64_t)b * a.V + i] == 3) seg_out[(int64_t)b * a.V + i] = a.et_replace;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[b * 4 + 0] = (int64_t)acc[b * 4 + 0];
    stats[b * 4 + 1] = (int64_t)acc[b * 4 + 1];
    stats[b * 4 + 2] = (int64_t)(acc[b * 4 + 2] + (all ? left : 0ull));
    stats[b * 4 + 3] = (int64_t)(all ? 0ull : left);
  }
}

extern "C" int cwf_postprocess_labels(const int64_t* seg_in, int64_t* seg_out, const int32_t* labels, const int32_t* sizes, const int32_t* largest,
                                      int B, int R, int D0, int D1, int D2, int wt_region, int et_region, int min_component, int keep_largest,
                                      int et_min_component, int et_min_voxels, int et_replace, int64_t* stats, void* ws, void* stream) {
  if (B <= 0 || B > 65535 || R <= 0 || R > 8 || D0 <= 0 || D1 <= 0 || D2 <= 0) return CWF_E_BADARG;
  const int64_t V = (int64_t)D0 * D1 * D2;
  if (V >= ((int64_t)1 << 31)) return CWF_E_TOOLARGE;
  if (!seg_in || !seg_out || !labels || !sizes || !largest || !stats || !ws) return CWF_E_BADARG;
  if (wt_region < 0 || wt_region >= R || et_region < 0 || et_region >= R) return CWF_E_BADARG;
  if (min_component < 0 || et_min_component < 0 || et_min_voxels < 0 || et_replace < 0 || et_replace > 2) return CWF_E_BADARG;
  if ((uintptr_t)ws & 7) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  unsigned long long* acc = (unsigned long long*)ws;
  if (hipMemsetAsync(acc, 0, (size_t)B * 32, st) != hipSuccess) return (int)hipErrorInvalidValue;
  PpArgs a = {R, wt_region, et_region, min_component, keep_largest != 0, et_min_component, et_min_voxels, et_replace, V, (V + 1) / 2};
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(V, 256), 2048);
  hipLaunchKernelGGL(pp_rules_kernel, dim3(gx, B), dim3(256), 0, st, seg_in, seg_out, labels, sizes, largest, a, acc);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pp_rule4_kernel, dim3(et_min_voxels > 0 ? gx : 1u, B), dim3(256), 0, st, seg_out, a, (const unsigned long long*)acc, stats);
  CWF_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ Dice / IoU counts of a label map
__global__ __launch_bounds__(256) void label_metrics_kernel(const int64_t* __restrict__ seg, const int64_t* __restrict__ target,
                                                            unsigned long long* __restrict__ counts, int64_t n) {
  int c[18];
#pragma unroll
  for (int j = 0; j < 18; ++j) c[j] = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t o = seg[i], t = target[i];
    const bool ro[6] = {o > 0, o == 1 || o == 3, o == 3, o == 1, o == 2, o == 3};
    const bool rt[6] = {t > 0, t == 1 || t == 3, t == 3, t == 1, t == 2, t == 3};
#pragma unroll
    for (int j = 0; j < 6; ++j) { c[j * 3] += ro[j] && rt[j]; c[j * 3 + 1] += ro[j]; c[j * 3 + 2] += rt[j]; }
  }
  pp_wave_add<18>(counts, c);
}

extern "C" int cwf_label_metrics(const int64_t* seg, const int64_t* target, uint64_t* counts, int64_t n, void* stream) {
  if (!seg || !target || !counts || n <= 0) return CWF_E_BADARG;
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(n, 256), 2048);      // at most 2^31 / (2048 * 256) rounds: an int counter holds it
  if (cdiv64(n, (int64_t)gx * 256) >= ((int64_t)1 << 31)) return CWF_E_TOOLARGE;
  hipLaunchKernelGGL(label_metrics_kernel, dim3(gx), dim3(256), 0, cwf_stream(stream), seg, target,
                     reinterpret_cast<unsigned long long*>(counts), n);
  CWF_LAUNCH_CHECK();
  return 0;
}
