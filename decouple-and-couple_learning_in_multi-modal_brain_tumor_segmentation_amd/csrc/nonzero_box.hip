// N9 -- the nonzero bounding box of a four-channel volume ("Nonzero box"): where the skull-stripped brain lies inside a
// BraTS volume.  The integer statement (restated in tests/nonzero_box_ref.py):
//   x       fp32 [B][4][S0][S1][S2], sample b at x + b * bstride floats, its four channels contiguous; V = S0 S1 S2.
//   nonzero voxel v of sample b is nonzero iff (bits & 0x7fffffff) != 0 for the bits of some channel: +-0 is background; denormals,
//           infinities and NaN are not.  The bits are tested, so the kernel's denormal mode cannot matter.
//   box     box[b] = lo0, lo1, lo2, hi0, hi1, hi2 (int32, hi exclusive): the tightest box holding every nonzero voxel.
//   count   count[b] = the number of nonzero voxels (int64).  A sample without one has lo = S, hi = 0, count = 0.
//
// Two launches on one stream:
//   nzb_tile_kernel      blockIdx = (tile g, sample b).  A workgroup of 256 lanes owns NZB_TILE consecutive voxel positions, counted from
//                        the 16-byte boundary at or below the sample's first float; a lane owns NZB_RUNS runs of four consecutive
//                        positions, run k of lane t at position (k * 256 + t) * 4 of the tile, so one load instruction of a wave reads 1 KiB
//                        in a row.  A run that lies wholly inside the volume is one 16-byte load per channel whose plane is congruent
//                        to the first mod 16 bytes (c V a multiple of 4: all four for a BraTS volume), four 4-byte loads otherwise; a run
//                        that the head or the tail of the volume cuts is read float by float, positions outside the volume read as
//                        zero.  The four channels are ORed before the one test per voxel.  A lane divides twice, for the coordinates
//                        of its first run; from run to run and from voxel to voxel the coordinates are carried like an odometer, so
//                        tiles need not hold whole rows and rows of any length (S2 = 1 too) cost the same.  Lane minima / maxima
//                        and the count are reduced over the wave by shuffles and over the four waves through LDS; the workgroup
//                        stores its eight words part[b][g][0..7] = lo[3], hi[3], count, 0 with plain stores.
//   nzb_finalize_kernel  one workgroup per sample reduces part[b][.] in a fixed order and writes box[b] and count[b].
// No atomics, no host synchronisation, nothing read back, no kernel waits on another workgroup: capturable.  ws may hold anything (the
// first launch rewrites every word the second reads); box and count are fully written; the result depends on nothing but x.
#include "common.h"

#define NZB_THREADS 256
#define NZB_RUNS 4                                    // runs of one lane: 16 loads of 16 bytes in flight with four aligned channels
#define NZB_TILE (NZB_THREADS * NZB_RUNS * 4)         // 4096 voxel positions (64 KiB of x) of one workgroup

static_assert(NZB_TILE == CWF_NONZERO_BOX_TILE, "the header states the tile");

struct nzb_coord { int i0, i1, i2; };

// c + d in the mixed radix (S0, S1, S2); d < S component-wise.  i0 may pass S0 only beyond the last voxel, where nothing is nonzero.
__device__ __forceinline__ nzb_coord nzb_add(nzb_coord c, nzb_coord d, int S1, int S2) {
  c.i2 += d.i2;
  int carry = c.i2 >= S2;
  c.i2 -= carry ? S2 : 0;
  c.i1 += d.i1 + carry;
  carry = c.i1 >= S1;
  c.i1 -= carry ? S1 : 0;
  c.i0 += d.i0 + carry;
  return c;
}

__device__ __forceinline__ nzb_coord nzb_split(uint32_t v, int S1, int S2) {
  const uint32_t row = v / (uint32_t)S2;
  nzb_coord c;
  c.i2 = (int)(v - row * (uint32_t)S2);
  c.i0 = (int)(row / (uint32_t)S1);
  c.i1 = (int)(row - (uint32_t)c.i0 * (uint32_t)S1);
  return c;
}

__global__ __launch_bounds__(NZB_THREADS) void nzb_tile_kernel(const float* __restrict__ x, int64_t bstride, int S0, int S1, int S2, int64_t V,
                                                               nzb_coord step, int32_t* __restrict__ part) {
  __shared__ int32_t red[NZB_THREADS / 64][8];
  const uint32_t* __restrict__ xb = reinterpret_cast<const uint32_t*>(x) + (int64_t)blockIdx.y * bstride;
  const int shift = (int)(((uintptr_t)xb >> 2) & 3);                // positions [shift, shift + V) hold voxels
  bool vec[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) vec[c] = (((int64_t)c * V) & 3) == 0;  // the plane of channel c is congruent to the first mod 16 bytes
  const int64_t p0 = (int64_t)blockIdx.x * NZB_TILE + (int64_t)threadIdx.x * 4 - shift;     // the linear index of run 0's first position

  // every load first, the four channels ORed: w[k][e] != 0 iff voxel p0 + k * 1024 + e exists and is nonzero
  uint32_t w[NZB_RUNS][4];
#pragma unroll
  for (int k = 0; k < NZB_RUNS; ++k) {
    const int64_t v = p0 + (int64_t)k * (NZB_THREADS * 4);
    w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0u;
    if (v + 4 <= 0 || v >= V) continue;
    const bool whole = v >= 0 && v + 4 <= V;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t* src = xb + (int64_t)c * V + v;
      if (whole && vec[c]) {
        const uint4 q = *reinterpret_cast<const uint4*>(src);       // 16-byte aligned: xb + v is, and c V is a multiple of 4
        w[k][0] |= q.x; w[k][1] |= q.y; w[k][2] |= q.z; w[k][3] |= q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v + e >= 0 && v + e < V) w[k][e] |= src[e];
      }
    }
  }

  int lo0 = S0, lo1 = S1, lo2 = S2, hi0 = 0, hi1 = 0, hi2 = 0, cnt = 0;
  nzb_coord at = nzb_split((uint32_t)(p0 > 0 ? (p0 < V ? p0 : V - 1) : 0), S1, S2);
#pragma unroll
  for (int k = 0; k < NZB_RUNS; ++k) {
    const int64_t v = p0 + (int64_t)k * (NZB_THREADS * 4);
    nzb_coord c = at;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (v + e < 0) continue;                                       // in front of voxel 0 (the head run alone): c stays at (0, 0, 0)
      if (w[k][e] & 0x7fffffffu) {
        lo0 = min(lo0, c.i0); lo1 = min(lo1, c.i1); lo2 = min(lo2, c.i2);
        hi0 = max(hi0, c.i0 + 1); hi1 = max(hi1, c.i1 + 1); hi2 = max(hi2, c.i2 + 1);
        ++cnt;
      }
      int carry = ++c.i2 >= S2;
      c.i2 = carry ? 0 : c.i2;
      c.i1 += carry;
      carry = c.i1 >= S1;
      c.i1 = carry ? 0 : c.i1;
      c.i0 += carry;
    }
    if (k + 1 < NZB_RUNS) {
      const int64_t nv = v + NZB_THREADS * 4;
      if (v < 0) at = nzb_split((uint32_t)(nv < V ? nv : V - 1), S1, S2);      // the head run started in front of voxel 0
      else at = nzb_add(at, step, S1, S2);
    }
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo0 = min(lo0, __shfl_xor(lo0, o, 64)); lo1 = min(lo1, __shfl_xor(lo1, o, 64)); lo2 = min(lo2, __shfl_xor(lo2, o, 64));
    hi0 = max(hi0, __shfl_xor(hi0, o, 64)); hi1 = max(hi1, __shfl_xor(hi1, o, 64)); hi2 = max(hi2, __shfl_xor(hi2, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    int32_t* r = red[threadIdx.x >> 6];
    r[0] = lo0; r[1] = lo1; r[2] = lo2; r[3] = hi0; r[4] = hi1; r[5] = hi2; r[6] = cnt; r[7] = 0;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int f = threadIdx.x;
    int32_t s = red[0][f];
#pragma unroll
    for (int k = 1; k < NZB_THREADS / 64; ++k) {
      const int32_t t = red[k][f];
      s = f < 3 ? min(s, t) : (f < 6 ? max(s, t) : s + t);
    }
    part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + f] = s;
  }
}

// blockIdx.x = sample b: part[b][0 .. G) -> box[b][6], count[b]
__global__ __launch_bounds__(NZB_THREADS) void nzb_finalize_kernel(const int32_t* __restrict__ part, int G, int S0, int S1, int S2,
                                                                   int32_t* __restrict__ box, int64_t* __restrict__ count) {
  __shared__ int32_t red[NZB_THREADS / 64][6];
  __shared__ int64_t redc[NZB_THREADS / 64];
  const int32_t* p = part + (int64_t)blockIdx.x * G * 8;
  int lo0 = S0, lo1 = S1, lo2 = S2, hi0 = 0, hi1 = 0, hi2 = 0;
  int64_t cnt = 0;
  for (int g = threadIdx.x; g < G; g += NZB_THREADS) {
    const int4 a = *reinterpret_cast<const int4*>(p + (int64_t)g * 8), b = *reinterpret_cast<const int4*>(p + (int64_t)g * 8 + 4);
    lo0 = min(lo0, a.x); lo1 = min(lo1, a.y); lo2 = min(lo2, a.z);
    hi0 = max(hi0, a.w); hi1 = max(hi1, b.x); hi2 = max(hi2, b.y);
    cnt += b.z;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo0 = min(lo0, __shfl_xor(lo0, o, 64)); lo1 = min(lo1, __shfl_xor(lo1, o, 64)); lo2 = min(lo2, __shfl_xor(lo2, o, 64));
    hi0 = max(hi0, __shfl_xor(hi0, o, 64)); hi1 = max(hi1, __shfl_xor(hi1, o, 64)); hi2 = max(hi2, __shfl_xor(hi2, o, 64));
    const uint32_t l = (uint32_t)__shfl_xor((int)(uint32_t)cnt, o, 64), h = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)cnt >> 32), o, 64);
    cnt += (int64_t)(((uint64_t)h << 32) | l);
  }
  if ((threadIdx.x & 63) == 0) {
    int32_t* r = red[threadIdx.x >> 6];
    r[0] = lo0; r[1] = lo1; r[2] = lo2; r[3] = hi0; r[4] = hi1; r[5] = hi2;
    redc[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int f = threadIdx.x;
    int32_t s = red[0][f];
#pragma unroll
    for (int k = 1; k < NZB_THREADS / 64; ++k) s = f < 3 ? min(s, red[k][f]) : max(s, red[k][f]);
    box[(int64_t)blockIdx.x * 6 + f] = s;
  }
  if (threadIdx.x == 6) {
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < NZB_THREADS / 64; ++k) s += redc[k];
    count[blockIdx.x] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t nzb_tiles(int64_t V) { return cdiv64(V + 3, NZB_TILE); }       // the head may shift the volume by up to 3 positions

static int nzb_check(int B, int S0, int S1, int S2) {
  if (B < 1 || S0 < 1 || S1 < 1 || S2 < 1) return CWF_E_BADARG;
  if ((int64_t)S0 * S1 > 0x7fffffffll || (int64_t)S0 * S1 * S2 > 0x7fffffffll || B > 65535) return CWF_E_TOOLARGE;
  return 0;
}

extern "C" int64_t cwf_nonzero_box_workspace(int B, int S0, int S1, int S2) {
  const int rc = nzb_check(B, S0, S1, S2);
  if (rc) return rc;
  return ((int64_t)B * nzb_tiles((int64_t)S0 * S1 * S2) * 8 * (int64_t)sizeof(int32_t) + 255) & ~(int64_t)255;
}

extern "C" int cwf_nonzero_box(const float* x, int64_t bstride, int B, int S0, int S1, int S2, int32_t* box, int64_t* count, void* ws,
                               void* stream) {
  const int rc = nzb_check(B, S0, S1, S2);
  if (rc) return rc;
  const int64_t V = (int64_t)S0 * S1 * S2;
  if (!x || !box || !count || !ws || bstride < 4 * V) return CWF_E_BADARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)box & 3) || ((uintptr_t)count & 7) || ((uintptr_t)ws & 255)) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  const int G = (int)nzb_tiles(V);
  const int64_t run = NZB_THREADS * 4;                                 // a lane's runs lie this many voxels apart
  nzb_coord step;
  step.i2 = (int)(run % S2);
  step.i1 = (int)((run / S2) % S1);
  step.i0 = (int)(run / S2 / S1);
  int32_t* part = (int32_t*)ws;
  hipLaunchKernelGGL(nzb_tile_kernel, dim3((unsigned)G, (unsigned)B), dim3(NZB_THREADS), 0, st, x, bstride, S0, S1, S2, V, step, part);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(nzb_finalize_kernel, dim3((unsigned)B), dim3(NZB_THREADS), 0, st, part, G, S0, S1, S2, box, count);
  CWF_LAUNCH_CHECK();
  return 0;
}
