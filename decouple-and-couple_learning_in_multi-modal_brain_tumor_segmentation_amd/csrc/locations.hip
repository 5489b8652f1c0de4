// N4 -- per-subject class location tables for foreground-oversampled training crops ("Foreground oversampling").
// The integer statement (restated in tests/foreground_ref.py):
//   label   uint8 [V], C-order linear index v.  Values 0..4 are classes, 4 read as 3; any other value belongs to no region.
//   region  r is a class bitmask posmasks[r] over classes 0..3, 1 <= R <= 8; regions may overlap.
//   counts  counts[r] = n_r, the number of voxels of region r (int64).
//   table   with m_r = min(n_r, K): table[r][j] for j < m_r is the linear index of the region voxel of rank floor(j n_r / m_r), ranks
//           counted in increasing linear index; table[r][j] = -1 for j >= m_r (int32 [R][K]).  With n_r <= K that is every voxel of the
//           region, otherwise an evenly ranked sample.
// A voxel of rank p is entry j = ceil(p m / n) iff j < m and floor(j n / m) == p, so every voxel decides for itself and the result
// depends on nothing but the label: not on the launch geometry, and there is no atomic whose order could matter.
//
// Three launches on one stream:
//   loc_count_kernel   a workgroup of 256 lanes owns one tile of LOC_TILE consecutive voxels, a lane LOC_LANE (64) consecutive ones, so
//                      lane order is linear order.  Tiles are laid out from the 16-byte boundary at or below `label`: a 16-byte run that
//                      lies wholly inside the volume is one vector load, a run that the head or the tail of the volume cuts is read byte
//                      by byte, and bytes outside the volume belong to no region.  Every label becomes a membership byte (bit r: the voxel
//                      is in region r) through a 5-entry table packed in 64 bits; a lane keeps one 64-bit voxel mask per region.  The
//                      per-lane popcounts travel as 16-bit fields of 64-bit words (a tile holds 2^14 voxels), are summed over the wave by
//                      shuffles and over the four waves through LDS; the workgroup stores part[g][r] with plain stores.
//   loc_scan_kernel    one workgroup turns part[.][r] into its exclusive prefix in place (a region holds fewer than 2^31 voxels, so 32
//                      bits are exact), writes counts[r] and the -1 entries table[r][m_r .. K).
//   loc_select_kernel  the same tiles and masks again; a lane's exclusive in-tile prefix per region comes from a wave scan of the packed
//                      words plus LDS across the waves, so the rank of its k-th region voxel is part[g][r] + prefix + k.  With n <= K the
//                      entry is the rank itself; otherwise the lane takes one ceil / floor pair in 64 bits for its first entry and steps
//                      j, quotient and remainder from there (n > m: the ranks of successive entries are strictly increasing).
// No atomics, no host synchronisation, nothing read back, no kernel waits on another workgroup: capturable.  ws may hold anything (the
// count kernel rewrites every word that is read later); counts and table are fully written.  Vector stores only.
#include "common.h"

#define LOC_THREADS 256
#define LOC_LANE 64                          // voxels of one lane: four 16-byte runs, one 64-bit mask per region
#define LOC_TILE (LOC_THREADS * LOC_LANE)    // 16384 voxels of one workgroup (cwf/_lib.py: LOCATIONS_TILE)
#define LOC_MAX_R 8
#define LOC_SCAN_THREADS 1024

static_assert(LOC_TILE == CWF_LOCATIONS_TILE, "the header states the tile");
static_assert(LOC_TILE < 65536, "in-tile counts travel in 16-bit fields");

__device__ __forceinline__ uint64_t loc_shfl_up(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t loc_shfl_xor(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

// membership bytes of four labels held in one 32-bit word; tab: byte c = the regions of class c (c = 4 repeats 3), bytes 5.. are 0
__device__ __forceinline__ uint32_t loc_member4(uint32_t w, uint64_t tab) {
  uint32_t out = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t lab = min((w >> (8 * b)) & 0xffu, 5u);
    out |= ((uint32_t)(tab >> (8 * lab)) & 0xffu) << (8 * b);
  }
  return out;
}

// The per-region voxel masks of this lane's LOC_LANE voxels of tile g: bit i of m[r] = voxel (g * LOC_TILE + lane * LOC_LANE + i - shift)
// is in region r.  shift = (address of label) & 15: positions count from the 16-byte boundary below the volume.
template <int NR>
__device__ __forceinline__ void loc_masks(const uint8_t* __restrict__ label, int64_t V, int shift, int64_t p0, uint64_t tab, uint64_t (&m)[NR]) {
#pragma unroll
  for (int r = 0; r < NR; ++r) m[r] = 0ull;
  const int64_t lo = shift, hi = (int64_t)shift + V;       // positions [lo, hi) hold voxels
#pragma unroll
  for (int run = 0; run < LOC_LANE / 16; ++run) {
    const int64_t p = p0 + run * 16;
    if (p + 16 <= lo || p >= hi) continue;
    uint32_t w[4];
    if (p >= lo && p + 16 <= hi) {
      const uint4 q = *reinterpret_cast<const uint4*>(label + (p - lo));      // 16-byte aligned: p and the address of label - shift are
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {                                                                  // the head or the tail of the volume cuts this run
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int64_t pp = p + 4 * k + b;
          const uint32_t lab = (pp >= lo && pp < hi) ? (uint32_t)label[pp - lo] : 0xffu;
          w[k] |= lab << (8 * b);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t mw = loc_member4(w[k], tab);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        // the four membership bits of region r, one per byte, gathered into a nibble (the partial products meet in no bit)
        const uint32_t nib = ((((mw >> r) & 0x01010101u) * 0x01020408u) >> 24) & 0xfu;
        m[r] |= (uint64_t)nib << (run * 16 + k * 4);
      }
    }
  }
}

// popcounts of regions 4w .. 4w+3 as the 16-bit fields of one word
template <int NR>
__device__ __forceinline__ void loc_pack(const uint64_t (&m)[NR], uint64_t (&c)[NR / 4]) {
#pragma unroll
  for (int w = 0; w < NR / 4; ++w) {
    c[w] = 0ull;
#pragma unroll
    for (int f = 0; f < 4; ++f) c[w] |= (uint64_t)__popcll(m[4 * w + f]) << (16 * f);
  }
}

template <int NR>
__global__ __launch_bounds__(LOC_THREADS) void loc_count_kernel(const uint8_t* __restrict__ label, int64_t V, int shift, uint64_t tab, int R,
                                                                uint32_t* __restrict__ part) {
  __shared__ uint64_t red[LOC_THREADS / 64][NR / 4];
  uint64_t m[NR], c[NR / 4];
  loc_masks<NR>(label, V, shift, (int64_t)blockIdx.x * LOC_TILE + (int64_t)threadIdx.x * LOC_LANE, tab, m);
  loc_pack<NR>(m, c);
#pragma unroll
  for (int w = 0; w < NR / 4; ++w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[w] += loc_shfl_xor(c[w], o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][w] = c[w];
  }
  __syncthreads();
  if ((int)threadIdx.x < R) {
    const int w = threadIdx.x >> 2, f = threadIdx.x & 3;
    uint64_t s = 0ull;
#pragma unroll
    for (int k = 0; k < LOC_THREADS / 64; ++k) s += red[k][w];
    part[(int64_t)blockIdx.x * R + threadIdx.x] = (uint32_t)(s >> (16 * f)) & 0xffffu;
  }
}

// One workgroup: part[g][r] -> its exclusive prefix over g, in place; counts[r]; table[r][min(n_r, K) .. K) = -1.
__global__ __launch_bounds__(LOC_SCAN_THREADS) void loc_scan_kernel(uint32_t* __restrict__ part, int G, int R, int K, int64_t* __restrict__ counts,
                                                                    int32_t* __restrict__ table) {
  __shared__ uint32_t wsum[LOC_SCAN_THREADS / 64];
  __shared__ uint32_t total[LOC_MAX_R];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (G + LOC_SCAN_THREADS - 1) / LOC_SCAN_THREADS;
  const int g0 = min(tid * per, G), g1 = min(g0 + per, G);
  for (int r = 0; r < R; ++r) {
    uint32_t s = 0u;
    for (int g = g0; g < g1; ++g) s += part[(int64_t)g * R + r];
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0u, all = 0u;
#pragma unroll
    for (int k = 0; k < LOC_SCAN_THREADS / 64; ++k) { const uint32_t t = wsum[k]; if (k < wave) base += t; all += t; }
    uint32_t run = base + inc - s;
    for (int g = g0; g < g1; ++g) { const uint32_t t = part[(int64_t)g * R + r]; part[(int64_t)g * R + r] = run; run += t; }
    if (tid == 0) { total[r] = all; counts[r] = (int64_t)all; }
    __syncthreads();
  }
  for (int r = 0; r < R; ++r) {
    const int m = (int)min(total[r], (uint32_t)K);
    for (int j = m + tid; j < K; j += LOC_SCAN_THREADS) table[(int64_t)r * K + j] = -1;
  }
}

template <int NR>
__global__ __launch_bounds__(LOC_THREADS) void loc_select_kernel(const uint8_t* __restrict__ label, int64_t V, int shift, uint64_t tab, int R, int K,
                                                                 const uint32_t* __restrict__ part, const int64_t* __restrict__ counts,
                                                                 int32_t* __restrict__ table) {
  __shared__ uint64_t wsum[LOC_THREADS / 64][NR / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * LOC_TILE + (int64_t)threadIdx.x * LOC_LANE;
  uint64_t m[NR], c[NR / 4], ex[NR / 4];
  loc_masks<NR>(label, V, shift, p0, tab, m);
  loc_pack<NR>(m, c);
#pragma unroll
  for (int w = 0; w < NR / 4; ++w) {
    uint64_t inc = c[w];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t t = loc_shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave][w] = inc;
    ex[w] = inc - c[w];
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NR / 4; ++w)
    for (int k = 0; k < wave; ++k) ex[w] += wsum[k][w];
  const int64_t v0 = p0 - shift;                  // the linear index of this lane's bit 0
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    uint64_t bits = m[r];
    if (r >= R || bits == 0ull) continue;
    const uint64_t n = (uint64_t)counts[r];
    const uint64_t rank0 = (uint64_t)part[(int64_t)blockIdx.x * R + r] + ((ex[r >> 2] >> (16 * (r & 3))) & 0xffffull);
    int32_t* row = table + (int64_t)r * K;
    if (n <= (uint64_t)K) {
      uint64_t j = rank0;
      while (bits) { row[j++] = (int32_t)(v0 + (__ffsll((long long)bits) - 1)); bits &= bits - 1ull; }
      continue;
    }
    // n > m = K: the entries whose rank falls among this lane's ranks [rank0, rank0 + cnt)
    const uint64_t mm = (uint64_t)K, rank1 = rank0 + (uint64_t)__popcll(bits);
    uint64_t j = (rank0 * mm + n - 1ull) / n;     // ceil(rank0 m / n), below 2^47
    if (j >= mm) continue;
    uint64_t q = (j * n) / mm, rem = (j * n) - q * mm;      // floor(j n / m) and the remainder
    const uint64_t dq = n / mm, dr = n - dq * mm;
    uint64_t at = rank0;                          // the rank of the lowest bit still set in `bits`
    while (j < mm && q < rank1) {
      while (at < q) { bits &= bits - 1ull; ++at; }
      row[j] = (int32_t)(v0 + (__ffsll((long long)bits) - 1));
      ++j; q += dq; rem += dr;
      if (rem >= mm) { rem -= mm; ++q; }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t loc_tiles(int64_t V) { return cdiv64(V + 15, LOC_TILE); }      // the head may shift the volume by up to 15 positions

static int loc_check(int64_t V, int R) {
  if (V < 1 || V > 0x7fffffffll || R < 1 || R > LOC_MAX_R) return CWF_E_BADARG;
  return 0;
}

extern "C" int64_t cwf_class_locations_workspace(int64_t V, int R) {
  const int rc = loc_check(V, R);
  if (rc) return rc;
  return (loc_tiles(V) * R * (int64_t)sizeof(uint32_t) + 255) & ~(int64_t)255;
}

extern "C" int cwf_class_locations(const uint8_t* label, int64_t V, const uint32_t* posmasks, int R, int K, int64_t* counts, int32_t* table,
                                   void* ws, void* stream) {
  const int rc = loc_check(V, R);
  if (rc) return rc;
  if (!label || !posmasks || !counts || !table || !ws || K < 1 || K > 65536) return CWF_E_BADARG;
  uint64_t tab = 0ull;
  for (int r = 0; r < R; ++r) {
    if (posmasks[r] & ~0xfu) return CWF_E_BADARG;
    for (int c = 0; c < 5; ++c)
      if ((posmasks[r] >> (c == 4 ? 3 : c)) & 1u) tab |= 1ull << (8 * c + r);
  }
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  const int shift = (int)((uintptr_t)label & 15);
  const int G = (int)cdiv64(V + shift, LOC_TILE);             // <= loc_tiles(V)
  uint32_t* part = (uint32_t*)ws;
  if (R <= 4) hipLaunchKernelGGL(loc_count_kernel<4>, dim3((unsigned)G), dim3(LOC_THREADS), 0, st, label, V, shift, tab, R, part);
  else hipLaunchKernelGGL(loc_count_kernel<8>, dim3((unsigned)G), dim3(LOC_THREADS), 0, st, label, V, shift, tab, R, part);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(loc_scan_kernel, dim3(1), dim3(LOC_SCAN_THREADS), 0, st, part, G, R, K, counts, table);
  CWF_LAUNCH_CHECK();
  if (R <= 4) hipLaunchKernelGGL(loc_select_kernel<4>, dim3((unsigned)G), dim3(LOC_THREADS), 0, st, label, V, shift, tab, R, K, part, counts, table);
  else hipLaunchKernelGGL(loc_select_kernel<8>, dim3((unsigned)G), dim3(LOC_THREADS), 0, st, label, V, shift, tab, R, K, part, counts, table);
  CWF_LAUNCH_CHECK();
  return 0;
}
