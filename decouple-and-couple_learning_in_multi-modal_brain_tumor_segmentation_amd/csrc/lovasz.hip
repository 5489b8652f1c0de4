// L5 -- Lovasz-Softmax (Berman, Triggs, Blaschko, CVPR 2018) on class-bitmask regions: the Jaccard loss's convex surrogate, by an exact
// sort of the per-voxel errors of the whole batch on the device.  This project's statement (restated in tests/lovasz_ref.py, derived in
// DESIGN.md):
//   prob    float32 [N, V, 4] channels-last; label int64 [N, V], class y = label & 3 (a foreign label reads inside its own voxel).
//           M = N V voxels; the sort runs over the whole batch (Berman's per_image=False).
//   regions r < R (1 <= R <= 8), class bitmasks m_r over bits 0..3 (values 1..15).  Per region and voxel:
//   fg      = (m_r >> y) & 1
//   q       = the p_c of the classes of m_r added in ascending class order, float32 (a one-class mask: q = p_c exactly)
//   qc      = (q > 0) ? fminf(q, 1.0f) : 0.0f          NaN, negatives and -0 become +0; anything above 1, and +inf, become 1
//   e       = fg ? 1.0f - qc : qc                      0 <= e <= 1;  bits(e) as uint32 orders like e
//   sgn     = (e > 0) ? (fg ? -1 : +1) : 0             a voxel with zero error has no gradient
//   groups  G = #{fg}.  The distinct values of e in DESCENDING order; group j holds the m_j voxels with that value, f_j of them
//           foreground; n_j = m_1 + .. + m_j, F_j = f_1 + .. + f_j, n_0 = F_0 = 0.
//   J(n, F) = 0.0 if n = 0, else 1.0 - (double)(G - F) / (double)(G + n - F);   dJ_j = J(n_j, F_j) - J(n_{j-1}, F_{j-1})   (float64)
//   L_r     = sum_j (double)e_j dJ_j.  A region is counted if G_r > 0, or always with only_present = 0; P = the number counted.
//   loss    = float32((double)w / max(P, 1) * sum_counted L_r), w read from device memory;  P = 0: +0
//   coef    [0] = float32((double)w / P) (+0 when P = 0), [1] = (float)P, [2] = [3] = +0
//   ties    every voxel of group j carries c_r(v) = float32(dJ_j / (double)m_j), the symmetric subgradient; c = 0 in a region that is
//           not counted.  vcoef[r][v] = c_r(v) * (float)sgn_r(v).
//   bwd     g0 = gscale[0] * coef[0];  dprob[v][c] = 0.0f + the (g0 * vcoef[r][v]) of the regions holding class c, ascending r, every
//           product and sum rounded on its own.
// This file is compiled with -ffp-contract=off.
//
// Pass structure (fifteen launches; no host synchronisation, nothing read back, no float atomics, no workgroup waits on another, no memcpy node; a
// launch boundary is the only ordering between workgroups):
//   lv_keys_kernel      reads prob and label (24 B / voxel) and writes one 32-bit key per voxel and region, (fg << 30) | bits(e)
//                       (bits(e) <= 0x3f800000 leaves bits 30 and 31 free), and the per-tile counts of digit 0
//   four LSD passes of 8 bits, each  lv_count_kernel (per-tile digit counts; pass 0 has them from the key pass)
//                                    lv_rowscan_kernel (one workgroup per digit and region: exclusive prefix over the tiles, digit total)
//                                    lv_scatter_kernel (stable: ranks from wave ballots in lane, round and wave order, never from the
//                                    arrival order of an atomic; keys are ordered in LDS first, so a digit's keys leave as one run)
//                       Equal keys are indistinguishable, so the sorted array is unique: [background by e][foreground by e], one
//                       ascending uint32 sequence.
//   lv_tree_kernel      samples every 16th, 256th, .. key of the sorted array into the levels of a 16-ary search tree (M / 15 keys)
//   lv_voxel_kernel     recomputes e per voxel and region (the key arrays are the sort's ping and pong, the unsorted keys are gone: a
//                       second read of prob and label costs no third key array), finds n_{j-1}, n_j, F_{j-1}, F_j as the lower / upper
//                       bounds of bits(e) and of bits(e) | fg bit, one 64-byte node per tree level (cache traffic: tree and array sit
//                       in L2 / Infinity Cache), evaluates dJ / m in float64, writes vcoef and a per-workgroup float64 partial of
//                       e dJ / m per region, stored plainly
//   lv_finalize_kernel  one workgroup adds the partials in index order, forms P, coef and the loss
//   lv_bwd_kernel       one streaming launch: reads vcoef, one 16-byte store per voxel
// G_r is the number of keys with bit 30 set: the sum of the last pass's digit totals from 64 up.  Every workspace word that is read has
// been written by an earlier launch of the same call: the workspace may hold anything on entry.
#include <algorithm>
#include "common.h"

#define LV_THREADS 256
#define LV_WAVES (LV_THREADS / 64)
#define LV_ITEMS 16                      // keys a thread of a sort pass holds
#define LV_TILE (LV_THREADS * LV_ITEMS)  // 4096 keys per workgroup of a sort pass
#define LV_BINS 256                      // 8-bit digits: shifts 0, 8, 16, 24
#define LV_MAX_R 8
#define LV_MAX_GRID 1024                 // workgroups of the voxel pass = partials per region
#define LV_FG_BIT 0x40000000u
#define LV_MAX_LEVELS 7                  // 16^8 = 2^32: eight levels with the array itself cover every 32-bit position

struct LvMasks { uint32_t m[LV_MAX_R]; };

__device__ __forceinline__ float lv_region_q(const float4 p, uint32_t m) {
  float q = 0.0f;
  bool first = true;
  if (m & 1u) { q = p.x; first = false; }
  if (m & 2u) { q = first ? p.y : q + p.y; first = false; }
  if (m & 4u) { q = first ? p.z : q + p.z; first = false; }
  if (m & 8u) { q = first ? p.w : q + p.w; }
  return q;
}

// e of a voxel in a region
__device__ __forceinline__ float lv_error(const float4 p, uint32_t m, bool fg) {
  const float q = lv_region_q(p, m);
  const float qc = (q > 0.f) ? fminf(q, 1.0f) : 0.0f;
  return fg ? 1.0f - qc : qc;
}

// ---- sort ---------------------------------------------------------------------------------------------------------------------
// counts[(r * 256 + d) * T + tile]: first the tile's count of digit d, after the row scan the count over the tiles before it

// One workgroup per tile of 4096 voxels: the keys of every region, and the counts of digit 0.
__global__ __launch_bounds__(LV_THREADS) void lv_keys_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label, LvMasks masks, int R,
                                                            int64_t M, int64_t S, int T, uint32_t* __restrict__ keys, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[LV_MAX_R * LV_BINS];
  for (int b = threadIdx.x; b < R * LV_BINS; b += LV_THREADS) hist[b] = 0u;
  __syncthreads();
  const float4* __restrict__ prob4 = reinterpret_cast<const float4*>(prob);
  const int64_t base = (int64_t)blockIdx.x * LV_TILE + threadIdx.x;
#pragma unroll 4
  for (int i = 0; i < LV_ITEMS; ++i) {
    const int64_t gv = base + (int64_t)i * LV_THREADS;
    if (gv >= M) break;
    const float4 p = prob4[gv];
    const int y = (int)(label[gv] & 3);
    for (int r = 0; r < R; ++r) {
      const bool fg = (masks.m[r] >> y) & 1u;
      const uint32_t key = __float_as_uint(lv_error(p, masks.m[r], fg)) | (fg ? LV_FG_BIT : 0u);
      keys[(int64_t)r * S + gv] = key;
      atomicAdd(&hist[r * LV_BINS + (key & 255u)], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < R * LV_BINS; b += LV_THREADS) counts[(int64_t)b * T + blockIdx.x] = hist[b];
}

template <int SHIFT>
__global__ __launch_bounds__(LV_THREADS) void lv_count_kernel(const uint32_t* __restrict__ keys, int64_t M, int64_t S, int T, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[LV_BINS];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t* __restrict__ src = keys + (int64_t)blockIdx.y * S;
  const int64_t base = (int64_t)blockIdx.x * LV_TILE + threadIdx.x;
#pragma unroll
  for (int i = 0; i < LV_ITEMS; ++i) {
    const int64_t idx = base + (int64_t)i * LV_THREADS;
    if (idx < M) atomicAdd(&hist[(src[idx] >> SHIFT) & 255u], 1u);
  }
  __syncthreads();
  counts[((int64_t)blockIdx.y * LV_BINS + threadIdx.x) * T + blockIdx.x] = hist[threadIdx.x];
}

// exclusive prefix sums of 256 values, one per thread (doubling; the result of thread t is the sum of the values of the threads below it)
__device__ __forceinline__ unsigned long long lv_block_exclusive(unsigned long long mine, unsigned long long (*part)[LV_THREADS]) {
  part[0][threadIdx.x] = mine;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < LV_THREADS; o <<= 1) {
    unsigned long long v = part[cur][threadIdx.x];
    if ((int)threadIdx.x >= o) v += part[cur][threadIdx.x - o];
    part[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  const unsigned long long res = part[cur][threadIdx.x] - mine;
  __syncthreads();                                   // (part may be filled again)
  return res;
}

// One workgroup per (digit, region): the row of T tile counts becomes its exclusive prefix, the row's sum goes to totals.
__global__ __launch_bounds__(LV_THREADS) void lv_rowscan_kernel(uint32_t* __restrict__ counts, int T, uint32_t* __restrict__ totals) {
  __shared__ unsigned long long part[2][LV_THREADS];
  const int row = blockIdx.y * LV_BINS + blockIdx.x;
  uint32_t* __restrict__ c = counts + (int64_t)row * T;
  const int per = (T + LV_THREADS - 1) / LV_THREADS;
  const int lo = min(T, (int)threadIdx.x * per), hi = min(T, lo + per);
  uint32_t mine = 0u;
  for (int t = lo; t < hi; ++t) mine += c[t];
  uint32_t before = (uint32_t)lv_block_exclusive(mine, part);
  for (int t = lo; t < hi; ++t) {
    const uint32_t v = c[t];
    c[t] = before;
    before += v;
  }
  if (threadIdx.x == LV_THREADS - 1) totals[row] = before;
}

// Stable scatter of one tile by the digit at SHIFT.  A key's place in the tile's order is (wave, round, lane): a wave owns 1024
// consecutive keys and takes them 64 at a time.
template <int SHIFT>
__global__ __launch_bounds__(LV_THREADS) void lv_scatter_kernel(const uint32_t* __restrict__ keys_in, uint32_t* __restrict__ keys_out, int64_t M, int64_t S, int T,
                                                               const uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals) {
  __shared__ uint32_t wcnt[LV_WAVES][LV_BINS];        // a wave's running count per digit, later its start inside the digit's run
  __shared__ unsigned long long part[2][LV_THREADS];
  __shared__ uint32_t tstart[LV_BINS];                // start of the digit's run in the ordered tile
  __shared__ uint32_t gstart[LV_BINS];                // global position of that run
  __shared__ uint32_t ordered[LV_TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = blockIdx.y;
  const uint32_t* __restrict__ src = keys_in + (int64_t)r * S;
  uint32_t* __restrict__ dst = keys_out + (int64_t)r * S;
  const int64_t tile0 = (int64_t)blockIdx.x * LV_TILE;
  const int ntile = (int)min((int64_t)LV_TILE, M - tile0);
#pragma unroll
  for (int w = 0; w < LV_WAVES; ++w) wcnt[w][tid] = 0u;
  __syncthreads();

  uint32_t key[LV_ITEMS], off[LV_ITEMS];
#pragma unroll
  for (int i = 0; i < LV_ITEMS; ++i) {
    const int e = wave * (LV_ITEMS * 64) + i * 64 + lane;
    key[i] = e < ntile ? src[tile0 + e] : 0xFFFFFFFFu;
  }
  volatile uint32_t* mycnt = wcnt[wave];
  const unsigned long long below_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < LV_ITEMS; ++i) {
    const bool valid = wave * (LV_ITEMS * 64) + i * 64 + lane < ntile;
    const uint32_t d = (key[i] >> SHIFT) & 255u;
    unsigned long long peers = __ballot(valid);       // the valid lanes of this round that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(peers & below_mask);
    const uint32_t pre = mycnt[d];                    // (every peer reads the same count before the first of them raises it)
    off[i] = pre + below;
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0u) mycnt[d] = pre + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  {                                                   // thread = digit
    uint32_t run = 0u;
#pragma unroll
    for (int w = 0; w < LV_WAVES; ++w) {
      const uint32_t c = wcnt[w][tid];
      wcnt[w][tid] = run;
      run += c;
    }
    // the digit's start in the tile (low word) and in the whole array (high word), by one scan
    const unsigned long long ex = lv_block_exclusive(((unsigned long long)totals[r * LV_BINS + tid] << 32) | run, part);
    tstart[tid] = (uint32_t)ex;
    gstart[tid] = (uint32_t)(ex >> 32) + counts[((int64_t)r * LV_BINS + tid) * T + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < LV_ITEMS; ++i) {
    const bool valid = wave * (LV_ITEMS * 64) + i * 64 + lane < ntile;
    const uint32_t d = (key[i] >> SHIFT) & 255u;
    const uint32_t p = tstart[d] + wcnt[wave][d] + off[i];
    if (valid && p < (uint32_t)LV_TILE) ordered[p] = key[i];        // (the ranks sum to ntile; the comparison only fences the LDS store)
  }
  __syncthreads();
  for (int j = tid; j < ntile; j += LV_THREADS) {
    const uint32_t k = ordered[j];
    const uint32_t d = (k >> SHIFT) & 255u;
    const int64_t p = (int64_t)gstart[d] + ((int64_t)j - (int64_t)tstart[d]);
    if (p >= 0 && p < M) dst[p] = k;                  // (counts and ranks come from the same keys; the comparison only fences the store)
  }
}

// ---- per-voxel pass -----------------------------------------------------------------------------------------------------------
// The sorted array of a region is one ascending uint32 sequence (every background key is below every foreground key).  Level l >= 1 of
// its search tree holds every 16^l-th key, tree[off[l] + j] = sorted[(j + 1) 16^l - 1] for j < n[l] = M >> 4 l: a node is 16 consecutive
// entries, one 64-byte line, and a search reads one node per level where a binary search reads one line per step.
struct LvTree { int nlev; uint32_t n[LV_MAX_LEVELS + 1]; uint32_t off[LV_MAX_LEVELS + 1]; };

__global__ __launch_bounds__(LV_THREADS) void lv_tree_kernel(const uint32_t* __restrict__ sorted, int64_t S, LvTree t, uint32_t total, int64_t tree_stride,
                                                            uint32_t* __restrict__ tree) {
  const uint32_t i = blockIdx.x * LV_THREADS + threadIdx.x;
  if (i >= total) return;
  int l = 1;
  while (l < t.nlev && i >= t.off[l + 1]) ++l;        // (the levels lie one after the other, each padded; i may fall into a padding)
  const uint32_t j = i - t.off[l];
  if (j >= t.n[l]) return;
  const int64_t pos = (((int64_t)j + 1) << (4 * l)) - 1;
  tree[(int64_t)blockIdx.y * tree_stride + i] = sorted[(int64_t)blockIdx.y * S + pos];
}

// lb = the first index whose key is >= t, ub = the first whose key is > t (M if none), in the region's sorted array s
__device__ __forceinline__ uint32_t lv_descend(const uint32_t* __restrict__ s, const uint32_t* __restrict__ tree, const LvTree& T, uint32_t M, uint32_t t,
                                               uint32_t* le, uint32_t* nvalid) {
  uint32_t c = 0u;
  for (int l = T.nlev; l >= 0; --l) {
    const uint32_t* __restrict__ a = l ? tree + T.off[l] : s;
    const uint32_t n = l ? T.n[l] : M;
    const uint32_t base = c * 16u;                    // <= n: the arrays are padded by a node
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(a + base);
    const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
    const uint32_t k[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
    uint32_t lt = 0u, leq = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool in = base + (uint32_t)i < n;
      lt += (in && k[i] < t) ? 1u : 0u;
      leq += (in && k[i] <= t) ? 1u : 0u;
    }
    c = base + lt;
    if (l == 0) { *le = base + leq; *nvalid = min(16u, n - base); *nvalid += base; }
  }
  return c;
}

__device__ __forceinline__ void lv_bounds(const uint32_t* __restrict__ s, const uint32_t* __restrict__ tree, const LvTree& T, uint32_t M, uint32_t t,
                                          uint32_t* lb, uint32_t* ub) {
  uint32_t le, end;
  *lb = lv_descend(s, tree, T, M, t, &le, &end);
  if (le < end) { *ub = le; return; }                 // a larger key lies in the same node
  uint32_t le2, end2;
  *ub = lv_descend(s, tree, T, M, t + 1u, &le2, &end2);   // (t <= 0x7f800000: no overflow)
}

__device__ __forceinline__ double lv_jaccard(uint32_t n, uint32_t F, uint32_t G) {
  return n == 0u ? 0.0 : 1.0 - (double)(G - F) / (double)((G - F) + n);
}

// G of every region from the last pass's digit totals (digits 64.. hold the keys with bit 30 set); call with all threads
__device__ __forceinline__ void lv_fg_counts(const uint32_t* __restrict__ totals, int R, uint32_t* G) {
  if (threadIdx.x < LV_MAX_R) {
    uint32_t g = 0u;
    if ((int)threadIdx.x < R)
      for (int d = 64; d < LV_BINS; ++d) g += totals[threadIdx.x * LV_BINS + d];
    G[threadIdx.x] = g;
  }
  __syncthreads();
}

__global__ __launch_bounds__(LV_THREADS) void lv_voxel_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label, LvMasks masks, int R,
                                                             int only_present, int64_t M, int64_t S, const uint32_t* __restrict__ sorted,
                                                             LvTree T, int64_t tree_stride, const uint32_t* __restrict__ tree,
                                                             const uint32_t* __restrict__ totals, float* __restrict__ vcoef,
                                                             double* __restrict__ slab) {
  __shared__ uint32_t G[LV_MAX_R];
  __shared__ double red[LV_WAVES][LV_MAX_R];
  lv_fg_counts(totals, R, G);
  double acc[LV_MAX_R];
#pragma unroll
  for (int r = 0; r < LV_MAX_R; ++r) acc[r] = 0.0;
  const float4* __restrict__ prob4 = reinterpret_cast<const float4*>(prob);
  const uint32_t Mu = (uint32_t)M;
  for (int64_t gv = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x; gv < M; gv += (int64_t)gridDim.x * LV_THREADS) {
    const float4 p = prob4[gv];
    const int y = (int)(label[gv] & 3);
#pragma unroll
    for (int r = 0; r < LV_MAX_R; ++r) {
      if (r >= R) break;
      const uint32_t g = G[r];
      float out = 0.0f;
      const bool fg = (masks.m[r] >> y) & 1u;
      const float e = lv_error(p, masks.m[r], fg);
      const float sgn = (e > 0.f) ? (fg ? -1.0f : 1.0f) : 0.0f;
      if (g > 0u || !only_present) {
        const uint32_t* __restrict__ s = sorted + (int64_t)r * S;
        const uint32_t* __restrict__ tr = tree + (int64_t)r * tree_stride;
        const uint32_t b = __float_as_uint(e);
        const uint32_t nbg = Mu - g;                  // the background keys are s[0, nbg), the foreground keys s[nbg, M)
        uint32_t lb0, ub0, lb1, ub1;
        lv_bounds(s, tr, T, Mu, b, &lb0, &ub0);                           // both inside [0, nbg]: every foreground key is larger
        lv_bounds(s, tr, T, Mu, b | LV_FG_BIT, &lb1, &ub1);                // both inside [nbg, M]
        const uint32_t F_prev = Mu - ub1, F_cur = Mu - lb1;             // foreground keys above / not below e
        const uint32_t n_prev = (nbg - ub0) + F_prev, n_cur = (nbg - lb0) + F_cur;
        const double dJ = lv_jaccard(n_cur, F_cur, g) - lv_jaccard(n_prev, F_prev, g);
        const double share = dJ / (double)(n_cur - n_prev);              // (the voxel's own key is in the group: n_cur > n_prev)
        acc[r] += (double)e * share;
        out = (float)share;
      }
      vcoef[(int64_t)r * M + gv] = out * sgn;
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < LV_MAX_R; ++r) {
    const double a = wave_sum_d(acc[r]);
    if ((threadIdx.x & 63) == 0) red[wave][r] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < R) {
    const int r = threadIdx.x;
    slab[(int64_t)r * LV_MAX_GRID + blockIdx.x] = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
  }
}

// one workgroup: stages the partials of four regions at a time in LDS, thread j adds those of region base + j in index order
__global__ __launch_bounds__(LV_THREADS) void lv_finalize_kernel(const double* __restrict__ slab, int nslab, const uint32_t* __restrict__ totals, int R,
                                                                int only_present, const float* __restrict__ weight, float* __restrict__ loss,
                                                                float* __restrict__ coef) {
  __shared__ uint32_t G[LV_MAX_R];
  __shared__ double stage[4][LV_MAX_GRID];
  __shared__ double L[LV_MAX_R];
  lv_fg_counts(totals, R, G);
  for (int base = 0; base < R; base += 4) {
    const int nr = min(4, R - base);
    for (int i = threadIdx.x; i < nr * nslab; i += LV_THREADS) stage[i / nslab][i % nslab] = slab[(int64_t)(base + i / nslab) * LV_MAX_GRID + i % nslab];
    __syncthreads();
    if ((int)threadIdx.x < nr) {
      double s = 0.0;
#pragma unroll 8
      for (int i = 0; i < nslab; ++i) s += stage[threadIdx.x][i];
      L[base + threadIdx.x] = s;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  int P = 0;
  double S = 0.0;
  for (int r = 0; r < R; ++r)
    if (G[r] > 0u || !only_present) { P += 1; S += L[r]; }
  const double w = (double)weight[0];
  loss[0] = P > 0 ? (float)(w / (double)P * S) : 0.0f;
  coef[0] = P > 0 ? (float)(w / (double)P) : 0.0f;
  coef[1] = (float)P;
  coef[2] = 0.0f;
  coef[3] = 0.0f;
}

__global__ __launch_bounds__(LV_THREADS) void lv_bwd_kernel(const float* __restrict__ vcoef, LvMasks masks, int R, const float* __restrict__ coef,
                                                           const float* __restrict__ gscale, float* __restrict__ dprob, int64_t M) {
  const int64_t gv = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (gv >= M) return;
  const float g0 = gscale[0] * coef[0];
  float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int r = 0; r < LV_MAX_R; ++r) {
    if (r >= R) break;
    const float t = g0 * vcoef[(int64_t)r * M + gv];
    const uint32_t m = masks.m[r];
    if (m & 1u) d.x += t;
    if (m & 2u) d.y += t;
    if (m & 4u) d.z += t;
    if (m & 8u) d.w += t;
  }
  reinterpret_cast<float4*>(dprob)[gv] = d;
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t lv_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

// M, or a negative CWF_E_*.  Positions in the sorted array are 32-bit.
static int64_t lv_voxels(int N, int64_t V) {
  if (N <= 0 || V <= 0) return CWF_E_BADARG;
  if (V > (int64_t)0x7fffffff / N) return CWF_E_TOOLARGE;
  return (int64_t)N * V;
}

static int lv_masks(const uint32_t* posmasks, int R, LvMasks& masks) {
  if (R < 1 || R > LV_MAX_R || !posmasks) return CWF_E_BADARG;
  for (int r = 0; r < LV_MAX_R; ++r) masks.m[r] = 0u;
  for (int r = 0; r < R; ++r) {
    if (posmasks[r] == 0u || posmasks[r] > 15u) return CWF_E_BADARG;
    masks.m[r] = posmasks[r];
  }
  return 0;
}

struct LvLayout { int64_t S, keys_bytes, counts_bytes, totals_bytes, slab_bytes, tree_stride, tree_bytes; int T; LvTree tree; uint32_t tree_total; };

static LvLayout lv_layout(int64_t M, int R) {
  LvLayout l;
  l.T = (int)cdiv64(M, LV_TILE);
  l.S = ((M + 15) & ~(int64_t)15) + 16;              // a region's keys start on a 64-byte line and a node may be read past the last key
  l.keys_bytes = lv_align((int64_t)R * l.S * 4);
  l.tree.nlev = 0;
  for (int i = 0; i <= LV_MAX_LEVELS; ++i) { l.tree.n[i] = 0u; l.tree.off[i] = 0u; }
  uint32_t off = 0u;
  for (int lev = 1; lev <= LV_MAX_LEVELS && (M >> (4 * (lev - 1))) > 16; ++lev) {       // up to the first level of at most 16 entries
    l.tree.nlev = lev;
    l.tree.n[lev] = (uint32_t)(M >> (4 * lev));
    l.tree.off[lev] = off;
    off += ((l.tree.n[lev] + 15u) & ~15u) + 16u;
  }
  l.tree_total = off;
  l.tree_stride = off;
  l.tree_bytes = lv_align((int64_t)R * off * 4);
  l.counts_bytes = lv_align((int64_t)R * LV_BINS * l.T * 4);
  l.totals_bytes = lv_align((int64_t)LV_MAX_R * LV_BINS * 4);
  l.slab_bytes = lv_align((int64_t)LV_MAX_R * LV_MAX_GRID * 8);
  return l;
}

extern "C" int64_t cwf_lovasz_workspace(int N, int64_t V, int R) {
  const int64_t M = lv_voxels(N, V);
  if (M < 0) return M;
  if (R < 1 || R > LV_MAX_R) return CWF_E_BADARG;
  const LvLayout l = lv_layout(M, R);
  return 2 * l.keys_bytes + l.counts_bytes + l.totals_bytes + l.slab_bytes + l.tree_bytes;
}

extern "C" int cwf_lovasz(const float* prob, const int64_t* label, const uint32_t* posmasks, int R, int only_present, const float* weight,
                          float* loss, float* coef, float* vcoef, int N, int64_t V, void* ws, void* stream) {
  if (!prob || !label || !weight || !loss || !coef || !vcoef || !ws) return CWF_E_BADARG;
  const int64_t M = lv_voxels(N, V);
  if (M < 0) return (int)M;
  LvMasks masks;
  const int rc = lv_masks(posmasks, R, masks);
  if (rc) return rc;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  if (((uintptr_t)prob & 15) || ((uintptr_t)label & 7) || ((uintptr_t)loss & 3) || ((uintptr_t)coef & 3) || ((uintptr_t)vcoef & 3)) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  const LvLayout l = lv_layout(M, R);
  uint8_t* w8 = (uint8_t*)ws;
  uint32_t* ka = (uint32_t*)w8;
  uint32_t* kb = (uint32_t*)(w8 + l.keys_bytes);
  uint32_t* counts = (uint32_t*)(w8 + 2 * l.keys_bytes);
  uint32_t* totals = (uint32_t*)(w8 + 2 * l.keys_bytes + l.counts_bytes);
  double* slab = (double*)(w8 + 2 * l.keys_bytes + l.counts_bytes + l.totals_bytes);
  uint32_t* tree = (uint32_t*)(w8 + 2 * l.keys_bytes + l.counts_bytes + l.totals_bytes + l.slab_bytes);
  const int64_t S = l.S;
  const int T = l.T;
  const dim3 block(LV_THREADS), tiles((unsigned)T, (unsigned)R), rows(LV_BINS, (unsigned)R);

  hipLaunchKernelGGL(lv_keys_kernel, dim3((unsigned)T), block, 0, st, prob, label, masks, R, M, S, T, ka, counts);
  CWF_LAUNCH_CHECK();
#define LV_PASS(SHIFT, SRC, DST)                                                                           \
  if (SHIFT) { hipLaunchKernelGGL(lv_count_kernel<SHIFT>, tiles, block, 0, st, SRC, M, S, T, counts); CWF_LAUNCH_CHECK(); } \
  hipLaunchKernelGGL(lv_rowscan_kernel, rows, block, 0, st, counts, T, totals);                            \
  CWF_LAUNCH_CHECK();                                                                                      \
  hipLaunchKernelGGL(lv_scatter_kernel<SHIFT>, tiles, block, 0, st, SRC, DST, M, S, T, counts, totals);       \
  CWF_LAUNCH_CHECK();
  LV_PASS(0, ka, kb)
  LV_PASS(8, kb, ka)
  LV_PASS(16, ka, kb)
  LV_PASS(24, kb, ka)
#undef LV_PASS
  const int nwg = (int)std::min<int64_t>(cdiv64(M, LV_THREADS), LV_MAX_GRID);
  if (l.tree_total) {
    hipLaunchKernelGGL(lv_tree_kernel, dim3((unsigned)cdiv64(l.tree_total, LV_THREADS), (unsigned)R), block, 0, st, ka, S, l.tree, l.tree_total,
                       l.tree_stride, tree);
    CWF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lv_voxel_kernel, dim3((unsigned)nwg), block, 0, st, prob, label, masks, R, only_present ? 1 : 0, M, S, ka, l.tree,
                     l.tree_stride, tree, totals, vcoef, slab);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(lv_finalize_kernel, dim3(1), block, 0, st, slab, nwg, totals, R, only_present ? 1 : 0, weight, loss, coef);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_lovasz_bwd(const float* vcoef, const uint32_t* posmasks, int R, const float* coef, const float* gscale, float* dprob,
                              int N, int64_t V, void* stream) {
  if (!vcoef || !coef || !gscale || !dprob) return CWF_E_BADARG;
  const int64_t M = lv_voxels(N, V);
  if (M < 0) return (int)M;
  LvMasks masks;
  const int rc = lv_masks(posmasks, R, masks);
  if (rc) return rc;
  if (((uintptr_t)vcoef & 3) || ((uintptr_t)dprob & 15)) return CWF_E_ALIGN;
  hipLaunchKernelGGL(lv_bwd_kernel, dim3((unsigned)cdiv64(M, LV_THREADS)), dim3(LV_THREADS), 0, cwf_stream(stream), vcoef, masks, R, coef, gscale,
                     dprob, M);
  CWF_LAUNCH_CHECK();
  return 0;
}
