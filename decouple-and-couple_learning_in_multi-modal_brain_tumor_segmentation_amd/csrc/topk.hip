// L3 -- top-k (hard-voxel) cross-entropy: the mean of -log p_t over the k voxels of the whole batch with the smallest p_t, by an exact
// radix select on the device.  This project's statement (restated in tests/topk_ref.py):
//   prob    float32 [N, V, C] channels-last, C = 4 or 2; label int64 [N, V].  Target class t = label (C = 4) or
//           (posmask >> (label & 31)) & 1 (C = 2), as in cwf_dice_ce_*.  (C = 4 takes labels 0..3; the kernels read class label & 3,
//           so a foreign label reads inside its own voxel.)  M = N V voxels; the selection runs over the whole batch.
//   pc      = (p_t > 0) ? fminf(p_t, 1.0f) : 0.0f                NaN, negatives and -0 become +0
//   key     = bits(pc) as uint32; pc >= 0, so key order is value order and the smallest key is the hardest voxel
//   l       = -logf(fmaxf(pc, 1e-7f))
//   tau     = the k-th smallest key, 1 <= k <= M;  a = #{key < tau}, n = #{key = tau}, s = k - a (1 <= s <= n)
//   loss    = float32( (double)w / k * ( sum_{key < tau} (double)l_v + (double)s * (double)l(tau) ) ), w read from device memory
//   ties    every voxel with key = tau carries the weight s / n (the symmetric subgradient): neither voxel order nor launch geometry
//           enters the gradient
//   coef    [0] = float32((double)w / k), [1] = float32((double)s / (double)n), [2] = bits tau, [3] = +0
//   bwd     g0 = gscale[0] * coef[0], r = -1.0f / fmaxf(pc, 1e-7f), every product rounded on its own:
//           dprob[v][t] = g0 * r for key < tau, (g0 * coef[1]) * r for key = tau, +0 for key > tau and for every other class.
//           The gradient passes through the 1e-7 floor as -1 / 1e-7: the hardest voxels keep their gradient.
// This file is compiled with -ffp-contract=off.
//
// Pass structure (nine launches, no host synchronisation, nothing read back, no workgroup waits on another, no memcpy node):
//   tk_zero_kernel      zeroes the three digit histograms in the workspace (the caller zeroes nothing)
//   tk_keys_kernel      the only pass over prob and label (24 or 16 B / voxel): writes the compact key array (4 B / voxel) and counts
//                       digit 0 = key bits 31..21
//   tk_scan_kernel      one workgroup: finds the bucket that holds the remaining rank, appends it to the prefix, reduces the rank
//   tk_digit_kernel     re-reads the keys (4 B / voxel), counts digit 1 = bits 20..10 of the keys that share the prefix; scan;
//                       the same for digit 2 = bits 9..0; scan -> tau, s, n
//   tk_sum_kernel       re-reads the keys: per-workgroup float64 partial of l over key < tau, stored to a slab (no float atomics)
//   tk_finalize_kernel  one workgroup stages the slab in LDS, one thread adds it in index order and writes loss and coef
// Why a key array: every pass after the first needs pc alone.  Re-reading prob and label would move 24 B / voxel four more times
// (120 B / voxel in all); the key array costs 4 B written once and 4 B read in each of three passes (40 B / voxel in all), and l is
// a function of the key, so the sum pass needs nothing else.
// Why 11 + 11 + 10 bits: three digit passes instead of four at 8 bits, and a 2048-bin histogram is 8 KiB of LDS.  A workgroup counts
// in LDS (32-bit: a workgroup sees fewer than 2^32 voxels, the entry refuses more) and merges with one 64-bit integer atomic per
// non-empty bin; the global bins are 64-bit, so a bin can hold all M voxels.  Integer atomics commute exactly, so the counts, tau, s
// and n are the same on every run; the slab is added in a fixed order, so the loss repeats bit for bit.
#include <algorithm>
#include "common.h"

#define TK_THREADS 256
#define TK_MAX_GRID 1024                 // workgroups of every streaming pass = entries of the partial slab
#define TK_BINS0 2048                    // digit 0: key bits 31..21
#define TK_BINS1 2048                    // digit 1: key bits 20..10
#define TK_BINS2 1024                    // digit 2: key bits  9..0
#define TK_SHIFT0 21
#define TK_SHIFT1 10
#define TK_BATCH 4                       // voxels a thread of the key pass loads together
#define TK_FLOOR 1e-7f

// device-resident selection state, written by the scans
struct TkState {
  uint32_t prefix;                       // the digits of tau chosen so far, in place
  uint32_t pad;
  unsigned long long rank;               // 1-based rank still to find inside the chosen bucket; after the last scan: s
  unsigned long long count;              // size of the chosen bucket; after the last scan: n
};

__device__ __forceinline__ float tk_clamp(float p) { return (p > 0.f) ? fminf(p, 1.0f) : 0.0f; }
__device__ __forceinline__ float tk_nll(float pc) { return -logf(fmaxf(pc, TK_FLOOR)); }

template <int C>
__device__ __forceinline__ int tk_target(int64_t lab, uint32_t posmask) {
  return (C == 4) ? (int)(lab & 3) : (int)((posmask >> (int)(lab & 31)) & 1u);
}

// p_t of voxel gv through one vector load of the voxel's C probabilities
template <int C>
__device__ __forceinline__ float tk_pt(const float* __restrict__ prob, int64_t gv, int t) {
  if (C == 4) {
    const float4 q = *reinterpret_cast<const float4*>(prob + gv * 4);
    return t == 0 ? q.x : t == 1 ? q.y : t == 2 ? q.z : q.w;
  }
  const float2 q = *reinterpret_cast<const float2*>(prob + gv * 2);
  return t == 0 ? q.x : q.y;
}

__global__ __launch_bounds__(TK_THREADS) void tk_zero_kernel(unsigned long long* __restrict__ hist, int n) {
  const int i = blockIdx.x * TK_THREADS + threadIdx.x;
  if (i < n) hist[i] = 0ull;
}

// merge a workgroup's LDS histogram into the global one: one integer atomic per non-empty bin
template <int BINS>
__device__ __forceinline__ void tk_merge(const uint32_t* lds, unsigned long long* __restrict__ hist) {
  for (int b = threadIdx.x; b < BINS; b += TK_THREADS) {
    const uint32_t c = lds[b];
    if (c) atomicAdd(hist + b, (unsigned long long)c);
  }
}

template <int C>
__global__ __launch_bounds__(TK_THREADS) void tk_keys_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label, uint32_t posmask,
                                                             int64_t M, uint32_t* __restrict__ keys, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t lds[TK_BINS0];
  for (int b = threadIdx.x; b < TK_BINS0; b += TK_THREADS) lds[b] = 0u;
  __syncthreads();
  // TK_BATCH voxels per trip, a grid stride apart: their loads are issued together, then the keys are stored and counted
  const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; base < M; base += stride * TK_BATCH) {
    float pt[TK_BATCH];
#pragma unroll
    for (int j = 0; j < TK_BATCH; ++j) {
      const int64_t gv = base + j * stride;
      pt[j] = gv < M ? tk_pt<C>(prob, gv, tk_target<C>(label[gv], posmask)) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < TK_BATCH; ++j) {
      const int64_t gv = base + j * stride;
      if (gv < M) {
        const uint32_t key = __float_as_uint(tk_clamp(pt[j]));
        keys[gv] = key;
        atomicAdd(&lds[key >> TK_SHIFT0], 1u);
      }
    }
  }
  __syncthreads();
  tk_merge<TK_BINS0>(lds, hist);
}

// digit HI_SHIFT-1..SHIFT of the keys whose bits 31..HI_SHIFT equal the prefix
template <int BINS, int HI_SHIFT, int SHIFT>
__global__ __launch_bounds__(TK_THREADS) void tk_digit_kernel(const uint32_t* __restrict__ keys, int64_t M, const TkState* __restrict__ state,
                                                              unsigned long long* __restrict__ hist) {
  __shared__ uint32_t lds[BINS];
  for (int b = threadIdx.x; b < BINS; b += TK_THREADS) lds[b] = 0u;
  __syncthreads();
  const uint32_t want = state->prefix >> HI_SHIFT;
  auto count = [&](uint32_t key) {
    if ((key >> HI_SHIFT) == want) atomicAdd(&lds[(key >> SHIFT) & (uint32_t)(BINS - 1)], 1u);
  };
  // four keys per 16-byte load (the key array starts on a 256-byte boundary); the M & 3 keys of the tail go to workgroup 0
  const int64_t M4 = M >> 2;
  const uint4* __restrict__ keys4 = reinterpret_cast<const uint4*>(keys);
  for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < M4; i += (int64_t)gridDim.x * TK_THREADS) {
    const uint4 q = keys4[i];
    count(q.x); count(q.y); count(q.z); count(q.w);
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (M & 3)) count(keys[M4 * 4 + threadIdx.x]);
  __syncthreads();
  tk_merge<BINS>(lds, hist);
}

// One workgroup.  The bins hold `total` keys (M for the first digit, the chosen bucket's size afterwards) and 1 <= rank <= total:
// exactly one bin b has before(b) < rank <= before(b) + hist[b].  FIRST: the rank is the launch argument k and the prefix starts at 0.
template <int BINS, int SHIFT, bool FIRST>
__global__ __launch_bounds__(TK_THREADS) void tk_scan_kernel(const unsigned long long* __restrict__ hist, TkState* __restrict__ state,
                                                             unsigned long long k) {
  constexpr int PER = BINS / TK_THREADS;
  __shared__ unsigned long long part[2][TK_THREADS];
  const unsigned long long rank = FIRST ? k : state->rank;
  const uint32_t prefix = FIRST ? 0u : state->prefix;
  unsigned long long h[PER], mine = 0ull;
#pragma unroll
  for (int j = 0; j < PER; ++j) { h[j] = hist[threadIdx.x * PER + j]; mine += h[j]; }
  part[0][threadIdx.x] = mine;
  __syncthreads();                                   // (every thread has read the state before any thread writes it below)
  int cur = 0;                                       // inclusive prefix sums of the threads' shares, doubling the reach each round
  for (int o = 1; o < TK_THREADS; o <<= 1) {
    unsigned long long v = part[cur][threadIdx.x];
    if ((int)threadIdx.x >= o) v += part[cur][threadIdx.x - o];
    part[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  unsigned long long before = part[cur][threadIdx.x] - mine;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (before < rank && rank <= before + h[j]) {
      state->prefix = prefix | ((uint32_t)(threadIdx.x * PER + j) << SHIFT);
      state->rank = rank - before;
      state->count = h[j];
    }
    before += h[j];
  }
}

// slab[workgroup] = sum over the workgroup's voxels with key < tau of (double)l(key)
__global__ __launch_bounds__(TK_THREADS) void tk_sum_kernel(const uint32_t* __restrict__ keys, int64_t M, const TkState* __restrict__ state,
                                                            double* __restrict__ slab) {
  __shared__ double red[TK_THREADS / 64];
  const uint32_t tau = state->prefix;
  double acc = 0.0;
  auto add = [&](uint32_t key) {
    if (key < tau) acc += (double)tk_nll(__uint_as_float(key));
  };
  const int64_t M4 = M >> 2;
  const uint4* __restrict__ keys4 = reinterpret_cast<const uint4*>(keys);
  for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < M4; i += (int64_t)gridDim.x * TK_THREADS) {
    const uint4 q = keys4[i];
    add(q.x); add(q.y); add(q.z); add(q.w);
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (M & 3)) add(keys[M4 * 4 + threadIdx.x]);
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slab[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup stages the slab in LDS; one thread adds it in index order, then writes loss and coef
__global__ __launch_bounds__(TK_THREADS) void tk_finalize_kernel(const double* __restrict__ slab, int nslab, const TkState* __restrict__ state, const float* __restrict__ weight,
                                   double k, float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ double part[TK_MAX_GRID];
  for (int i = threadIdx.x; i < nslab; i += TK_THREADS) part[i] = slab[i];
  __syncthreads();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double S = 0.0;
  for (int i = 0; i < nslab; ++i) S += part[i];
  const uint32_t tau = state->prefix;
  const double kd = (double)weight[0] / k;
  loss[0] = (float)(kd * (S + (double)state->rank * (double)tk_nll(__uint_as_float(tau))));
  coef[0] = (float)kd;
  coef[1] = (float)((double)state->rank / (double)state->count);
  coef[2] = __uint_as_float(tau);                    // (tau <= bits(1.0f): an ordinary float, its bits survive the store)
  coef[3] = 0.f;
}

template <int C>
__global__ __launch_bounds__(TK_THREADS) void tk_bwd_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label, uint32_t posmask,
                                                            const float* __restrict__ coef, const float* __restrict__ gscale,
                                                            float* __restrict__ dprob, int64_t M) {
  const int64_t gv = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (gv >= M) return;
  const float g0 = gscale[0] * coef[0];
  const float g1 = g0 * coef[1];
  const uint32_t tau = __float_as_uint(coef[2]);
  const int t = tk_target<C>(label[gv], posmask);
  const float pc = tk_clamp(tk_pt<C>(prob, gv, t));
  const uint32_t key = __float_as_uint(pc);
  const float r = -1.0f / fmaxf(pc, TK_FLOOR);
  const float g = key < tau ? g0 * r : key == tau ? g1 * r : 0.f;
  if (C == 4) *reinterpret_cast<float4*>(dprob + gv * 4) = make_float4(t == 0 ? g : 0.f, t == 1 ? g : 0.f, t == 2 ? g : 0.f, t == 3 ? g : 0.f);
  else *reinterpret_cast<float2*>(dprob + gv * 2) = make_float2(t == 0 ? g : 0.f, t == 1 ? g : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t tk_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

#define TK_HIST_WORDS (TK_BINS0 + TK_BINS1 + TK_BINS2)
#define TK_HIST_BYTES ((int64_t)TK_HIST_WORDS * 8)
#define TK_STATE_BYTES 256
#define TK_SLAB_BYTES ((int64_t)TK_MAX_GRID * 8)

// M, or a negative CWF_E_*.  2^40 voxels keep a workgroup's share (M / TK_MAX_GRID at the most, rounded up) inside its 32-bit counters.
static int64_t tk_voxels(int N, int64_t V) {
  if (N <= 0 || V <= 0) return CWF_E_BADARG;
  if (V > ((int64_t)1 << 40) / N) return CWF_E_TOOLARGE;
  return (int64_t)N * V;
}

extern "C" int64_t cwf_topk_ce_workspace(int N, int64_t V) {
  const int64_t M = tk_voxels(N, V);
  if (M < 0) return M;
  return TK_HIST_BYTES + TK_STATE_BYTES + TK_SLAB_BYTES + tk_align(M * 4);
}

extern "C" int cwf_topk_ce(const float* prob, const int64_t* label, uint32_t posmask, int64_t k, const float* weight, float* loss, float* coef,
                           int N, int64_t V, int C, void* ws, void* stream) {
  if (!prob || !label || !weight || !loss || !coef || !ws || (C != 2 && C != 4)) return CWF_E_BADARG;
  const int64_t M = tk_voxels(N, V);
  if (M < 0) return (int)M;
  if (k < 1 || k > M) return CWF_E_BADARG;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  unsigned long long* h0 = (unsigned long long*)ws;
  unsigned long long* h1 = h0 + TK_BINS0;
  unsigned long long* h2 = h1 + TK_BINS1;
  TkState* state = (TkState*)((uint8_t*)ws + TK_HIST_BYTES);
  double* slab = (double*)((uint8_t*)ws + TK_HIST_BYTES + TK_STATE_BYTES);
  uint32_t* keys = (uint32_t*)((uint8_t*)ws + TK_HIST_BYTES + TK_STATE_BYTES + TK_SLAB_BYTES);
  const int nwg = (int)std::min<int64_t>(cdiv64(M, TK_THREADS), TK_MAX_GRID);
  const dim3 grid((unsigned)nwg), block(TK_THREADS), one(1);

  hipLaunchKernelGGL(tk_zero_kernel, dim3(cdiv(TK_HIST_WORDS, TK_THREADS)), block, 0, st, h0, TK_HIST_WORDS);
  CWF_LAUNCH_CHECK();
  if (C == 4) hipLaunchKernelGGL(tk_keys_kernel<4>, grid, block, 0, st, prob, label, posmask, M, keys, h0);
  else hipLaunchKernelGGL(tk_keys_kernel<2>, grid, block, 0, st, prob, label, posmask, M, keys, h0);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL((tk_scan_kernel<TK_BINS0, TK_SHIFT0, true>), one, block, 0, st, h0, state, (unsigned long long)k);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL((tk_digit_kernel<TK_BINS1, TK_SHIFT0, TK_SHIFT1>), grid, block, 0, st, keys, M, state, h1);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL((tk_scan_kernel<TK_BINS1, TK_SHIFT1, false>), one, block, 0, st, h1, state, 0ull);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL((tk_digit_kernel<TK_BINS2, TK_SHIFT1, 0>), grid, block, 0, st, keys, M, state, h2);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL((tk_scan_kernel<TK_BINS2, 0, false>), one, block, 0, st, h2, state, 0ull);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(tk_sum_kernel, grid, block, 0, st, keys, M, state, slab);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(tk_finalize_kernel, one, block, 0, st, slab, nwg, state, weight, (double)k, loss, coef);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_topk_ce_bwd(const float* prob, const int64_t* label, uint32_t posmask, const float* coef, const float* gscale, float* dprob,
                               int N, int64_t V, int C, void* stream) {
  if (!prob || !label || !coef || !gscale || !dprob || (C != 2 && C != 4)) return CWF_E_BADARG;
  const int64_t M = tk_voxels(N, V);
  if (M < 0) return (int)M;
  if (cdiv64(M, TK_THREADS) > 0x7fffffffll) return CWF_E_TOOLARGE;
  const dim3 grid((unsigned)cdiv64(M, TK_THREADS));
  if (C == 4) hipLaunchKernelGGL(tk_bwd_kernel<4>, grid, dim3(TK_THREADS), 0, cwf_stream(stream), prob, label, posmask, coef, gscale, dprob, M);
  else hipLaunchKernelGGL(tk_bwd_kernel<2>, grid, dim3(TK_THREADS), 0, cwf_stream(stream), prob, label, posmask, coef, gscale, dprob, M);
  CWF_LAUNCH_CHECK();
  return 0;
}
