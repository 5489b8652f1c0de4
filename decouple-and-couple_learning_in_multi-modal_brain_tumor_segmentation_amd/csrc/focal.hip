// L4 -- focal Tversky on class-bitmask regions + focal cross-entropy, one optional loss term.  This project's statement (restated in
// tests/focal_ref.py, derived in DESIGN.md):
//   prob    float32 [N, V, 4] channels-last; label int64 [N, V], class y = label & 3 (a foreign label reads inside its own voxel).
//           M = N V voxels; every sum below runs over the whole batch.
//   regions r < R (0 <= R <= 8), class bitmasks m_r over bits 0..3.  t_r = (m_r >> y) & 1;
//           p_r = 0.0f + p_c + ... over the classes of m_r in ascending class order, float32, every addition rounded.
//   sums    TP_r = sum t_r (double)p_r, SP_r = sum (double)p_r, ST_r = sum t_r (an exact integer), float64 accumulation.
//   Tversky FN = ST - TP, FP = SP - TP, num = TP + s, den = ((TP + a FN) + b FP) + s, TI = num / den, x = 1 - TI;
//           FT = (1 / R) sum_r (x > 0 ? x pow(x, e - 1) : 0), ascending r     (one pow call per region; e = 1: none, the term is x)
//   focal   q = fminf(fmaxf(p_y, 1e-7f), 1.0f), nl = -logf(q), om = 1.0f - q,
//   CE      pw = 1 | om | om om | (om om) om | powf(om, gamma) for gamma = 0 | 1 | 2 | 3 | anything else in [1, 5] (gamma and the class
//           weights k_c are rounded to float32 once, on the host);  SF = sum (double)k_y ((double)pw (double)nl), float64.
//   loss    = float32( w (FT + rho SF / M) ), w read from device memory.  R = 0: FT = 0.  rho = 0: no log, no power, SF = 0.
//   coef    float32 [2 R + 1]:  [2 r] = w (K_r A_r), [2 r + 1] = w (K_r B_r), [2 R] = w rho / M, with
//           K_r = -(e / R) pow(x, e - 1) (the same power), A_r = (den - num ((1 - a) - b)) / den^2, B_r = -(num b) / den^2,
//           and both entries of a region with x <= 0 are +0.
//   bwd     g = gscale[0];  u_r = t_r ? coef[2 r] + coef[2 r + 1] : coef[2 r + 1];  d_c = 0.0f + the u_r of the regions holding class c,
//           ascending r.  Where c = y and 1e-7 <= p_y <= 1 (torch's clamp rule):  l = logf(q),
//             h = -1 / q | l - om / q | (2 om) l - (om om) / q | (3 (om om)) l - ((om om) om) / q | (gamma powf(om, gamma - 1)) l - powf(om, gamma) / q
//             d_y += coef[2 R] (k_y h).   dprob[v][c] = g d_c.  Every operation float32, rounded on its own.
// This file is compiled with -ffp-contract=off.
//
// Pass structure (two launches forward, one backward; no host synchronisation, nothing read back, no float atomics, no workgroup waits
// on another):
//   focal_sums_kernel      the only pass over prob and label (24 B / voxel): a thread keeps 3 R + 1 accumulators, a workgroup reduces
//                          them (wave butterfly, then the four waves in order) and stores its 3 R + 1 partials to its row of the workspace
//   focal_finalize_kernel  one workgroup stages the rows in LDS 256 at a time; thread j adds column j in workgroup-index order; thread r
//                          then forms TI, the power and the two coefficients of region r, thread 0 the loss, all in float64
//   focal_bwd_kernel       the Tversky gradient of a voxel depends on its label alone: a 4 x 4 table (label class x channel) is built in
//                          LDS from coef; with rho = 0 prob is not even read.  One float4 store per voxel.
// The workspace is fully written before it is read: it may hold anything on entry.
#include <algorithm>
#include <cmath>
#include "common.h"

#define FO_THREADS 256
#define FO_MAX_GRID 1024                 // workgroups of the sums pass = rows of the partial table
#define FO_MAX_R 8
#define FO_MAX_COLS (3 * FO_MAX_R + 1)
#define FO_BATCH 4                       // voxels a thread loads together
#define FO_STAGE 256                     // rows the finalize stages at a time (256 x 25 doubles = 51,200 B of LDS)
#define FO_FLOOR 1e-7f

// how (1 - q)^gamma is formed
enum { FO_CE_OFF = 0, FO_G0 = 1, FO_G1 = 2, FO_G2 = 3, FO_G3 = 4, FO_POW = 5 };

struct FoMasks { uint32_t m[FO_MAX_R]; };
struct FoCe { int mode; float gamma; float k[4]; };
struct FoTv { double a, b, e, s, rho; };

__device__ __forceinline__ float fo_pick(const float4 q, int c) { return c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w; }

__device__ __forceinline__ float fo_class_weight(const FoCe& ce, int c) { return c == 0 ? ce.k[0] : c == 1 ? ce.k[1] : c == 2 ? ce.k[2] : ce.k[3]; }

__device__ __forceinline__ float fo_region_prob(const float4 q, uint32_t m) {
  float pr = 0.0f;
  if (m & 1u) pr += q.x;
  if (m & 2u) pr += q.y;
  if (m & 4u) pr += q.z;
  if (m & 8u) pr += q.w;
  return pr;
}

__device__ __forceinline__ float fo_power(float om, int mode, float gamma) {
  switch (mode) {
    case FO_G0: return 1.0f;
    case FO_G1: return om;
    case FO_G2: return om * om;
    case FO_G3: return (om * om) * om;
    default: return powf(om, gamma);
  }
}

__device__ __forceinline__ uint32_t fo_wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// row blockIdx.x of the partial table: TP_0.., SP_0.., ST_0.., SF
template <int R>
__global__ __launch_bounds__(FO_THREADS) void focal_sums_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label, FoMasks masks,
                                                                FoCe ce, int64_t M, double* __restrict__ ws) {
  constexpr int RR = R ? R : 1;
  constexpr int NC = 3 * R + 1;
  __shared__ double red[FO_THREADS / 64][FO_MAX_COLS];
  double tp[RR], sp[RR], sf = 0.0;
  uint32_t st[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) { tp[r] = 0.0; sp[r] = 0.0; st[r] = 0u; }
  const float4* __restrict__ prob4 = reinterpret_cast<const float4*>(prob);
  const int64_t stride = (int64_t)gridDim.x * FO_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * FO_THREADS + threadIdx.x; base < M; base += stride * FO_BATCH) {
    float4 q[FO_BATCH];
    int y[FO_BATCH];
#pragma unroll
    for (int j = 0; j < FO_BATCH; ++j) {
      const int64_t gv = base + j * stride;
      if (gv < M) { q[j] = prob4[gv]; y[j] = (int)(label[gv] & 3); }
      else { q[j] = make_float4(0.f, 0.f, 0.f, 0.f); y[j] = -1; }
    }
#pragma unroll
    for (int j = 0; j < FO_BATCH; ++j) {
      if (y[j] < 0) continue;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double pr = (double)fo_region_prob(q[j], masks.m[r]);
        sp[r] += pr;
        if ((masks.m[r] >> y[j]) & 1u) { tp[r] += pr; st[r] += 1u; }
      }
      if (ce.mode != FO_CE_OFF) {
        const float qc = fminf(fmaxf(fo_pick(q[j], y[j]), FO_FLOOR), 1.0f);
        const float nl = -logf(qc);
        const float pw = fo_power(1.0f - qc, ce.mode, ce.gamma);
        sf += (double)fo_class_weight(ce, y[j]) * ((double)pw * (double)nl);
      }
    }
  }
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double a = wave_sum_d(tp[r]), b = wave_sum_d(sp[r]);
    const uint32_t c = fo_wave_sum_u32(st[r]);
    if (lead) { red[wave][r] = a; red[wave][R + r] = b; red[wave][2 * R + r] = (double)c; }
  }
  sf = wave_sum_d(sf);
  if (lead) red[wave][3 * R] = sf;
  __syncthreads();
  if (threadIdx.x < NC) {
    const int j = threadIdx.x;
    ws[(int64_t)blockIdx.x * NC + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

__global__ __launch_bounds__(FO_THREADS) void focal_finalize_kernel(const double* __restrict__ ws, int nrows, int R, FoTv tv, const float* __restrict__ weight,
                                                                    double M, float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ double stage[FO_STAGE * FO_MAX_COLS];
  __shared__ double tot[FO_MAX_COLS];
  __shared__ double term[FO_MAX_R];
  const int nc = 3 * R + 1;
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int base = 0; base < nrows; base += FO_STAGE) {
    const int cnt = min(FO_STAGE, nrows - base);
    for (int i = tid; i < cnt * nc; i += FO_THREADS) stage[i] = ws[(int64_t)base * nc + i];
    __syncthreads();
    if (tid < nc) {
#pragma unroll 8
      for (int i = 0; i < cnt; ++i) acc += stage[i * nc + tid];      // workgroup-index order (unrolled: the LDS reads run ahead of the adds)
    }
    __syncthreads();
  }
  if (tid < nc) tot[tid] = acc;
  __syncthreads();
  const double w = (double)weight[0];
  if (tid < R) {                                     // one lane per region: the pow calls, the long part, run side by side
    const int r = tid;
    const double TP = tot[r], SP = tot[R + r], ST = tot[2 * R + r];
    const double FN = ST - TP, FP = SP - TP;
    const double num = TP + tv.s;
    const double den = ((TP + tv.a * FN) + tv.b * FP) + tv.s;
    const double x = 1.0 - num / den;
    double xe = 0.0;
    float ct = 0.0f, c1 = 0.0f;
    if (x > 0.0) {
      const double pw1 = (tv.e == 1.0) ? 1.0 : pow(x, tv.e - 1.0);
      xe = x * pw1;
      const double K = -(tv.e / (double)R) * pw1;
      const double A = (den - num * ((1.0 - tv.a) - tv.b)) / (den * den);
      const double B = -(num * tv.b) / (den * den);
      ct = (float)(w * (K * A));
      c1 = (float)(w * (K * B));
    }
    coef[2 * r] = ct;
    coef[2 * r + 1] = c1;
    term[r] = xe;
  }
  __syncthreads();
  if (tid != 0) return;
  double ft = 0.0;
  for (int r = 0; r < R; ++r) ft += term[r];          // ascending r
  if (R > 0) ft = ft / (double)R;
  double total = ft;
  if (tv.rho != 0.0) total = ft + tv.rho * (tot[3 * R] / M);
  loss[0] = (float)(w * total);
  coef[2 * R] = (float)(w * tv.rho / M);
}

__global__ __launch_bounds__(FO_THREADS) void focal_bwd_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label, FoMasks masks, int R, FoCe ce,
                                                               const float* __restrict__ coef, const float* __restrict__ gscale,
                                                               float* __restrict__ dprob, int64_t M) {
  __shared__ float4 tab[4];                          // tab[y] = the Tversky part of (d_0, d_1, d_2, d_3) of a voxel labelled y
  if (threadIdx.x < 16) {
    const int y = threadIdx.x >> 2, c = threadIdx.x & 3;
    float d = 0.0f;
    for (int r = 0; r < R; ++r) {
      if ((masks.m[r] >> c) & 1u) {
        const float u = ((masks.m[r] >> y) & 1u) ? coef[2 * r] + coef[2 * r + 1] : coef[2 * r + 1];
        d += u;
      }
    }
    reinterpret_cast<float*>(tab)[threadIdx.x] = d;
  }
  __syncthreads();
  const float g = gscale[0];
  const float cf = coef[2 * R];
  const float4* __restrict__ prob4 = reinterpret_cast<const float4*>(prob);
  float4* __restrict__ dprob4 = reinterpret_cast<float4*>(dprob);
  const int64_t base = (int64_t)blockIdx.x * (FO_THREADS * FO_BATCH) + threadIdx.x;
  float4 q[FO_BATCH];
  int y[FO_BATCH];
#pragma unroll
  for (int j = 0; j < FO_BATCH; ++j) {
    const int64_t gv = base + j * FO_THREADS;
    y[j] = gv < M ? (int)(label[gv] & 3) : -1;
    q[j] = (gv < M && ce.mode != FO_CE_OFF) ? prob4[gv] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < FO_BATCH; ++j) {
    if (y[j] < 0) continue;
    float4 d = tab[y[j]];
    if (ce.mode != FO_CE_OFF) {
      const float py = fo_pick(q[j], y[j]);
      if (py >= FO_FLOOR && py <= 1.0f) {              // (then q = p_y; NaN passes neither comparison)
        const float om = 1.0f - py;
        float h;
        switch (ce.mode) {
          case FO_G0: h = -1.0f / py; break;
          case FO_G1: h = logf(py) - om / py; break;
          case FO_G2: h = (2.0f * om) * logf(py) - (om * om) / py; break;
          case FO_G3: h = (3.0f * (om * om)) * logf(py) - ((om * om) * om) / py; break;
          default: h = (ce.gamma * powf(om, ce.gamma - 1.0f)) * logf(py) - powf(om, ce.gamma) / py; break;
        }
        const float f = cf * (fo_class_weight(ce, y[j]) * h);
        if (y[j] == 0) d.x += f; else if (y[j] == 1) d.y += f; else if (y[j] == 2) d.z += f; else d.w += f;
      }
    }
    dprob4[base + j * FO_THREADS] = make_float4(g * d.x, g * d.y, g * d.z, g * d.w);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t fo_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

// M, or a negative CWF_E_*
static int64_t fo_voxels(int N, int64_t V) {
  if (N <= 0 || V <= 0) return CWF_E_BADARG;
  if (V > ((int64_t)1 << 40) / N) return CWF_E_TOOLARGE;
  return (int64_t)N * V;
}

static int fo_rows(int64_t M) { return (int)std::min<int64_t>(cdiv64(M, FO_THREADS * FO_BATCH), FO_MAX_GRID); }

// the regions and the parameters, checked; fills the kernels' argument blocks
static int fo_setup(const uint32_t* posmasks, int R, const struct cwf_focal_params* p, FoMasks& masks, FoCe& ce, FoTv& tv) {
  if (R < 0 || R > FO_MAX_R || !p || (R > 0 && !posmasks)) return CWF_E_BADARG;
  for (int r = 0; r < FO_MAX_R; ++r) masks.m[r] = 0u;
  for (int r = 0; r < R; ++r) {
    if (posmasks[r] == 0u || posmasks[r] > 15u) return CWF_E_BADARG;
    masks.m[r] = posmasks[r];
  }
  if (!std::isfinite(p->fn) || !std::isfinite(p->fp) || p->fn < 0.0 || p->fp < 0.0 || !(p->fn + p->fp > 0.0)) return CWF_E_BADARG;
  if (!(p->exponent > 0.0 && p->exponent <= 4.0)) return CWF_E_BADARG;
  if (!std::isfinite(p->smooth) || !(p->smooth > 0.0)) return CWF_E_BADARG;
  if (!(p->gamma == 0.0 || (p->gamma >= 1.0 && p->gamma <= 5.0))) return CWF_E_BADARG;
  if (!std::isfinite(p->ce_ratio) || p->ce_ratio < 0.0) return CWF_E_BADARG;
  for (int c = 0; c < 4; ++c)
    if (!std::isfinite(p->class_weight[c]) || p->class_weight[c] < 0.0) return CWF_E_BADARG;
  if (R == 0 && !(p->ce_ratio > 0.0)) return CWF_E_BADARG;           // both parts off
  tv.a = p->fn; tv.b = p->fp; tv.e = p->exponent; tv.s = p->smooth; tv.rho = p->ce_ratio;
  ce.gamma = (float)p->gamma;
  for (int c = 0; c < 4; ++c) ce.k[c] = (float)p->class_weight[c];
  ce.mode = p->ce_ratio == 0.0 ? FO_CE_OFF
          : ce.gamma == 0.0f ? FO_G0 : ce.gamma == 1.0f ? FO_G1 : ce.gamma == 2.0f ? FO_G2 : ce.gamma == 3.0f ? FO_G3 : FO_POW;
  return 0;
}

extern "C" int64_t cwf_focal_workspace(int N, int64_t V, int R) {
  const int64_t M = fo_voxels(N, V);
  if (M < 0) return M;
  if (R < 0 || R > FO_MAX_R) return CWF_E_BADARG;
  return fo_align((int64_t)FO_MAX_GRID * (3 * R + 1) * 8);
}

#define FO_FOR_R(R, CALL)                                                                                  \
  switch (R) {                                                                                             \
    case 0: CALL(0); break; case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;       \
  }

extern "C" int cwf_focal_loss(const float* prob, const int64_t* label, const uint32_t* posmasks, int R, const struct cwf_focal_params* params,
                              const float* weight, float* loss, float* coef, int N, int64_t V, int C, void* ws, void* stream) {
  if (!prob || !label || !weight || !loss || !coef || !ws || C != 4) return CWF_E_BADARG;
  const int64_t M = fo_voxels(N, V);
  if (M < 0) return (int)M;
  FoMasks masks; FoCe ce; FoTv tv;
  const int rc = fo_setup(posmasks, R, params, masks, ce, tv);
  if (rc) return rc;
  if ((uintptr_t)ws & 255) return CWF_E_ALIGN;
  if (((uintptr_t)prob & 15) || ((uintptr_t)label & 7) || ((uintptr_t)loss & 3) || ((uintptr_t)coef & 3)) return CWF_E_ALIGN;
  hipStream_t st = cwf_stream(stream);
  const int rows = fo_rows(M);
  const dim3 grid((unsigned)rows), block(FO_THREADS);
#define FO_SUMS(RV) hipLaunchKernelGGL(focal_sums_kernel<RV>, grid, block, 0, st, prob, label, masks, ce, M, (double*)ws)
  FO_FOR_R(R, FO_SUMS)
#undef FO_SUMS
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), block, 0, st, (const double*)ws, rows, R, tv, weight, (double)M, loss, coef);
  CWF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cwf_focal_loss_bwd(const float* prob, const int64_t* label, const uint32_t* posmasks, int R, const struct cwf_focal_params* params,
                                  const float* coef, const float* gscale, float* dprob, int N, int64_t V, int C, void* stream) {
  if (!prob || !label || !coef || !gscale || !dprob || C != 4) return CWF_E_BADARG;
  const int64_t M = fo_voxels(N, V);
  if (M < 0) return (int)M;
  FoMasks masks; FoCe ce; FoTv tv;
  const int rc = fo_setup(posmasks, R, params, masks, ce, tv);
  if (rc) return rc;
  if (((uintptr_t)prob & 15) || ((uintptr_t)dprob & 15) || ((uintptr_t)label & 7)) return CWF_E_ALIGN;
  const int64_t nwg = cdiv64(M, FO_THREADS * FO_BATCH);
  if (nwg > 0x7fffffffll) return CWF_E_TOOLARGE;
  hipLaunchKernelGGL(focal_bwd_kernel, dim3((unsigned)nwg), dim3(FO_THREADS), 0, cwf_stream(stream), prob, label, masks, R, ce, coef, gscale,
                     dprob, M);
  CWF_LAUNCH_CHECK();
  return 0;
}
