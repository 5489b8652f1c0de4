// K13 -- the tail of the training step on the flat gradient buffer (cwf.optim.GradSink.flat, 16.8 M floats): gradient accumulation
// over micro-batches (cwf_grad_add), the global gradient norm and its clip coefficient (cwf_grad_norm_clip, semantics of
// torch.nn.utils.clip_grad_norm_), and the fused Adam(amsgrad) launch of optim.hip extended by a device-resident gradient scale and
// an exponential moving average of the new weights (cwf_adam_amsgrad_ex).  All HBM-bound; nothing here reads the host.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// y = a + b (b == NULL: y = a) on arbitrary float-aligned slices.  y may BE a or b (the same address, not a shifted overlap): every
// element is read and written by one thread, loads before stores, so nothing is declared __restrict__.  When the pointers are
// congruent mod 16 the body moves float4s between `head` leading and `tail` trailing scalars; otherwise everything is scalar
// (nvec = 0, head = n).  Grid-stride, two independent float4s per thread and trip to keep enough loads in flight.
// ---------------------------------------------------------------------------------------------------------------------------------
#define GRAD_ADD_THREADS 256
#define GRAD_ADD_MAX_BLOCKS 1024

template <bool HAS_B>
__global__ __launch_bounds__(GRAD_ADD_THREADS) void grad_add_kernel(const float* a, const float* b, float* y, int64_t n, int64_t head, int64_t nvec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float4* a4 = reinterpret_cast<const float4*>(a + head);
  const float4* b4 = reinterpret_cast<const float4*>(HAS_B ? b + head : a);
  float4* y4 = reinterpret_cast<float4*>(y + head);
  int64_t i = tid;
  for (; i + stride < nvec; i += 2 * stride) {
    float4 u0 = a4[i], u1 = a4[i + stride];
    if (HAS_B) {
      const float4 w0 = b4[i], w1 = b4[i + stride];
      u0.x += w0.x; u0.y += w0.y; u0.z += w0.z; u0.w += w0.w;
      u1.x += w1.x; u1.y += w1.y; u1.z += w1.z; u1.w += w1.w;
    }
    y4[i] = u0; y4[i + stride] = u1;
  }
  if (i < nvec) {
    float4 u0 = a4[i];
    if (HAS_B) { const float4 w0 = b4[i]; u0.x += w0.x; u0.y += w0.y; u0.z += w0.z; u0.w += w0.w; }
    y4[i] = u0;
  }
  // scalar head [0, head) and tail [head + 4 nvec, n): at most three elements each on the vector path, everything on the scalar one
  for (int64_t j = tid; j < head; j += stride) y[j] = HAS_B ? a[j] + b[j] : a[j];
  for (int64_t j = head + 4 * nvec + tid; j < n; j += stride) y[j] = HAS_B ? a[j] + b[j] : a[j];
}

extern "C" int cwf_grad_add(const float* a, const float* b, float* y, int64_t n, void* stream) {
  if (!a || !y || n <= 0) return CWF_E_BADARG;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 3) return CWF_E_ALIGN;
  const unsigned ya = (unsigned)((uintptr_t)y & 15);
  const bool congruent = ((uintptr_t)a & 15) == ya && (!b || ((uintptr_t)b & 15) == ya);
  int64_t head = n, nvec = 0;
  if (congruent) {
    head = ((16 - ya) & 15) >> 2;
    if (head > n) head = n;
    nvec = (n - head) >> 2;
  }
  const int64_t work = nvec > 0 ? cdiv64(nvec, 2) : n;
  int64_t gx = cdiv64(work, GRAD_ADD_THREADS);
  if (gx > GRAD_ADD_MAX_BLOCKS) gx = GRAD_ADD_MAX_BLOCKS;
  if (b) hipLaunchKernelGGL(grad_add_kernel<true>, dim3((unsigned)gx), dim3(GRAD_ADD_THREADS), 0, cwf_stream(stream), a, b, y, n, head, nvec);
  else   hipLaunchKernelGGL(grad_add_kernel<false>, dim3((unsigned)gx), dim3(GRAD_ADD_THREADS), 0, cwf_stream(stream), a, b, y, n, head, nvec);
  CWF_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Global gradient norm.  Launch 1: CWF_GRADNORM_WS_DOUBLES workgroups, workgroup k owns the fixed contiguous range of 16-byte groups
// [k * per, (k + 1) * per) counted from the aligned address at or below g; every value is widened to double BEFORE squaring (1e30^2
// overflows float) and accumulated in double -- per thread in index order, then a fixed LDS tree -- and the workgroup stores its
// partial plainly (no atomics: the result is bit-identical from run to run).  Launch 2: one workgroup adds the partials in a fixed
// order and writes {coefficient, norm}.
// ---------------------------------------------------------------------------------------------------------------------------------
#define GRADNORM_THREADS 256
static_assert(CWF_GRADNORM_WS_DOUBLES % GRADNORM_THREADS == 0, "launch 2 reads the partials in whole rounds");

__device__ __forceinline__ double block_sum_f64(double s, double* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = GRADNORM_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// `shift` = floats between the aligned base and g (0..3); element i of g sits at virtual index i + shift
__global__ __launch_bounds__(GRADNORM_THREADS) void grad_sqsum_kernel(const float* __restrict__ g, int64_t n, int shift, int64_t per, double* __restrict__ partial) {
  __shared__ double red[GRADNORM_THREADS];
  const float* base = g - shift;                                   // 16-byte aligned; only [shift, shift + n) is ever read
  const int64_t vlo = shift, vhi = (int64_t)shift + n;
  const int64_t q0 = (int64_t)blockIdx.x * per, q1 = q0 + per;
  double s = 0.0;
#pragma unroll 2
  for (int64_t q = q0 + threadIdx.x; q < q1; q += GRADNORM_THREADS) {
    const int64_t v = 4 * q;
    if (v >= vhi) break;
    if (v >= vlo && v + 4 <= vhi) {
      const float4 x = *reinterpret_cast<const float4*>(base + v);
      const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
      s += x0 * x0; s += x1 * x1; s += x2 * x2; s += x3 * x3;
    } else {                                                       // the first / last group of the buffer: element by element
      for (int e = 0; e < 4; ++e)
        if (v + e >= vlo && v + e < vhi) { const double xe = (double)base[v + e]; s += xe * xe; }
    }
  }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(GRADNORM_THREADS) void grad_norm_finish_kernel(const double* __restrict__ partial, float grad_scale, float max_norm, float* __restrict__ out2) {
  __shared__ double red[GRADNORM_THREADS];
  double s = 0.0;
  for (int k = threadIdx.x; k < CWF_GRADNORM_WS_DOUBLES; k += GRADNORM_THREADS) s += partial[k];
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) {
    const double norm = (double)grad_scale * sqrt(s);               // norm of the AVERAGED gradient, before clipping
    double c = (double)max_norm / (norm + 1e-6);                    // torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6),
    c = c > 1.0 ? 1.0 : c;                                          // clamped to 1 (a NaN stays a NaN, as torch.clamp leaves it)
    out2[0] = (float)((double)grad_scale * c);
    out2[1] = (float)norm;
  }
}

extern "C" int cwf_grad_norm_clip(const float* g, int64_t n, float grad_scale, float max_norm, double* ws, float* out2, void* stream) {
  if (!g || !ws || !out2 || n <= 0 || !(max_norm >= 0.f) || grad_scale != grad_scale) return CWF_E_BADARG;
  if (((uintptr_t)g | (uintptr_t)out2) & 3 || ((uintptr_t)ws & 7)) return CWF_E_ALIGN;
  const int shift = (int)(((uintptr_t)g & 15) >> 2);
  const int64_t per = cdiv64(cdiv64(n + shift, 4), CWF_GRADNORM_WS_DOUBLES);
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3(CWF_GRADNORM_WS_DOUBLES), dim3(GRADNORM_THREADS), 0, cwf_stream(stream), g, n, shift, per, ws);
  CWF_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GRADNORM_THREADS), 0, cwf_stream(stream), (const double*)ws, grad_scale, max_norm, out2);
  CWF_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// adam_kernel of optim.hip, operation for operation, with two additions: the gradient scale may come from device memory (the clip
// coefficient of cwf_grad_norm_clip: it never visits the host), and the new parameter value, still in a register, is blended into
// an EMA copy of the weights: ema += w * (p_new - ema), Tensor.lerp_ in its weight < 0.5 form.
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool EMA>
__global__ void adam_ex_kernel(const cwf_adam_desc* __restrict__ table, const float* __restrict__ hyper, float step_size, float omb1, float beta2,
                               float omb2, float eps, float wd, float bc2_sqrt, int amsgrad, float gscale, const float* __restrict__ gscale_dev,
                               float* const* __restrict__ ema_table, float ema_w) {
  const cwf_adam_desc d = table[blockIdx.y];
  if (hyper) { step_size = hyper[0]; bc2_sqrt = hyper[1]; }
  if (gscale_dev) gscale = gscale_dev[0];
  float* ema = EMA ? ema_table[blockIdx.y] : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p = d.p[i];
    const float g = fmaf(wd, p, d.g[i] * gscale);
    const float m = d.m[i] + omb1 * (g - d.m[i]);
    const float v = beta2 * d.v[i] + omb2 * g * g;
    d.m[i] = m; d.v[i] = v;
    float vv = v;
    if (amsgrad) { vv = fmaxf(d.vmax[i], v); d.vmax[i] = vv; }
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    const float pn = p - step_size * (m / denom);
    d.p[i] = pn;
    if (EMA) { const float e = ema[i]; ema[i] = e + ema_w * (pn - e); }
  }
}

extern "C" int cwf_adam_amsgrad_ex(const struct cwf_adam_desc* table, int ntensors, int64_t max_n,
                                   double lr, double beta1, double beta2, double eps, double weight_decay, int step, int amsgrad,
                                   const float* hyper_dev, float grad_scale, const float* gscale_dev, float* const* ema_table, float ema_weight,
                                   void* stream) {
  if (!table || ntensors <= 0 || max_n <= 0 || (step <= 0 && !hyper_dev)) return CWF_E_BADARG;
  if (ema_table && !(ema_weight > 0.f && ema_weight <= 0.5f)) return CWF_E_BADARG;
  const double bc1 = 1.0 - pow(beta1, (double)(step > 0 ? step : 1));
  const double bc2 = 1.0 - pow(beta2, (double)(step > 0 ? step : 1));
  int64_t gx = cdiv64(max_n, 256); if (gx > 64) gx = 64;
  const dim3 grid((unsigned)gx, ntensors);
  if (ema_table)
    hipLaunchKernelGGL(adam_ex_kernel<true>, grid, dim3(256), 0, cwf_stream(stream), table, hyper_dev, (float)(lr / bc1), (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)sqrt(bc2), amsgrad, grad_scale, gscale_dev,
                       ema_table, ema_weight);
  else
    hipLaunchKernelGGL(adam_ex_kernel<false>, grid, dim3(256), 0, cwf_stream(stream), table, hyper_dev, (float)(lr / bc1), (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)sqrt(bc2), amsgrad, grad_scale, gscale_dev,
                       ema_table, ema_weight);
  CWF_LAUNCH_CHECK();
  return 0;
}
