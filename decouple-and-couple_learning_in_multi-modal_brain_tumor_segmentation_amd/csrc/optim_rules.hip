// K14 -- the update rules of the fused step beside Adam with L2 decay (optim.hip / grad_step.hip): AdamW (torch.optim.AdamW, decay
// applied to the weight, not the gradient) and SGD with momentum / Nesterov (torch.optim.SGD), over the same cwf_adam_desc table, with
// the same step controls (device-resident gradient scale, EMA of the new weights) and a per-tensor weight-decay multiplier.
// HBM-bound; one float per access (gradient slices of the flat buffer are 4-byte aligned only), so an element's result does not
// depend on where its tensor starts.  This file is compiled with -ffp-contract=off: every statement below is the rounding it shows,
// and a fused multiply-add is one only where fmaf says so.
#include "common.h"

struct optim_rule_args {
  const cwf_adam_desc* table;
  const float* hyper;          // AdamW, nullable: {step_size, bc2_sqrt}
  const float* wd_mul;         // nullable: per-tensor multiplier of the decay
  const float* gscale_dev;     // nullable: replaces gscale
  float* const* ema_table;     // EMA only
  double decay;                // AdamW: lr * weight_decay; SGD: weight_decay -- multiplied by wd_mul[t] in double, once per workgroup
  float lr;                    // AdamW: step_size = lr / (1 - beta1^t); SGD: lr
  float omb1, beta2, omb2, eps, bc2_sqrt;
  float mu, omd;               // SGD: momentum, 1 - dampening
  float gscale, ema_w;
  int amsgrad, nesterov, first;
};

template <int RULE, bool EMA>
__global__ __launch_bounds__(256) void optim_rule_kernel(const optim_rule_args a) {
  const cwf_adam_desc d = a.table[blockIdx.y];
  const double wdm = a.decay * (double)(a.wd_mul ? a.wd_mul[blockIdx.y] : 1.f);
  const float gscale = a.gscale_dev ? a.gscale_dev[0] : a.gscale;
  float* ema = EMA ? a.ema_table[blockIdx.y] : nullptr;
  float step_size = a.lr, bc2_sqrt = a.bc2_sqrt;
  if (RULE == CWF_RULE_ADAMW && a.hyper) { step_size = a.hyper[0]; bc2_sqrt = a.hyper[1]; }
  const float keep = (float)(1.0 - wdm);                             // AdamW: param.mul_(1 - lr * weight_decay)
  const float wd = (float)wdm;                                       // SGD: grad.add(param, alpha=weight_decay)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * blockDim.x) {
    // Every load of the element first, every store after: nothing here is __restrict__ (a table row could name any address), so a
    // load written after a store would wait for it -- for the EMA, a second round trip to HBM per element.  The tensors of
    // a row are distinct allocations and element i belongs to this thread alone, so the order of loads and stores changes no value.
    const float p = d.p[i];
    float g = d.g[i] * gscale;
    const float e = EMA ? ema[i] : 0.f;
    float pn;
    if (RULE == CWF_RULE_ADAMW) {
      const float m0 = d.m[i], v0 = d.v[i];
      const float x0 = a.amsgrad ? d.vmax[i] : 0.f;
      const float pd = p * keep;
      const float m = m0 + a.omb1 * (g - m0);                        // exp_avg.lerp_(grad, 1 - beta1)
      const float v = a.beta2 * v0 + a.omb2 * g * g;                 // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
      d.m[i] = m; d.v[i] = v;
      float vv = v;
      if (a.amsgrad) { vv = fmaxf(x0, v); d.vmax[i] = vv; }
      const float denom = sqrtf(vv) / bc2_sqrt + a.eps;
      pn = fmaf(-step_size, m / denom, pd);                          // param.addcdiv_(exp_avg, denom, value=-step_size)
    } else {
      const bool has_buf = a.mu > 0.f;
      const float b0 = has_buf && !a.first ? d.m[i] : 0.f;
      g = fmaf(wd, p, g);
      if (has_buf) {
        float b = g;                                                 // first update: momentum_buffer = clone(grad)
        if (!a.first) b = fmaf(a.omd, g, a.mu * b0);                 // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
        d.m[i] = b;
        g = a.nesterov ? fmaf(a.mu, b, g) : b;                       // grad.add(buf, alpha=momentum) | buf
      }
      pn = fmaf(-step_size, g, p);                                   // param.add_(grad, alpha=-lr)
    }
    d.p[i] = pn;
    if (EMA) ema[i] = e + a.ema_w * (pn - e);
  }
}

template <int RULE>
static void launch_optim_rule(const optim_rule_args& a, dim3 grid, hipStream_t st) {
  if (a.ema_table) hipLaunchKernelGGL((optim_rule_kernel<RULE, true>), grid, dim3(256), 0, st, a);
  else             hipLaunchKernelGGL((optim_rule_kernel<RULE, false>), grid, dim3(256), 0, st, a);
}

static inline bool nonneg(double x) { return x >= 0.0; }             // false for a NaN

extern "C" int cwf_optim_step(int rule, const struct cwf_adam_desc* table, int ntensors, int64_t max_n, double lr, double weight_decay,
                              const float* wd_mul, double beta1, double beta2, double eps, int step, int amsgrad, const float* hyper_dev,
                              double momentum, double dampening, int nesterov, int first,
                              float grad_scale, const float* gscale_dev, float* const* ema_table, float ema_weight, void* stream) {
  if (!table || ntensors <= 0 || max_n <= 0 || (rule != CWF_RULE_ADAMW && rule != CWF_RULE_SGD)) return CWF_E_BADARG;
  if (!nonneg(lr) || !nonneg(weight_decay) || !nonneg(momentum) || !nonneg(dampening)) return CWF_E_BADARG;
  if (ema_table && !(ema_weight > 0.f && ema_weight <= 0.5f)) return CWF_E_BADARG;
  optim_rule_args a = {};
  a.table = table; a.wd_mul = wd_mul; a.gscale_dev = gscale_dev; a.ema_table = ema_table;
  a.gscale = grad_scale; a.ema_w = ema_weight;
  if (rule == CWF_RULE_ADAMW) {
    if (step <= 0 && !hyper_dev) return CWF_E_BADARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !nonneg(eps)) return CWF_E_BADARG;
    const double bc1 = 1.0 - pow(beta1, (double)(step > 0 ? step : 1));
    const double bc2 = 1.0 - pow(beta2, (double)(step > 0 ? step : 1));
    a.hyper = hyper_dev; a.decay = lr * weight_decay; a.lr = (float)(lr / bc1);
    a.omb1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps; a.bc2_sqrt = (float)sqrt(bc2);
    a.amsgrad = amsgrad;
  } else {
    a.decay = weight_decay; a.lr = (float)lr; a.mu = (float)momentum; a.omd = (float)(1.0 - dampening);
    if (nesterov && (!(a.mu > 0.f) || dampening != 0.0)) return CWF_E_BADARG;
    a.nesterov = nesterov; a.first = first;
  }
  int64_t gx = cdiv64(max_n, 256); if (gx > 64) gx = 64;
  const dim3 grid((unsigned)gx, ntensors);
  if (rule == CWF_RULE_ADAMW) launch_optim_rule<CWF_RULE_ADAMW>(a, grid, cwf_stream(stream));
  else                        launch_optim_rule<CWF_RULE_SGD>(a, grid, cwf_stream(stream));
  CWF_LAUNCH_CHECK();
  return 0;
}
