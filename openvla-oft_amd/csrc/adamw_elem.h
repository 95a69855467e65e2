// adamw_elem.h -- the element update of the fused AdamW, shared by ovla_adamw (head_optim.hip) and ovla_adamw_clipped (grad_clip.hip): the two
// kernels differ only in how they form `grad`, the gradient in the parameter's precision, and call these functions for everything after it.
// ovla_adamw_master (adamw_master.hip) runs the fp32 update on an fp32 master copy and publishes its bf16 rounding.
#pragma once
#include <math.h>
#include "common.h"

struct AdamScalars {
  float decay, w1, beta2, w2, bc2_sqrt, eps, step_size, grad_scale;
};

// scalars exactly as torch/optim/adamw.py computes them (Python floats = double), then narrowed to the fp32 opmath type
template <class Args>
static inline AdamScalars adam_scalars(const Args& a) {
  const double bc1 = 1.0 - pow(a.beta1, (double)a.step);
  const double bc2 = 1.0 - pow(a.beta2, (double)a.step);
  AdamScalars s;
  s.decay = (float)(1.0 - a.lr * a.weight_decay);
  s.w1 = (float)(1.0 - a.beta1);
  s.beta2 = (float)a.beta2;
  s.w2 = (float)(1.0 - a.beta2);
  s.bc2_sqrt = (float)sqrt(bc2);
  s.eps = (float)a.eps;
  s.step_size = (float)(-(a.lr / bc1));
  s.grad_scale = a.grad_scale;
  return s;
}

// lerp as ATen's vectorised CPU kernel computes it (aten/src/ATen/native/cpu/LerpKernel.cpp):
// fmadd(|w| < 0.5 ? w : w - 1, b - a, |w| < 0.5 ? a : b)
OVLA_DEV float aten_lerp(float a, float b, float w) {
  return fabsf(w) < 0.5f ? __builtin_fmaf(w, b - a, a) : __builtin_fmaf(w - 1.f, b - a, b);
}

// `grad`: what autograd would have stored in the bf16 .grad (already rounded to bf16)
OVLA_DEV void adamw_elem_bf16(bf16_bits* __restrict__ p, bf16_bits* __restrict__ m, bf16_bits* __restrict__ v, int64_t i, float grad,
                              const AdamScalars& s) {
#pragma clang fp contract(off)  // keep ATen's operation order and roundings: no fused multiply-adds the reference lacks
  float pp = bfround(bf2f(p[i]) * s.decay);                  // param.mul_(1 - lr*wd)
  const float mm = bfround(aten_lerp(bf2f(m[i]), grad, s.w1));  // exp_avg.lerp_(grad, 1-beta1)
  float vv = bfround(bf2f(v[i]) * s.beta2);                  // exp_avg_sq.mul_(beta2)
  vv = bfround(vv + (s.w2 * grad) * grad);                   //   .addcmul_(grad, grad, value=1-beta2): self + value*t1*t2
  float d = bfround(sqrtf(vv));                              // exp_avg_sq.sqrt()
  d = bfround(d / s.bc2_sqrt);                               //   / bias_correction2_sqrt
  d = bfround(d + s.eps);                                    //   .add_(eps)
  pp = bfround(pp + (s.step_size * mm) / d);                 // param.addcdiv_(exp_avg, denom, value=-step_size): self + value*t1/t2
  p[i] = f2bf(pp);
  m[i] = f2bf(mm);
  v[i] = f2bf(vv);
}

// The fp32 element update by value: (p, m, v) in, (p, m, v) out.  adamw_elem_f32 below and ovla_adamw_master (adamw_master.hip, whose `p` is
// the fp32 master copy of a bf16 parameter) both call it, so the two agree bit for bit by construction.
struct AdamElemF32 {
  float p, m, v;
};
OVLA_DEV AdamElemF32 adamw_update_f32(float p, float m, float v, float grad, const AdamScalars& s) {
#pragma clang fp contract(off)
  float pp = p * s.decay;
  const float mm = aten_lerp(m, grad, s.w1);
  float vv = v * s.beta2;
  vv = vv + (s.w2 * grad) * grad;
  const float d = sqrtf(vv) / s.bc2_sqrt + s.eps;
  pp = pp + (s.step_size * mm) / d;
  return {pp, mm, vv};
}

OVLA_DEV void adamw_elem_f32(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int64_t i, float grad, const AdamScalars& s) {
  const AdamElemF32 r = adamw_update_f32(p[i], m[i], v[i], grad, s);
  p[i] = r.p;
  m[i] = r.m;
  v[i] = r.v;
}
