// lr_schedule.hip — per-step learning-rate schedules written on the device (gfx950).
//
// Every launch that consumes a learning rate reads it from device memory (the lr scalar of kml_sgd /
// kml_adam, column 0 of the grouped launches' [G][2] table and of the layer-wise [T][4] table, the SGD
// riders, the update inside the ZeRO-1 collective).  This launch writes those words: one block, once per
// step, after the step's last LR reader.  Everything that changes between replays of a captured step
// lives in device memory: ctl = [t, 0, 0, 0] (int32), pos = [x0, dx], base = the peak LR per row; the
// shape of the schedule is fixed per schedule object and travels as kernel arguments.
//
//   x = x0 + float(t') * dx,  t' = t + advance          (product, then sum: two roundings)
//   x < warmup (warmup > 0):  f = ws + (1 - ws) * (x / warmup)
//   else  q = clamp((x - warmup) / (total - warmup), 0, 1),  f = m + (1 - m) * d(q)
//   out[r * stride] = base[r] * f;  ctl[0] = t';  last = [x, f]
//
// constant, linear and step spell out every rounding (rounded() keeps -ffp-contract=fast from fusing a
// product into the following add), so kubeml_amd.optim.lr_factor gives the same bits with stock torch
// fp32 operations; cosine and a general power go through cosf / powf and are held to a tolerance.
#include "kml_common.h"

#define KML_LR_MILESTONES 8

namespace {

enum { LR_CONSTANT = 0, LR_LINEAR = 1, LR_POLYNOMIAL = 2, LR_COSINE = 3, LR_STEP = 4 };

struct LrMilestones {
  float v[KML_LR_MILESTONES];
};

// as in ema.hip: a value of its own, so the product before it is rounded and not fused (v_fma_f32)
__device__ __forceinline__ float rounded(float q) {
  asm volatile("" : "+v"(q));
  return q;
}

// a + b * c with two roundings
__device__ __forceinline__ float mul_add(float a, float b, float c) { return __fadd_rn(a, rounded(__fmul_rn(b, c))); }

__device__ __forceinline__ float lr_factor(float x, int kind, float warmup, float total, float m, float ws, float power,
                                           float gamma, int n_ms, const LrMilestones& ms) {
  if (warmup > 0.f && x < warmup) return mul_add(ws, __fsub_rn(1.f, ws), __fdiv_rn(x, warmup));
  if (kind == LR_STEP) {
    float d = 1.f;
    for (int k = 0; k < n_ms; ++k)
      if (ms.v[k] <= x) d = rounded(__fmul_rn(d, gamma));
    return d;
  }
  float q = __fdiv_rn(__fsub_rn(x, warmup), __fsub_rn(total, warmup));
  q = q < 0.f ? 0.f : (q > 1.f ? 1.f : q);
  float d = 1.f;
  if (kind == LR_LINEAR || (kind == LR_POLYNOMIAL && power == 1.f)) {
    d = __fsub_rn(1.f, q);
  } else if (kind == LR_POLYNOMIAL) {
    d = powf(__fsub_rn(1.f, q), power);
  } else if (kind == LR_COSINE) {
    d = __fmul_rn(0.5f, __fadd_rn(1.f, cosf(rounded(__fmul_rn(3.14159265358979323846f, q)))));
  }
  return mul_add(m, __fsub_rn(1.f, m), d);
}

__global__ __launch_bounds__(256) void k_lr_schedule(float* __restrict__ out, int rows, int stride,
                                                     const float* __restrict__ base, int* __restrict__ ctl,
                                                     const float* __restrict__ pos, float* __restrict__ last,
                                                     int advance, int kind, float warmup, float total, float m,
                                                     float ws, float power, float gamma, int n_ms, LrMilestones ms) {
  // every thread reads the counter before the barrier; thread 0 is its only writer, after it
  const int t = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + advance;
  const float x = mul_add(pos[0], (float)t, pos[1]);
  const float f = lr_factor(x, kind, warmup, total, m, ws, power, gamma, n_ms, ms);
  for (int r = threadIdx.x; r < rows; r += blockDim.x) out[(long long)r * stride] = __fmul_rn(base[r], f);
  __syncthreads();
  if (threadIdx.x == 0) {
    ctl[0] = t;
    last[0] = x;
    last[1] = f;
  }
}

}  // namespace

// out[r * stride] = base[r] * f(x) for r < rows (the other words of out stay untouched); ctl: int32 [4] =
// [t, 0, 0, 0]; pos: fp32 [2] = [x0, dx]; last: fp32 [2] = [x, f] of the LR just written.  x = x0 + float(t +
// advance) * dx, advance in {0, 1}; then ctl[0] = t + advance.  kind: 0 constant, 1 linear, 2 polynomial,
// 3 cosine, 4 step (gamma^k, k = milestones <= x, n_ms <= 8 of ms0..ms7; m and total unused).  The caller
// keeps t + advance < 2^24 (float(t) exact).
KML_API int kml_lr_schedule(float* out, int rows, int stride, const float* base, int* ctl, const float* pos,
                            float* last, int advance, int kind, float warmup, float total, float min_ratio,
                            float warmup_start, float power, float gamma, int n_ms, float ms0, float ms1, float ms2,
                            float ms3, float ms4, float ms5, float ms6, float ms7, hipStream_t s) {
  if (!out || !base || !ctl || !pos || !last || rows < 1 || stride < 1 || (advance != 0 && advance != 1) ||
      kind < LR_CONSTANT || kind > LR_STEP || n_ms < 0 || n_ms > KML_LR_MILESTONES || !(warmup >= 0.f) ||
      (kind != LR_STEP && !(total > warmup)))
    return (int)hipErrorInvalidValue;
  const LrMilestones ms = {{ms0, ms1, ms2, ms3, ms4, ms5, ms6, ms7}};
  hipLaunchKernelGGL(k_lr_schedule, dim3(1), dim3(256), 0, s, out, rows, stride, base, ctl, pos, last, advance, kind,
                     warmup, total, min_ratio, warmup_start, power, gamma, n_ms, ms);
  KML_LAUNCH_CHECK();
}
