// optim.hip — fused multi-tensor optimizers over the flat parameter buffer (gfx950).
//
// All trainable parameters of a model live in ONE fp32 master buffer, their
// gradients in ONE fp32 buffer (the same buffer RCCL all-reduces) and their bf16
// compute copies in ONE shadow buffer.  Each optimizer step is therefore a single
// streaming launch over ~N floats: read w, g (+ state), write w, state and the bf16
// shadow the next forward consumes.  The data-parallel 1/world average is folded in
// as grad_scale, so the all-reduce needs no separate scaling pass.
//
// Learning rate and step count are read from device memory, so a hipGraph-captured
// training step follows an LR schedule / Adam bias correction without re-capture.
//
// Semantics follow torch.optim.SGD (momentum, dampening, nesterov, weight_decay) and
// torch.optim.Adam / AdamW (L2 vs decoupled decay), which is what the reference's user
// code configures (function_lenet.py:77-79, function_resnet34.py:62, function_vgg11.py:54).
// Optimizer-state reset at every K-AVG round (reference network.py:121-128) is a
// hipMemsetAsync of the state buffers (kml_memset).
#include "kml_common.h"
#include "kml_sgd.h"

namespace {

// The data-sampler counter advance (k_advance's job) folded into an SGD launch: one thread, no
// other block reads the counter, the next step's augment reads it after the launch boundary.
__device__ __forceinline__ void fold_advance(float* __restrict__ adv_ctr, float adv_batch, float adv_n) {
  if (adv_ctr && blockIdx.x == 0 && threadIdx.x == 0) {
    adv_ctr[1] += 1.f;
    float st = adv_ctr[2] + adv_batch;
    if (st >= adv_n) st -= adv_n;
    adv_ctr[2] = st;
  }
}

__global__ void k_sgd(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                      bf16_t* __restrict__ shadow, const float* __restrict__ lr_ptr, float lr_host, float wd,
                      float momentum, float dampening, int nesterov, const float* __restrict__ first_ptr,
                      int first_host, float grad_scale, long long n, float* __restrict__ adv_ctr,
                      float adv_batch, float adv_n, const float* __restrict__ clip_ptr) {
  fold_advance(adv_ctr, adv_batch, adv_n);
  const float lr = lr_ptr ? *lr_ptr : lr_host;
  // first step after a reset (torch: momentum buffer := d, no dampening).  The flag lives
  // in device memory so a graph-captured step follows reset_state() between replays.
  const int first = first_ptr ? (*first_ptr != 0.f) : first_host;
  // global-norm clipping: the coefficient k_grad_norm left on the device scales the gradient
  if (clip_ptr) grad_scale *= *clip_ptr;
  kml_sgd_range(w, g, mom, shadow, lr, wd, momentum, dampening, nesterov, first, grad_scale, n,
                blockIdx.x * (long long)blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

// The groups' (lr, weight_decay) pairs, once per block into LDS; entries past G read as zeros and
// a lookup masks the byte to the table's 8 entries, so no byte of gid can index outside it.
__device__ __forceinline__ void load_group_table(float2* sh, const float* __restrict__ hp, int G) {
  if (threadIdx.x < KML_MAX_GROUPS)
    sh[threadIdx.x] = (int)threadIdx.x < G ? make_float2(hp[2 * threadIdx.x], hp[2 * threadIdx.x + 1])
                                           : make_float2(0.f, 0.f);
  __syncthreads();
}

// group of float4 `i` of a range that starts at element elem0 of the space
__device__ __forceinline__ int group_of(const unsigned char* __restrict__ gid, long long elem0, long long i) {
  return gid[(elem0 + 4 * i) >> KML_GRANULE_SHIFT] & (KML_MAX_GROUPS - 1);
}

// k_sgd with one (lr, weight_decay) per 64-element granule: the same single streaming launch and,
// through kml_sgd_vec4, the same element update.  n is a multiple of 64: no scalar tail.
__global__ void k_sgd_groups(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                             bf16_t* __restrict__ shadow, const unsigned char* __restrict__ gid,
                             const float* __restrict__ hp, int G, long long elem0, float momentum, float dampening,
                             int nesterov, const float* __restrict__ first_ptr, int first_host, float grad_scale,
                             long long n, float* __restrict__ adv_ctr, float adv_batch, float adv_n,
                             const float* __restrict__ clip_ptr) {
  __shared__ float2 sh_hp[KML_MAX_GROUPS];
  fold_advance(adv_ctr, adv_batch, adv_n);
  load_group_table(sh_hp, hp, G);
  const int first = first_ptr ? (*first_ptr != 0.f) : first_host;
  if (clip_ptr) grad_scale *= *clip_ptr;
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float2 h = sh_hp[group_of(gid, elem0, i)];
    kml_sgd_vec4(w, g, mom, shadow, h.x, h.y, momentum, dampening, nesterov, first, grad_scale, i);
  }
}

// The torch.optim.Adam / AdamW element update (L2 or decoupled decay) of float4 `i`, already loaded
// as W / G / M / V, and the stores of master, moments and bf16 shadow.  Shared by k_adam (one lr /
// wd per launch) and k_adam_groups (its granule's), so both give the same bits for the same values.
// step_size = lr / (1 - b1^t), rbc2 = rsqrt(1 - b2^t)
__device__ __forceinline__ void adam_vec4(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                          bf16_t* __restrict__ shadow, const float4& W, const float4& G,
                                          const float4& M, const float4& V, float lr, float wd, float step_size,
                                          float rbc2, float b1, float b2, float eps, int decoupled, float grad_scale,
                                          long long i) {
  float wv[4] = {W.x, W.y, W.z, W.w}, gv[4] = {G.x, G.y, G.z, G.w};
  float mv[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // The roundings are spelled out.  Left to -ffp-contract=fast, which product of
    // b * x + (1 - b) * y is fused, and whether sqrt(v) * rbc2 + eps is, depends on the surrounding
    // code (the vectoriser pairs some of the products first), so two kernels inlining this body
    // could round differently.  These are the forms k_adam has always compiled to, element by
    // element: its results must not change.  In particular the first three elements of a float4
    // round sqrt(v) * rbc2 before adding eps (that product was paired with step_size * m), the
    // fourth fuses the two.
    float gg = gv[k] * grad_scale;
    if (decoupled) wv[k] *= __builtin_fmaf(-lr, wd, 1.f);
    else gg = __builtin_fmaf(wd, wv[k], gg);
    mv[k] = __builtin_fmaf(b1, mv[k], (1.f - b1) * gg);
    vv[k] = __builtin_fmaf(b2, vv[k], (1.f - b2) * gg * gg);
    float denom;
    if (k < 3) {
      float q = sqrtf(vv[k]) * rbc2;
      asm volatile("" : "+v"(q));   // a rounded product of its own (contract pragmas are ignored)
      denom = q + eps;
    } else {
      denom = __builtin_fmaf(sqrtf(vv[k]), rbc2, eps);
    }
    wv[k] -= step_size * mv[k] / denom;
  }
  reinterpret_cast<float4*>(w)[i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
  reinterpret_cast<float4*>(m)[i] = make_float4(mv[0], mv[1], mv[2], mv[3]);
  reinterpret_cast<float4*>(v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
  if (shadow) {
    uint2 s;
    s.x = pack_bf2(wv[0], wv[1]);
    s.y = pack_bf2(wv[2], wv[3]);
    reinterpret_cast<uint2*>(shadow)[i] = s;
  }
}

__global__ void k_adam(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, bf16_t* __restrict__ shadow, const float* __restrict__ lr_ptr,
                       const float* __restrict__ step_ptr, float lr_host, float step_host, float b1, float b2,
                       float eps, float wd, int decoupled, float grad_scale, long long n,
                       const float* __restrict__ clip_ptr) {
  const float lr = lr_ptr ? *lr_ptr : lr_host;
  if (clip_ptr) grad_scale *= *clip_ptr;  // global-norm clipping coefficient (k_grad_norm)
  const float t = step_ptr ? *step_ptr : step_host;
  const float bc1 = 1.f - __powf(b1, t), bc2 = 1.f - __powf(b2, t);
  const float step_size = lr / bc1;
  const float rbc2 = rsqrtf(bc2);
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  // two float4 groups per thread and iteration, all eight loads issued before any math: the
  // 30-byte-per-parameter stream (4 reads, 3 writes, the bf16 shadow) keeps twice the bytes
  // in flight per wave (the one-group loop ran at ~78% of the achievable HBM rate)
  constexpr int U = 2;
  for (long long i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i0 < n4; i0 += U * stride) {
    float4 W[U], G[U], M[U], V[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = i0 + u * stride;
      if (i < n4) {
        W[u] = reinterpret_cast<float4*>(w)[i];
        G[u] = reinterpret_cast<const float4*>(g)[i];
        M[u] = reinterpret_cast<float4*>(m)[i];
        V[u] = reinterpret_cast<float4*>(v)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = i0 + u * stride;
      if (i >= n4) break;
      adam_vec4(w, m, v, shadow, W[u], G[u], M[u], V[u], lr, wd, step_size, rbc2, b1, b2, eps, decoupled,
                grad_scale, i);
    }
  }
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) {
    float gg = g[i] * grad_scale;
    float wi = w[i];
    if (decoupled) wi *= (1.f - lr * wd);
    else gg += wd * wi;
    m[i] = b1 * m[i] + (1.f - b1) * gg;
    v[i] = b2 * v[i] + (1.f - b2) * gg * gg;
    wi -= step_size * m[i] / (sqrtf(v[i]) * rbc2 + eps);
    w[i] = wi;
    if (shadow) shadow[i] = f2bf(wi);
  }
}

// k_adam with one (lr, weight_decay) per 64-element granule: the same single streaming launch, the
// same two-float4 unroll and, through adam_vec4, the same element update.  Each group's step size
// lr / (1 - b1^t) is formed once per block, as k_adam forms its one.  n is a multiple of 64.
__global__ void k_adam_groups(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                              float* __restrict__ v, bf16_t* __restrict__ shadow,
                              const unsigned char* __restrict__ gid, const float* __restrict__ hp, int G,
                              long long elem0, const float* __restrict__ step_ptr, float step_host, float b1,
                              float b2, float eps, int decoupled, float grad_scale, long long n,
                              const float* __restrict__ clip_ptr) {
  __shared__ float2 sh_hp[KML_MAX_GROUPS];
  __shared__ float sh_ss[KML_MAX_GROUPS];
  if (clip_ptr) grad_scale *= *clip_ptr;
  const float t = step_ptr ? *step_ptr : step_host;
  const float bc1 = 1.f - __powf(b1, t), bc2 = 1.f - __powf(b2, t);
  const float rbc2 = rsqrtf(bc2);
  if (threadIdx.x < KML_MAX_GROUPS) sh_ss[threadIdx.x] = (int)threadIdx.x < G ? hp[2 * threadIdx.x] / bc1 : 0.f;
  load_group_table(sh_hp, hp, G);
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  constexpr int U = 2;
  for (long long i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i0 < n4; i0 += U * stride) {
    float4 W[U], Gr[U], M[U], V[U];
    int grp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = i0 + u * stride;
      if (i < n4) {
        W[u] = reinterpret_cast<float4*>(w)[i];
        Gr[u] = reinterpret_cast<const float4*>(g)[i];
        M[u] = reinterpret_cast<float4*>(m)[i];
        V[u] = reinterpret_cast<float4*>(v)[i];
        grp[u] = group_of(gid, elem0, i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = i0 + u * stride;
      if (i >= n4) break;
      const float2 h = sh_hp[grp[u]];
      adam_vec4(w, m, v, shadow, W[u], Gr[u], M[u], V[u], h.x, h.y, sh_ss[grp[u]], rbc2, b1, b2, eps, decoupled,
                grad_scale, i);
    }
  }
}

__global__ void k_inc(float* p, float by) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += by; }

// ---- global-norm gradient clipping ----------------------------------------------------------
// One launch: every block sums the squares of its grid-stride share of g (fp32, fixed order) into
// part[blockIdx.x]; the last block to arrive (ticket on `counter`, which it resets to 0) folds the
// partials in index order and writes
//   out[0] = sum g^2
//   out[1] = grad_scale * sqrt(out[0])                 the norm of the averaged gradient
//   out[2] = min(1, *max_norm_ptr / (out[1] + 1e-6))   torch.nn.utils.clip_grad_norm_'s coefficient
// No atomics on the sums: the result is a function of (g, n, grid) only, bit for bit.  The
// threshold is read from device memory, so a graph-captured step follows a changed threshold.
constexpr int KML_NORM_MAX_BLOCKS = 1024;  // the final fold is one pass of 256 threads x 4

// every thread gets the block's sum (4 waves of 64); sh is reusable after the call's barrier pair
__device__ __forceinline__ float block_sum256(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_grad_norm(const float* __restrict__ g, long long n, float grad_scale,
                                                   const float* __restrict__ max_norm_ptr, float* __restrict__ part,
                                                   unsigned* __restrict__ counter, float* __restrict__ out) {
  __shared__ float sh[4];
  __shared__ unsigned last;
  const int tid = threadIdx.x;
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * 256;
  // four float4 groups per thread and iteration, all loads issued before the math (a read-only
  // stream: as k_adam's U = 2 with a quarter of its bytes per group), one accumulator per slot
  constexpr int U = 4;
  float acc[U] = {0.f, 0.f, 0.f, 0.f};
  long long i0 = blockIdx.x * 256LL + tid;
  // full iterations load unconditionally (a per-load bounds select makes the compiler branch
  // around every load and wait for each); the up to U - 1 groups left go one at a time
  for (; i0 + (U - 1) * stride < n4; i0 += U * stride) {
    float4 G[U];
#pragma unroll
    for (int u = 0; u < U; ++u) G[u] = reinterpret_cast<const float4*>(g)[i0 + u * stride];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[u] = fmaf(G[u].x, G[u].x, acc[u]);
      acc[u] = fmaf(G[u].y, G[u].y, acc[u]);
      acc[u] = fmaf(G[u].z, G[u].z, acc[u]);
      acc[u] = fmaf(G[u].w, G[u].w, acc[u]);
    }
  }
  for (; i0 < n4; i0 += stride) {
    const float4 v = reinterpret_cast<const float4*>(g)[i0];
    acc[0] = fmaf(v.x, v.x, acc[0]);
    acc[0] = fmaf(v.y, v.y, acc[0]);
    acc[0] = fmaf(v.z, v.z, acc[0]);
    acc[0] = fmaf(v.w, v.w, acc[0]);
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  for (long long i = (n4 << 2) + blockIdx.x * 256LL + tid; i < n; i += stride) s = fmaf(g[i], g[i], s);
  s = block_sum256(s, sh);
  // hand-off to the last arriver (the ticket of k_bn_bwd_reduce2): plain store, agent-scope release
  // before the ticket, acquire after it; the counter word is back at 0 when the launch ends
  if (tid == 0) {
    part[blockIdx.x] = s;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned l = (t == gridDim.x - 1) ? 1u : 0u;
    if (l) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last = l;
  }
  __syncthreads();
  if (!last) return;
  // partial b goes to thread b % 256, each thread adds its (at most 4) partials in index order;
  // agent-scope loads are served by the L2 / memory, never by this CU's L1
  float t = 0.f;
  for (int b = tid; b < (int)gridDim.x; b += 256)
    t += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  t = block_sum256(t, sh);
  if (tid == 0) {
    const float nrm = grad_scale * sqrtf(t);
    // c > 1 is false for a NaN norm, so NaN reaches the update (fminf would return 1); inf gives 0
    const float c = *max_norm_ptr / (nrm + 1e-6f);
    out[0] = t;
    out[1] = nrm;
    out[2] = c > 1.f ? 1.f : c;
  }
}

// x *= coef[0] (the eager in-place clip; coef = out + 2 of k_grad_norm).  A coefficient of exactly
// 1 leaves the buffer untouched; NaN is not 1 and poisons it.
__global__ void k_clip_scale(float* __restrict__ x, const float* __restrict__ coef, long long n) {
  const float c = *coef;
  if (c == 1.f) return;
  const long long n4 = n >> 2, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x *= c; v.y *= c; v.z *= c; v.w *= c;
    reinterpret_cast<float4*>(x)[i] = v;
  }
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= c;
}

}  // namespace

// NOTE: hipMemsetAsync is avoided on capturable paths (graph memset nodes raced with
// kernel nodes on this ROCm build); use kml_zero from util.hip.
KML_API int kml_memset(void* p, int value, long long bytes, hipStream_t s) {
  return (int)hipMemsetAsync(p, value, (size_t)bytes, s);
}

// Grid of a streaming optimizer launch over n elements, a float4 per thread.  max_blocks > 0 caps
// it (a range update running next to latency-bound backward kernels on a side stream should take
// a slice of the CUs, not all of them).
static inline unsigned kml_capped_grid(long long n, int max_blocks) {
  unsigned grid = kml_stream_grid((n + 3) / 4, 256);
  if (max_blocks > 0 && grid > (unsigned)max_blocks) grid = (unsigned)max_blocks;
  return grid;
}

KML_API int kml_sgd(float* w, const float* g, float* mom, bf16_t* shadow, const float* lr_ptr, float lr, float wd,
                    float momentum, float dampening, int nesterov, const float* first_ptr, int first,
                    float grad_scale, long long n, int max_blocks, float* adv_ctr, float adv_batch, float adv_n,
                    const float* clip_ptr, hipStream_t s) {
  const unsigned grid = kml_capped_grid(n, max_blocks);
  hipLaunchKernelGGL(k_sgd, dim3(grid), dim3(256), 0, s, w, g, mom, shadow, lr_ptr, lr, wd, momentum, dampening,
                     nesterov, first_ptr, first, grad_scale, n, adv_ctr, adv_batch, adv_n, clip_ptr);
  KML_LAUNCH_CHECK();
}

KML_API int kml_adam(float* w, const float* g, float* m, float* v, bf16_t* shadow, const float* lr_ptr,
                     const float* step_ptr, float lr, float step, float b1, float b2, float eps, float wd,
                     int decoupled, float grad_scale, long long n, int max_blocks, const float* clip_ptr,
                     hipStream_t s) {
  const unsigned grid = kml_capped_grid(n, max_blocks);
  hipLaunchKernelGGL(k_adam, dim3(grid), dim3(256), 0, s, w, g, m, v, shadow, lr_ptr,
                     step_ptr, lr, step, b1, b2, eps, wd, decoupled, grad_scale, n, clip_ptr);
  KML_LAUNCH_CHECK();
}

// what every grouped launch needs: whole granules (n % 64 == 0, the range starts on one), 16-byte
// aligned buffers (a null optional buffer passes) and 1..8 groups
static inline bool kml_groups_ok(long long n, long long elem0, int G, const void* gid, const void* hp,
                                 const void* a, const void* b, const void* c, const void* d, const void* e) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e;
  return n >= 0 && elem0 >= 0 && (n & 63) == 0 && (elem0 & 63) == 0 && G >= 1 && G <= KML_MAX_GROUPS && gid && hp &&
         a && b && (bits & 15) == 0;
}

// kml_sgd with per-granule (lr, weight_decay): gid is the byte table of the whole space (one group
// id per 64 elements), elem0 the offset of w / g / mom / shadow into that space, hp the fp32 device
// table hp[G][2].  Everything else as kml_sgd.
KML_API int kml_sgd_groups(float* w, const float* g, float* mom, bf16_t* shadow, const unsigned char* gid,
                           const float* hp, int G, long long elem0, float momentum, float dampening, int nesterov,
                           const float* first_ptr, int first, float grad_scale, long long n, int max_blocks,
                           float* adv_ctr, float adv_batch, float adv_n, const float* clip_ptr, hipStream_t s) {
  if (!kml_groups_ok(n, elem0, G, gid, hp, w, g, mom, shadow, nullptr)) return (int)hipErrorInvalidValue;
  const unsigned grid = kml_capped_grid(n, max_blocks);
  hipLaunchKernelGGL(k_sgd_groups, dim3(grid), dim3(256), 0, s, w, g, mom, shadow, gid, hp, G, elem0, momentum,
                     dampening, nesterov, first_ptr, first, grad_scale, n, adv_ctr, adv_batch, adv_n, clip_ptr);
  KML_LAUNCH_CHECK();
}

// kml_adam with per-granule (lr, weight_decay); gid / hp / G / elem0 as kml_sgd_groups
KML_API int kml_adam_groups(float* w, const float* g, float* m, float* v, bf16_t* shadow, const unsigned char* gid,
                            const float* hp, int G, long long elem0, const float* step_ptr, float step, float b1,
                            float b2, float eps, int decoupled, float grad_scale, long long n, int max_blocks,
                            const float* clip_ptr, hipStream_t s) {
  if (!m || !v || !kml_groups_ok(n, elem0, G, gid, hp, w, g, m, v, shadow)) return (int)hipErrorInvalidValue;
  const unsigned grid = kml_capped_grid(n, max_blocks);
  hipLaunchKernelGGL(k_adam_groups, dim3(grid), dim3(256), 0, s, w, g, m, v, shadow, gid, hp, G, elem0, step_ptr,
                     step, b1, b2, eps, decoupled, grad_scale, n, clip_ptr);
  KML_LAUNCH_CHECK();
}

KML_API int kml_increment(float* p, float by, hipStream_t s) {
  hipLaunchKernelGGL(k_inc, dim3(1), dim3(64), 0, s, p, by);
  KML_LAUNCH_CHECK();
}

// blocks of kml_grad_norm for n elements: a function of (n, max_blocks) only, so every rank of a
// data-parallel group (same n) sums in the same order; at most KML_NORM_MAX_BLOCKS
static inline unsigned kml_norm_grid(long long n, int max_blocks) {
  long long g = ((n >> 2) + 255) / 256;
  if (g > KML_NORM_MAX_BLOCKS) g = KML_NORM_MAX_BLOCKS;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// part: >= kml_norm_grid(n, max_blocks) floats of scratch; counter: one word, 0 on entry and on
// exit; out: 3 floats (sum of squares, norm of grad_scale * g, clip coefficient)
KML_API int kml_grad_norm(const float* g, long long n, float grad_scale, const float* max_norm_ptr, float* part,
                          unsigned* counter, float* out, int max_blocks, hipStream_t s) {
  if (n < 0 || !g || !max_norm_ptr || !part || !counter || !out || ((uintptr_t)g & 15)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grad_norm, dim3(kml_norm_grid(n, max_blocks)), dim3(256), 0, s, g, n, grad_scale,
                     max_norm_ptr, part, counter, out);
  KML_LAUNCH_CHECK();
}

KML_API int kml_scale_by_coef(float* g, const float* coef, long long n, hipStream_t s) {
  if (((uintptr_t)g & 15)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_clip_scale, dim3(kml_stream_grid((n + 3) / 4, 256)), dim3(256), 0, s, g, coef, n);
  KML_LAUNCH_CHECK();
}


// ---------------------------------------------------------------------------------------
// K-AVG model average over ONE persistent flat state buffer (reference: the TrainJob's
// merge, ml/pkg/model/model.go:249-302 + parallelSGD.go:26-54).  Layout of `state`:
//   [0, n_params)            fp32 master parameters (the optimizer's buffer)
//   [n_params, i64_off)      fp32 module buffers (BN running_mean / running_var)
//   [i64_off, i64_off+n_i64) int64 buffers (num_batches_tracked) carried as fp32
//   [count_idx]              1 if this rank contributes to the round, else 0
// pack:   i64 -> fp32 slots, count slot := participate (non-participants send zeros)
// <RCCL all-reduce SUM of the whole buffer on the caller's stream>
// finish: x *= 1/max(count, 1); bf16 shadow of the parameter range refreshed in the
//         same pass; int64 buffers := floor(average) (the reference's integer division)
// No host synchronisation: the divisor never leaves the device.
// ---------------------------------------------------------------------------------------
__global__ void k_kavg_pack(float* __restrict__ state, const long long* __restrict__ i64, long long i64_off,
                            int n_i64, long long count_idx, int participate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_i64) state[i64_off + i] = participate ? (float)i64[i] : 0.f;
  if (i == 0) state[count_idx] = participate ? 1.f : 0.f;
}

__global__ void k_kavg_finish(float* __restrict__ state, long long n_params, long long count_idx,
                              bf16_t* __restrict__ shadow, long long* __restrict__ i64, long long i64_off,
                              int n_i64) {
  const float inv = 1.f / fmaxf(state[count_idx], 1.f);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long n4 = count_idx >> 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<float4*>(state)[i];
    v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
    reinterpret_cast<float4*>(state)[i] = v;
    const long long e = i << 2;
    if (shadow && e + 3 < n_params) {
      uint2 s;
      s.x = pack_bf2(v.x, v.y);
      s.y = pack_bf2(v.z, v.w);
      reinterpret_cast<uint2*>(shadow)[i] = s;
    } else if (shadow) {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int k = 0; k < 4; ++k)
        if (e + k < n_params) shadow[e + k] = f2bf(vv[k]);
    }
    if (i64) {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int k = 0; k < 4; ++k) {
        const long long j = e + k - i64_off;
        if (j >= 0 && j < n_i64) i64[j] = (long long)floorf(vv[k] + 1e-3f);
      }
    }
  }
  for (long long e = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; e < count_idx; e += stride) {
    const float v = state[e] * inv;
    state[e] = v;
    if (shadow && e < n_params) shadow[e] = f2bf(v);
    const long long j = e - i64_off;
    if (i64 && j >= 0 && j < n_i64) i64[j] = (long long)floorf(v + 1e-3f);
  }
}

// Staleness-1 K-AVG (parallel/kavg.py AsyncModelAverager), two passes per round instead of six:
// launch: flat := x, snap := x (one read, two writes; flat then goes into the async SUM);
// apply:  x := x + (flat / world - snap), the bf16 shadow of the parameter range refreshed in
// the same pass (same operation order as the torch div / sub / add it replaces).
__global__ void k_kavg_snap(const float* __restrict__ x, float* __restrict__ flat, float* __restrict__ snap,
                            long long n) {
  const long long n4 = n >> 2, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<float4*>(flat)[i] = v;
    reinterpret_cast<float4*>(snap)[i] = v;
  }
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) {
    flat[i] = x[i];
    snap[i] = x[i];
  }
}

// x + (flat / world - snap): a multiply by the fp32 reciprocal (computed once on the host), then
// the subtraction and the addition, each rounded on its own (no contraction into an FMA)
__device__ __forceinline__ float kavg_step(float x, float f, float sn, float inv) {
  // the build's -ffp-contract=fast ignores contract pragmas: an empty asm on the product keeps
  // it a rounded value of its own, so the subtraction is not fused into an FMA
  float q = f * inv;
  asm volatile("" : "+v"(q));
  return x + (q - sn);
}

__global__ void k_kavg_async_apply(float* __restrict__ x, const float* __restrict__ flat,
                                   const float* __restrict__ snap, bf16_t* __restrict__ shadow, float inv,
                                   long long n, long long n_params) {
  const long long n4 = n >> 2, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    const float4 f = reinterpret_cast<const float4*>(flat)[i], sn = reinterpret_cast<const float4*>(snap)[i];
    v.x = kavg_step(v.x, f.x, sn.x, inv); v.y = kavg_step(v.y, f.y, sn.y, inv);
    v.z = kavg_step(v.z, f.z, sn.z, inv); v.w = kavg_step(v.w, f.w, sn.w, inv);
    reinterpret_cast<float4*>(x)[i] = v;
    if (shadow && 4 * i + 3 < n_params) {
      uint2 sh;
      sh.x = pack_bf2(v.x, v.y);
      sh.y = pack_bf2(v.z, v.w);
      reinterpret_cast<uint2*>(shadow)[i] = sh;
    } else if (shadow) {
      const float vv[4] = {v.x, v.y, v.z, v.w};
      for (int k = 0; k < 4; ++k)
        if (4 * i + k < n_params) shadow[4 * i + k] = f2bf(vv[k]);
    }
  }
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) {
    x[i] = kavg_step(x[i], flat[i], snap[i], inv);
    if (shadow && i < n_params) shadow[i] = f2bf(x[i]);
  }
}

KML_API int kml_kavg_snap(const float* x, float* flat, float* snap, long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_kavg_snap, dim3(kml_stream_grid((n + 3) / 4, 256)), dim3(256), 0, s, x, flat, snap, n);
  KML_LAUNCH_CHECK();
}

KML_API int kml_kavg_async_apply(float* x, const float* flat, const float* snap, bf16_t* shadow, float world,
                                 long long n, long long n_params, hipStream_t s) {
  hipLaunchKernelGGL(k_kavg_async_apply, dim3(kml_stream_grid((n + 3) / 4, 256)), dim3(256), 0, s, x, flat, snap,
                     shadow, 1.0f / world, n, n_params);
  KML_LAUNCH_CHECK();
}

KML_API int kml_kavg_pack(float* state, const long long* i64, long long i64_off, int n_i64, long long count_idx,
                          int participate, hipStream_t s) {
  const int n = n_i64 > 1 ? n_i64 : 1;
  hipLaunchKernelGGL(k_kavg_pack, dim3((n + 255) / 256), dim3(256), 0, s, state, i64, i64_off, n_i64, count_idx,
                     participate);
  KML_LAUNCH_CHECK();
}

KML_API int kml_kavg_finish(float* state, long long n_params, long long count_idx, bf16_t* shadow, long long* i64,
                            long long i64_off, int n_i64, hipStream_t s) {
  hipLaunchKernelGGL(k_kavg_finish, dim3(kml_stream_grid((count_idx + 3) / 4, 256)), dim3(256), 0, s, state,
                     n_params, count_idx, shadow, i64, i64_off, n_i64);
  KML_LAUNCH_CHECK();
}
