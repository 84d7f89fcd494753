// ema.hip — exponential moving average of the flat fp32 state prefix (gfx950).
//
// Parameters (storage layout) and fp32 module buffers (BN running statistics) are one contiguous
// fp32 prefix of FlatParamSpace.state, so the average is ONE streaming launch over one buffer, run
// after every update of the master (end-of-step optimizer launch, SGD riders, per-stage ranges).
//
// Everything that changes per step lives in device memory, so one captured launch serves every
// replay: ctl = [ticks, updates, applied, 0] (int32) gates the launch (update_every) and drives
// timm's decay warm-up, aout[0] is the weight 1 - d the launch ran with.  The last block to arrive
// (ticket, as advance_tail in decode.hip) advances the counters; every block read them at entry.
//
// Evaluation with the averaged weights exchanges the two buffers in place (kml_ema_swap): the
// forward kernels read the bf16 shadow and views of the state buffer, so nothing is re-captured.
#include "kml_common.h"

namespace {

// A value of its own: the build's -ffp-contract=fast would otherwise fuse the product into the
// following add (v_fma_f32), and __fmul_rn / __fadd_rn are plain operators in this toolchain.  Emits
// no instruction.
__device__ __forceinline__ float rounded(float q) {
  asm volatile("" : "+v"(q));
  return q;
}

// e + (w - e) * a, three roundings: torch's e + (w - e) * a in fp32 gives the same bits
__device__ __forceinline__ float ema_elem(float e, float w, float a) {
  const float prod = rounded(__fmul_rn(__fsub_rn(w, e), a));
  return __fadd_rn(e, prod);
}

__device__ __forceinline__ float4 ema_vec4(const float4& E, const float4& W, float a) {
  return make_float4(ema_elem(E.x, W.x, a), ema_elem(E.y, W.y, a), ema_elem(E.z, W.z, a), ema_elem(E.w, W.w, a));
}

__global__ __launch_bounds__(256) void k_ema_update(float* __restrict__ ema, const float* __restrict__ w,
                                                    long long n4, float decay, int every, int warmup,
                                                    int* __restrict__ ctl, float* __restrict__ aout,
                                                    unsigned* __restrict__ ticket) {
  // read before this block's ticket: the last arriver is the only writer of ctl
  const int ticks = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int updates = __hip_atomic_load(ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int apply = ((unsigned)ticks + 1u) % (unsigned)every == 0u;
  float d = decay;
  if (warmup) {
    // timm's warm-up: min(decay, (1 + u) / (10 + u)), the quotient of the two integers as fp32
    const float r = __fdiv_rn((float)(updates + 1), (float)(updates + 10));
    d = r < decay ? r : decay;
  }
  const float a = __fsub_rn(1.f, d);
  if (apply) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    // two float4 groups per thread and iteration, all four loads issued before the math (k_adam's
    // reason: twice the bytes in flight per wave on a 12-byte-per-element stream)
    constexpr int U = 2;
    for (long long i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i0 < n4; i0 += U * stride) {
      float4 E[U], W[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long i = i0 + u * stride;
        if (i < n4) {
          E[u] = reinterpret_cast<const float4*>(ema)[i];
          W[u] = reinterpret_cast<const float4*>(w)[i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long i = i0 + u * stride;
        if (i >= n4) break;
        reinterpret_cast<float4*>(ema)[i] = ema_vec4(E[u], W[u], a);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  __threadfence();
  const unsigned tk = atomicAdd(ticket, 1u);
  if (tk == gridDim.x - 1) {
    ctl[0] = ticks + 1;
    ctl[1] = updates + apply;
    ctl[2] = apply;
    aout[0] = a;
    atomicExch(ticket, 0u);
  }
}

// state <-> ema over n elements; the bf16 shadow of the parameter range follows the new state
__global__ __launch_bounds__(256) void k_ema_swap(float* __restrict__ state, float* __restrict__ ema,
                                                  bf16_t* __restrict__ shadow, long long n4, long long n_params) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 s = reinterpret_cast<const float4*>(state)[i];
    const float4 e = reinterpret_cast<const float4*>(ema)[i];
    reinterpret_cast<float4*>(state)[i] = e;
    reinterpret_cast<float4*>(ema)[i] = s;
    const long long el = i << 2;
    if (shadow && el + 3 < n_params) {
      uint2 p;
      p.x = pack_bf2(e.x, e.y);
      p.y = pack_bf2(e.z, e.w);
      reinterpret_cast<uint2*>(shadow)[i] = p;
    } else if (shadow && el < n_params) {
      const float ev[4] = {e.x, e.y, e.z, e.w};
      for (int k = 0; k < 4; ++k)
        if (el + k < n_params) shadow[el + k] = f2bf(ev[k]);
    }
  }
}

static inline unsigned ema_grid(long long n, int max_blocks) {
  unsigned grid = kml_stream_grid((n + 3) / 4, 256);
  if (max_blocks > 0 && grid > (unsigned)max_blocks) grid = (unsigned)max_blocks;
  return grid;
}

}  // namespace

// ema, w: fp32 [n], n % 4 == 0, 16-byte aligned.  ctl: int32 [4] = [ticks, updates, applied, 0];
// aout: fp32 [1]; ticket: one word, 0 on entry and on exit.  The launch applies
// ema += (w - ema) * (1 - d) iff (ticks + 1) % every == 0, d = warmup ? min(decay, (1 + updates) /
// (10 + updates)) : decay; then ticks += 1, updates += applied.  max_blocks > 0 caps the grid.
KML_API int kml_ema_update(float* ema, const float* w, long long n, float decay, int every, int warmup, int* ctl,
                           float* aout, unsigned* ticket, int max_blocks, hipStream_t s) {
  if (n < 0 || (n & 3) || every < 1 || !ema || !w || !ctl || !aout || !ticket ||
      (((uintptr_t)ema | (uintptr_t)w) & 15))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ema_update, dim3(ema_grid(n, max_blocks)), dim3(256), 0, s, ema, w, n >> 2, decay, every,
                     warmup, ctl, aout, ticket);
  KML_LAUNCH_CHECK();
}

// state[i] <-> ema[i] for i < n (n % 4 == 0, 16-byte aligned); shadow[i] = bf16(new state[i]) for
// i < n_params <= n (shadow may be null).  Two calls restore every bit.
KML_API int kml_ema_swap(float* state, float* ema, bf16_t* shadow, long long n, long long n_params, hipStream_t s) {
  if (n < 0 || (n & 3) || n_params < 0 || n_params > n || !state || !ema ||
      (((uintptr_t)state | (uintptr_t)ema) & 15) || ((uintptr_t)shadow & 7))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ema_swap, dim3(ema_grid(n, 0)), dim3(256), 0, s, state, ema, shadow, n >> 2, n_params);
  KML_LAUNCH_CHECK();
}
