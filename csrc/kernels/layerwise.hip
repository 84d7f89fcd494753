// layerwise.hip — fused LAMB and LARS over the flat parameter buffer (gfx950).
//
// Both optimizers scale each parameter tensor's update by a trust ratio of two 2-norms taken over
// that tensor alone, so a step needs a segmented reduction over the flat space before any element
// of the tensor is updated.  A step is two launches, the kernel boundary being the only grid-wide
// synchronisation (no cooperative launch, no grid barrier, no spin wait):
//
//   launch 1  kml_lamb_moments / kml_lars_norms.  The host cut the space once into chunks: whole
//             64-element granules of ONE tensor, at most KML_LAYER_CHUNK elements, a tensor's chunks
//             consecutive.  A block takes chunks grid-stride, one chunk at a time; thread j of the
//             block visits float4 j, j + 256, ... of the chunk, so the two sums of squares a chunk
//             leaves in part[chunk] are a function of the chunk's values alone.  LAMB also updates
//             and stores the moments here and forms the update direction u in registers.  The last
//             block to arrive (the ticket of k_grad_norm: the counter is back at 0 when the launch
//             ends) folds every tensor's partials in chunk order (a wave's lane j adds a tensor's
//             partials j, j + 64, ... then a butterfly; four tensors per wave in flight) and writes
//             ratio[tensor].
//   launch 2  kml_lamb_apply / kml_lars_apply.  Per chunk: the tensor's ratio and (lr, weight
//             decay), the update, the master and the bf16 shadow.  LAMB recomputes u from the stored
//             m, v, w through lamb_u(), the function launch 1 summed: storing u would cost the same
//             42 bytes per parameter and a numel fp32 scratch buffer.
//
// No float atomics: every result is a function of (layout, values), not of the grid size.  The step
// count, first-step flag, clip coefficient and the per-tensor table hp[T][4] = (lr, weight decay,
// adapt, unused) are read from device memory, so a captured step follows set_lr / reset_state /
// set_max_grad_norm without re-capture.  Padding of a region holds zeros in every buffer and both
// updates map zeros to zeros.
//
// Semantics: LAMB as You et al. 2020 / apex FusedLAMB with decoupled decay and bias correction;
// LARS as You, Gitman, Ginsburg 2017 in the "scale" form of apex LARC around momentum SGD.  A
// NaN norm gives a NaN ratio (never 1), as the clip coefficient does.
#include "kml_common.h"

constexpr int KML_LAYER_CHUNK = 8192;   // elements per chunk at most (ops/kernels.py LAYER_CHUNK)
constexpr int KML_LAYER_MAX_BLOCKS = 2048;    // launch 2: a plain stream, as kml_stream_grid
// Launch 1 pays a release fence and a ticket per block, and tickets on one word serialise: at 2048
// blocks that was 45 - 60 us of the launch (ResNet-34 norms 101 us against 58 us at 512 blocks,
// BERT-base moments 566 against 507 us; profiles/r9/layerwise_optim.md).  Two blocks per CU keep
// the stream at the HBM rate.  The results do not depend on the grid.
constexpr int KML_LAYER_NORM_BLOCKS = 512;

namespace {

// every thread gets the block's two sums (4 waves of 64), in a fixed order; one barrier pair for both
__device__ __forceinline__ void lw_block_sum2(float& a, float& b, float* sh) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = a;
    sh[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

struct Chunk {
  long long start;   // first element
  int len4;          // float4 groups
  int tensor;
  bool ok;
};

// chunk c of the table, checked against the buffers (n elements, T tensors): a row that does not
// lie inside them is skipped, so a damaged table cannot make a launch touch memory outside
__device__ __forceinline__ Chunk load_chunk(const int* __restrict__ chunks, int c, long long n, int T) {
  const int s = chunks[3 * c], l = chunks[3 * c + 1], t = chunks[3 * c + 2];
  Chunk k;
  k.start = s;
  k.len4 = l >> 2;
  k.tensor = t;
  k.ok = s >= 0 && l > 0 && l <= KML_LAYER_CHUNK && (s & 63) == 0 && (l & 63) == 0 && (long long)s + l <= n &&
         t >= 0 && t < T;
  return k;
}

// b^t for the integral step count t (square and multiply, fp64): the bias corrections 1 - b^t
// cancel badly in fp32 (1 - 0.999 carries 24 - 10 bits), and u divides by them
__device__ __forceinline__ double pow_step(double b, float t) {
  double p = 1.0;
  for (unsigned k = (unsigned)fmaxf(t, 0.f); k; k >>= 1) {
    if (k & 1u) p *= b;
    b *= b;
  }
  return p;
}

struct LambCoef {
  float b1, omb1, b2, omb2;   // the betas and one minus them, each rounded once from fp64
  float c1, c2;               // 1 / (1 - b1^t), 1 / sqrt(1 - b2^t)
  float eps;
};

__device__ __forceinline__ LambCoef lamb_coef(double b1, double b2, float eps, const float* step_ptr, float step_host) {
  const float t = step_ptr ? *step_ptr : step_host;
  LambCoef k;
  k.b1 = (float)b1;
  k.omb1 = (float)(1.0 - b1);
  k.b2 = (float)b2;
  k.omb2 = (float)(1.0 - b2);
  k.c1 = (float)(1.0 / (1.0 - pow_step(b1, t)));
  k.c2 = (float)(1.0 / sqrt(1.0 - pow_step(b2, t)));
  k.eps = eps;
  return k;
}

// LAMB's update direction of one element: (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd * w.
// The one definition both launches use; every rounding is spelled out (a product feeding a
// division, two explicit fmas), so -ffp-contract=fast has nothing to choose and launch 2 applies
// the bits launch 1 took the norm of.
__device__ __forceinline__ float lamb_u(float m, float v, float w, float wd, const LambCoef& k) {
  const float q = (m * k.c1) / __builtin_fmaf(sqrtf(v), k.c2, k.eps);
  return __builtin_fmaf(wd, w, q);
}

// The hand-off of launch 1 (k_grad_norm's): thread 0, the only writer of this block's partials,
// drains its stores, releases at agent scope and takes a ticket; the last arriver acquires and
// puts the counter back to 0.  Returns true in every thread of the last block.
__device__ __forceinline__ bool last_block(unsigned* __restrict__ counter, unsigned* sh_last) {
  if (threadIdx.x == 0) {
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
    *sh_last = l;
  }
  __syncthreads();
  return *sh_last != 0u;
}

// The fold of launch 1's last block.  part[c] = (two sums of chunk c) as one 8-byte word; a tensor's
// sums are added in a fixed order that depends on its chunk count alone: lane j of a wave adds the
// partials j, j + 64, j + 128, ... in that order, then the butterfly.  A wave folds FOUR tensors at a
// time (tensors 4 * wave + 16 * round + {0..3}) with all their loads in flight together, and reads
// the next round's table rows before it waits for this round's partials: the fold is bound by
// round trips to the L2 (agent-scope loads, never this CU's L1), not by arithmetic.
// ratio_of(sums.x, sums.y, hp row) runs in lane 0.
struct FoldRow {
  int c0, cnt;
  float4 hp;
};

__device__ __forceinline__ FoldRow fold_row(const int* __restrict__ ranges, const float* __restrict__ hp, int t,
                                            int T, int C) {
  FoldRow r;
  r.c0 = 0;
  r.cnt = 0;
  r.hp = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < T) {
    r.c0 = ranges[2 * t];
    r.cnt = ranges[2 * t + 1];
    r.hp = reinterpret_cast<const float4*>(hp)[t];
    if (r.c0 < 0 || r.cnt < 0 || (long long)r.c0 + r.cnt > C) r.c0 = r.cnt = 0;   // a damaged row reads nothing
  }
  return r;
}

template <class RatioOf>
__device__ __forceinline__ void fold_tensors(const float* __restrict__ part, const int* __restrict__ ranges,
                                             const float* __restrict__ hp, int T, int C, float* __restrict__ ratio,
                                             RatioOf ratio_of) {
  constexpr int Q = 4, U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long* part2 = reinterpret_cast<const unsigned long long*>(part);
  FoldRow next[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) next[q] = fold_row(ranges, hp, Q * wave + q, T, C);
  for (int t0 = Q * wave; t0 < T; t0 += 4 * Q) {
    FoldRow row[Q];
    int most = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      row[q] = next[q];
      most = row[q].cnt > most ? row[q].cnt : most;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) next[q] = fold_row(ranges, hp, t0 + 4 * Q + q, T, C);
    float a[Q] = {0.f, 0.f, 0.f, 0.f}, b[Q] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < most; k0 += 64 * U) {
      unsigned long long v[U][Q];
      // every load is issued (index clamped into the tensor's partials, or to word 0), the ones past
      // a tensor's end are dropped afterwards: a branch per load would wait for each in turn
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int k = k0 + 64 * u + lane;
          const int at = row[q].cnt > 0 ? row[q].c0 + (k < row[q].cnt ? k : row[q].cnt - 1) : 0;
          v[u][q] = __hip_atomic_load(part2 + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const bool in = k0 + 64 * u + lane < row[q].cnt;
          a[q] += in ? __uint_as_float((unsigned)v[u][q]) : 0.f;
          b[q] += in ? __uint_as_float((unsigned)(v[u][q] >> 32)) : 0.f;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float sa = wave_sum(a[q]), sb = wave_sum(b[q]);
      if (lane == 0 && t0 + q < T) ratio[t0 + q] = ratio_of(sa, sb, row[q].hp);
    }
  }
}

__global__ __launch_bounds__(256) void k_lamb_moments(
    const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const int* __restrict__ chunks, int C, const int* __restrict__ ranges, int T, const float* __restrict__ hp,
    const float* __restrict__ step_ptr, float step_host, double b1, double b2, float eps, float grad_scale,
    const float* __restrict__ clip_ptr, float* __restrict__ part, unsigned* __restrict__ counter,
    float* __restrict__ ratio, long long n) {
  __shared__ float sh[8];
  __shared__ unsigned sh_last;
  const int tid = threadIdx.x;
  if (clip_ptr) grad_scale *= *clip_ptr;   // global-norm clipping coefficient (k_grad_norm)
  const LambCoef k = lamb_coef(b1, b2, eps, step_ptr, step_host);
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, n, T);
    float sw = 0.f, su = 0.f;
    if (ch.ok) {
      const float wd = hp[4 * ch.tensor + 1];
      const long long base = ch.start >> 2;
      // two float4 groups per iteration, all eight loads issued before the math (k_adam's unroll)
      constexpr int U = 2;
      for (int i0 = tid; i0 < ch.len4; i0 += U * 256) {
        float4 W[U], G[U], M[U], V[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * 256;
          if (i < ch.len4) {
            W[u] = reinterpret_cast<const float4*>(w)[base + i];
            G[u] = reinterpret_cast<const float4*>(g)[base + i];
            M[u] = reinterpret_cast<const float4*>(m)[base + i];
            V[u] = reinterpret_cast<const float4*>(v)[base + i];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * 256;
          if (i >= ch.len4) break;
          const float wv[4] = {W[u].x, W[u].y, W[u].z, W[u].w}, gv[4] = {G[u].x, G[u].y, G[u].z, G[u].w};
          float mv[4] = {M[u].x, M[u].y, M[u].z, M[u].w}, vv[4] = {V[u].x, V[u].y, V[u].z, V[u].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float gg = gv[e] * grad_scale;
            mv[e] = __builtin_fmaf(k.b1, mv[e], k.omb1 * gg);
            vv[e] = __builtin_fmaf(k.b2, vv[e], k.omb2 * gg * gg);
            const float uu = lamb_u(mv[e], vv[e], wv[e], wd, k);
            sw = __builtin_fmaf(wv[e], wv[e], sw);
            su = __builtin_fmaf(uu, uu, su);
          }
          reinterpret_cast<float4*>(m)[base + i] = make_float4(mv[0], mv[1], mv[2], mv[3]);
          reinterpret_cast<float4*>(v)[base + i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
      }
    }
    lw_block_sum2(sw, su, sh);
    if (tid == 0) reinterpret_cast<float2*>(part)[c] = make_float2(sw, su);
  }
  if (!last_block(counter, &sh_last)) return;
  fold_tensors(part, ranges, hp, T, C, ratio, [](float sw, float su, const float4& h) {
    const float wn = sqrtf(sw), un = sqrtf(su);
    float r = 1.f;
    if (h.z != 0.f) {   // adapt
      if (wn > 0.f && un > 0.f) r = wn / un;
      else if (wn != wn || un != un) r = wn + un;   // NaN reaches the weights
    }
    return r;
  });
}

__global__ __launch_bounds__(256) void k_lamb_apply(
    float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v, bf16_t* __restrict__ shadow,
    const int* __restrict__ chunks, int C, int T, const float* __restrict__ hp, const float* __restrict__ ratio,
    const float* __restrict__ step_ptr, float step_host, double b1, double b2, float eps, long long n) {
  const int tid = threadIdx.x;
  const LambCoef k = lamb_coef(b1, b2, eps, step_ptr, step_host);
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, n, T);
    if (!ch.ok) continue;
    const float wd = hp[4 * ch.tensor + 1];
    const float nstep = -(hp[4 * ch.tensor] * ratio[ch.tensor]);   // -lr * r
    const long long base = ch.start >> 2;
    constexpr int U = 2;
    for (int i0 = tid; i0 < ch.len4; i0 += U * 256) {
      float4 W[U], M[U], V[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        if (i < ch.len4) {
          W[u] = reinterpret_cast<const float4*>(w)[base + i];
          M[u] = reinterpret_cast<const float4*>(m)[base + i];
          V[u] = reinterpret_cast<const float4*>(v)[base + i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        if (i >= ch.len4) break;
        float wv[4] = {W[u].x, W[u].y, W[u].z, W[u].w};
        const float mv[4] = {M[u].x, M[u].y, M[u].z, M[u].w}, vv[4] = {V[u].x, V[u].y, V[u].z, V[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[e] = __builtin_fmaf(nstep, lamb_u(mv[e], vv[e], wv[e], wd, k), wv[e]);
        reinterpret_cast<float4*>(w)[base + i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
        if (shadow) {
          uint2 s;
          s.x = pack_bf2(wv[0], wv[1]);
          s.y = pack_bf2(wv[2], wv[3]);
          reinterpret_cast<uint2*>(shadow)[base + i] = s;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_lars_norms(
    const float* __restrict__ w, const float* __restrict__ g, const int* __restrict__ chunks, int C,
    const int* __restrict__ ranges, int T, const float* __restrict__ hp, float trust, float eps, float grad_scale,
    const float* __restrict__ clip_ptr, float* __restrict__ part, unsigned* __restrict__ counter,
    float* __restrict__ ratio, long long n) {
  __shared__ float sh[8];
  __shared__ unsigned sh_last;
  const int tid = threadIdx.x;
  if (clip_ptr) grad_scale *= *clip_ptr;
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, n, T);
    float sw = 0.f, sg = 0.f;
    if (ch.ok) {
      const long long base = ch.start >> 2;
      // a read-only stream: four float4 groups of each buffer in flight (k_grad_norm's unroll)
      constexpr int U = 4;
      for (int i0 = tid; i0 < ch.len4; i0 += U * 256) {
        float4 W[U], G[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * 256;
          if (i < ch.len4) {
            W[u] = reinterpret_cast<const float4*>(w)[base + i];
            G[u] = reinterpret_cast<const float4*>(g)[base + i];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (i0 + u * 256 >= ch.len4) break;
          const float wv[4] = {W[u].x, W[u].y, W[u].z, W[u].w}, gv[4] = {G[u].x, G[u].y, G[u].z, G[u].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float gg = gv[e] * grad_scale;
            sw = __builtin_fmaf(wv[e], wv[e], sw);
            sg = __builtin_fmaf(gg, gg, sg);
          }
        }
      }
    }
    lw_block_sum2(sw, sg, sh);
    if (tid == 0) reinterpret_cast<float2*>(part)[c] = make_float2(sw, sg);
  }
  if (!last_block(counter, &sh_last)) return;
  fold_tensors(part, ranges, hp, T, C, ratio, [trust, eps](float sw, float sg, const float4& h) {
    const float wn = sqrtf(sw), gn = sqrtf(sg);
    float r = 1.f;
    if (h.z != 0.f) {   // adapt; h.y is the tensor's weight decay
      if (wn > 0.f && gn > 0.f) r = trust * wn / (__builtin_fmaf(h.y, wn, gn) + eps);
      else if (wn != wn || gn != gn) r = wn + gn;   // NaN reaches the weights
    }
    return r;
  });
}

__global__ __launch_bounds__(256) void k_lars_apply(
    float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom, bf16_t* __restrict__ shadow,
    const int* __restrict__ chunks, int C, int T, const float* __restrict__ hp, const float* __restrict__ ratio,
    float momentum, float dampening, int nesterov, const float* __restrict__ first_ptr, int first_host,
    float grad_scale, const float* __restrict__ clip_ptr, long long n) {
  const int tid = threadIdx.x;
  if (clip_ptr) grad_scale *= *clip_ptr;
  const int first = first_ptr ? (*first_ptr != 0.f) : first_host;
  const bool has_mom = mom != nullptr && momentum != 0.f;
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, n, T);
    if (!ch.ok) continue;
    const float lr = hp[4 * ch.tensor], wd = hp[4 * ch.tensor + 1];
    const float r = ratio[ch.tensor];
    const long long base = ch.start >> 2;
    constexpr int U = 2;
    for (int i0 = tid; i0 < ch.len4; i0 += U * 256) {
      float4 W[U], G[U], M[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        if (i < ch.len4) {
          W[u] = reinterpret_cast<const float4*>(w)[base + i];
          G[u] = reinterpret_cast<const float4*>(g)[base + i];
          if (has_mom) M[u] = reinterpret_cast<const float4*>(mom)[base + i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        if (i >= ch.len4) break;
        float wv[4] = {W[u].x, W[u].y, W[u].z, W[u].w};
        const float gv[4] = {G[u].x, G[u].y, G[u].z, G[u].w};
        float mv[4] = {0.f, 0.f, 0.f, 0.f};
        if (has_mom) { mv[0] = M[u].x; mv[1] = M[u].y; mv[2] = M[u].z; mv[3] = M[u].w; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float d = r * __builtin_fmaf(wd, wv[e], gv[e] * grad_scale);
          if (has_mom) {
            mv[e] = first ? d : __builtin_fmaf(momentum, mv[e], (1.f - dampening) * d);
            d = nesterov ? __builtin_fmaf(momentum, mv[e], d) : mv[e];
          }
          wv[e] = __builtin_fmaf(-lr, d, wv[e]);
        }
        reinterpret_cast<float4*>(w)[base + i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
        if (has_mom) reinterpret_cast<float4*>(mom)[base + i] = make_float4(mv[0], mv[1], mv[2], mv[3]);
        if (shadow) {
          uint2 s;
          s.x = pack_bf2(wv[0], wv[1]);
          s.y = pack_bf2(wv[2], wv[3]);
          reinterpret_cast<uint2*>(shadow)[base + i] = s;
        }
      }
    }
  }
}

}  // namespace

// blocks of a layer-wise launch: one chunk per block and round, at most `cap`
static inline unsigned kml_layer_grid(int C, int max_blocks, int cap = KML_LAYER_MAX_BLOCKS) {
  int g = C < cap ? C : cap;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return (unsigned)(g < 1 ? 1 : g);
}

// what every layer-wise launch needs: whole granules (n % 64 == 0, below 2^31: the chunk table is
// int32), the tables (hp rows are read as float4), and 16-byte aligned buffers (a null optional
// buffer passes)
static inline bool kml_layer_ok(long long n, int C, int T, const void* chunks, const void* hp, const void* ratio,
                                const void* a, const void* b, const void* c, const void* d, const void* e) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e;
  return n >= 0 && n < (1LL << 31) && (n & 63) == 0 && C >= 1 && T >= 1 && chunks && hp && ratio && a && b &&
         ((bits | (uintptr_t)hp) & 15) == 0;
}

// LAMB, launch 1.  chunks: int32 [C][3] (start, length, tensor); ranges: int32 [T][2] (first chunk,
// chunks) of each tensor; hp: fp32 [T][4] (lr, weight decay, adapt, unused); part: 2 * C floats of
// scratch, 8-byte aligned; counter: one word, 0 on entry and on exit; ratio: T floats (the trust ratios).  step_ptr
// (or step) is the step count t >= 1 of this step; clip_ptr as kml_adam's.
KML_API int kml_lamb_moments(const float* w, const float* g, float* m, float* v, const int* chunks, int C,
                             const int* ranges, int T, const float* hp, const float* step_ptr, float step, double b1,
                             double b2, float eps, float grad_scale, const float* clip_ptr, float* part,
                             unsigned* counter, float* ratio, long long n, int max_blocks, hipStream_t s) {
  if (!m || !v || !ranges || !part || ((uintptr_t)part & 7) || !counter ||
      !kml_layer_ok(n, C, T, chunks, hp, ratio, w, g, m, v, nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lamb_moments, dim3(kml_layer_grid(C, max_blocks, KML_LAYER_NORM_BLOCKS)), dim3(256), 0, s, w, g,
                     m, v, chunks, C, ranges, T, hp, step_ptr, step, b1, b2, eps, grad_scale, clip_ptr, part, counter,
                     ratio, n);
  KML_LAUNCH_CHECK();
}

// LAMB, launch 2: w -= lr * ratio * u with u recomputed from (m, v, w); the bf16 shadow refreshed
KML_API int kml_lamb_apply(float* w, const float* m, const float* v, bf16_t* shadow, const int* chunks, int C, int T,
                           const float* hp, const float* ratio, const float* step_ptr, float step, double b1, double b2,
                           float eps, long long n, int max_blocks, hipStream_t s) {
  if (!v || !kml_layer_ok(n, C, T, chunks, hp, ratio, w, m, v, shadow, nullptr)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lamb_apply, dim3(kml_layer_grid(C, max_blocks)), dim3(256), 0, s, w, m, v, shadow, chunks, C, T,
                     hp, ratio, step_ptr, step, b1, b2, eps, n);
  KML_LAUNCH_CHECK();
}

// LARS, launch 1: ratio[t] = trust * |w_t| / (|g'_t| + wd_t * |w_t| + eps); tables as kml_lamb_moments
KML_API int kml_lars_norms(const float* w, const float* g, const int* chunks, int C, const int* ranges, int T,
                           const float* hp, float trust, float eps, float grad_scale, const float* clip_ptr,
                           float* part, unsigned* counter, float* ratio, long long n, int max_blocks, hipStream_t s) {
  if (!ranges || !part || ((uintptr_t)part & 7) || !counter ||
      !kml_layer_ok(n, C, T, chunks, hp, ratio, w, g, nullptr, nullptr, nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lars_norms, dim3(kml_layer_grid(C, max_blocks, KML_LAYER_NORM_BLOCKS)), dim3(256), 0, s, w, g,
                     chunks, C, ranges, T, hp, trust, eps, grad_scale, clip_ptr, part, counter, ratio, n);
  KML_LAUNCH_CHECK();
}

// LARS, launch 2: momentum SGD on d = ratio * (g' + wd * w); mom may be null when momentum == 0
KML_API int kml_lars_apply(float* w, const float* g, float* mom, bf16_t* shadow, const int* chunks, int C, int T,
                           const float* hp, const float* ratio, float momentum, float dampening, int nesterov,
                           const float* first_ptr, int first, float grad_scale, const float* clip_ptr, long long n,
                           int max_blocks, hipStream_t s) {
  if ((momentum != 0.f && !mom) || !kml_layer_ok(n, C, T, chunks, hp, ratio, w, g, mom, shadow, nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lars_apply, dim3(kml_layer_grid(C, max_blocks)), dim3(256), 0, s, w, g, mom, shadow, chunks, C,
                     T, hp, ratio, momentum, dampening, nesterov, first_ptr, first, grad_scale, clip_ptr, n);
  KML_LAUNCH_CHECK();
}
