// llama.hip — the non-GEMM, non-attention ops of a Llama-style decoder block for gfx950:
//   RMSNorm fwd (+ fused residual add, the pre-norm stream carried in the launch) / bwd
//     (dgamma: ordered per-block partial rows, folded in block order by the last block to arrive),
//   rotary position embedding (HF rotate_half convention) in place on the fused QKV buffer,
//     forward and transpose (backward) rotation from one entry,
//   SwiGLU h = silu(gate) * up on the fused gate/up GEMM output, fwd / bwd.
// All arithmetic in fp32 from the bf16 loads, one rounding to bf16 at each store.  The grouped-
// query attention that completes the block is in attention.hip.
#include "kml_common.h"

namespace {

constexpr int MAXV = 8;   // RMSNorm: up to 8 x (64 lanes x 4) = 2048 columns held in registers

__device__ __forceinline__ void unpack4(const uint2 v, float* f) {
  f[0] = lo_bf(v.x); f[1] = hi_bf(v.x); f[2] = lo_bf(v.y); f[3] = hi_bf(v.y);
}
__device__ __forceinline__ uint2 pack4(const float* f) {
  uint2 v;
  v.x = pack_bf2(f[0], f[1]);
  v.y = pack_bf2(f[2], f[3]);
  return v;
}
__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
  f[0] = lo_bf(v.x); f[1] = hi_bf(v.x); f[2] = lo_bf(v.y); f[3] = hi_bf(v.y);
  f[4] = lo_bf(v.z); f[5] = hi_bf(v.z); f[6] = lo_bf(v.w); f[7] = hi_bf(v.w);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 v;
  v.x = pack_bf2(f[0], f[1]); v.y = pack_bf2(f[2], f[3]);
  v.z = pack_bf2(f[4], f[5]); v.w = pack_bf2(f[6], f[7]);
  return v;
}

// ------------------------------------------------------------------------------ RMSNorm fwd
// s = x (+ res); rstd = rsqrt(mean(s^2) + eps); y = s * rstd * gamma; sum_out (optional) = s.
// One wave per row, four rows per block; the row stays in NV = ceil(N / 256) register vectors
// between the reduction and the apply: one HBM read and one write per element.
template <int NV>
__global__ __launch_bounds__(256) void k_rmsnorm_fwd(const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                     const float* __restrict__ gamma, bf16_t* __restrict__ y,
                                                     bf16_t* __restrict__ sum_out, float* __restrict__ rstd,
                                                     long long M, int N, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  uint2 xv[NV], rv[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) {   // all loads first
    const int c = (u * 64 + lane) * 4;
    if (c < N) {
      xv[u] = *reinterpret_cast<const uint2*>(x + row * N + c);
      if (res) rv[u] = *reinterpret_cast<const uint2*>(res + row * N + c);
    }
  }
  float v[NV][4];
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = (u * 64 + lane) * 4;
    if (c < N) {
      unpack4(xv[u], v[u]);
      if (res) {
        float r[4];
        unpack4(rv[u], r);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[u][k] += r[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) q += v[u][k] * v[u][k];
    }
  }
  q = wave_sum(q);
  const float rs = rsqrtf(q / N + eps);
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = (u * 64 + lane) * 4;
    if (c < N) {
      if (sum_out) *reinterpret_cast<uint2*>(sum_out + row * N + c) = pack4(v[u]);
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = v[u][k] * rs * gamma[c + k];
      *reinterpret_cast<uint2*>(y + row * N + c) = pack4(o);
    }
  }
  if (lane == 0) rstd[row] = rs;
}

// ------------------------------------------------------------------------------ RMSNorm bwd
// sh = s * rstd; dx = rstd * (gamma dy - sh * mean(gamma dy sh)) (+ dx_add, the stream gradient).
// A block owns rows_per_block rows, one wave per row with the wave's next row (row + 4) in
// flight while this one is reduced and stored.  dgamma: every wave sums dy * sh over its rows in
// registers; the four waves meet in LDS and the block publishes ONE partial row of N floats
// (write-through).  The last block to take the ticket sums the partial rows in block order and
// adds them to dgamma: no float atomics, the same bits every run.
template <int NV>
__global__ __launch_bounds__(256) void k_rmsnorm_bwd(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ sin_,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     bf16_t* __restrict__ dx, const bf16_t* __restrict__ dx_add,
                                                     float* __restrict__ dgamma, float* __restrict__ part,
                                                     unsigned* __restrict__ ticket, long long M, int N,
                                                     int rows_per_block) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float pg[NV][4], gm[NV][4];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = (u * 64 + lane) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pg[u][k] = 0.f;
      gm[u][k] = c < N ? gamma[c + k] : 0.f;
    }
  }
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min(M, r0 + rows_per_block);
  uint2 dv[NV], sv[NV], av[NV];
  float rs = 0.f;
  auto load = [&](long long row) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int c = (u * 64 + lane) * 4;
      if (c < N) {
        dv[u] = *reinterpret_cast<const uint2*>(dy + row * N + c);
        sv[u] = *reinterpret_cast<const uint2*>(sin_ + row * N + c);
        if (dx_add) av[u] = *reinterpret_cast<const uint2*>(dx_add + row * N + c);
      }
    }
    rs = rstd[row];
  };
  long long row = r0 + wv;
  if (row < r1) load(row);
  for (; row < r1; row += 4) {
    uint2 d_cur[NV], s_cur[NV], a_cur[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) { d_cur[u] = dv[u]; s_cur[u] = sv[u]; a_cur[u] = av[u]; }
    const float rs_c = rs;
    if (row + 4 < r1) load(row + 4);   // next row of this wave, in flight during this one
    float sh[NV][4], gd[NV][4];
    float a2 = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int c = (u * 64 + lane) * 4;
      if (c < N) {
        float d[4], sf[4];
        unpack4(d_cur[u], d);
        unpack4(s_cur[u], sf);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          sh[u][k] = sf[k] * rs_c;
          gd[u][k] = d[k] * gm[u][k];
          a2 += gd[u][k] * sh[u][k];
          pg[u][k] += d[k] * sh[u][k];
        }
      }
    }
    a2 = wave_sum(a2) / N;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int c = (u * 64 + lane) * 4;
      if (c < N) {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = rs_c * (gd[u][k] - sh[u][k] * a2);
        if (dx_add) {
          float e[4];
          unpack4(a_cur[u], e);
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] += e[k];
        }
        *reinterpret_cast<uint2*>(dx + row * N + c) = pack4(o);
      }
    }
  }
  // the block's partial row: the four waves in LDS, summed in wave order
  __shared__ float red[4][64 * 4 * MAXV];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = (u * 64 + lane) * 4;
    if (c < N)
#pragma unroll
      for (int k = 0; k < 4; ++k) red[wv][c + k] = pg[u][k];
  }
  __syncthreads();
  float* mine = part + (long long)blockIdx.x * N;
  for (int c = threadIdx.x; c < N; c += 256)
    __hip_atomic_store(mine + c, (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  // published write-through; drain, one ticket per block, the last block folds (loss.hip's scheme)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __shared__ unsigned last;
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == gridDim.x - 1) ? 1u : 0u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // graph-replay safe
    }
  }
  __syncthreads();
  if (!last) return;
  const int G = (int)gridDim.x;
  for (int j = threadIdx.x; j < N / 4; j += 256) {   // one float4 column group per thread, 8 rows in flight
    const float4* col = reinterpret_cast<const float4*>(part) + j;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g0 = 0; g0 < G; g0 += 8) {
      float4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v[k] = g0 + k < G ? col[(long long)(g0 + k) * (N / 4)] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < 8; ++k) { t.x += v[k].x; t.y += v[k].y; t.z += v[k].z; t.w += v[k].w; }
    }
    float* o = dgamma + 4 * j;   // a slice of the flat gradient buffer: no alignment assumed
    o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
  }
}

int rms_bwd_blocks(long long M, int* rpb) {
  long long r = 16;
  long long g = (M + r - 1) / r;
  if (g > 512) { r = (M + 511) / 512; g = (M + r - 1) / r; }
  *rpb = (int)r;
  return (int)g;
}

// ------------------------------------------------------------------------------ rotary embedding
// In place on the fused projection buffer [T, ld]: columns [0, (H + Hkv) 64) are the H query and
// Hkv key heads (V, behind them, is never touched).  HF rotate_half: element i < 32 of a head
// pairs with i + 32; (a, b) -> (a c - b s, b c + a s), c / s = cos / sin(pos theta^(-i/32)) read
// from the fp32 table [max_pos][cos(32) | sin(32)]; pos = row % L.  Backward: s -> -s, the
// transpose rotation, on dQ / dK.  A thread owns 8 pairs: 16 bytes from each half of a head.
// HALF: half the head width — 32 as described, or 64 for head dim 128 (pairs i and i + 64, table
// rows cos(64) | sin(64), f_i = theta^(-i/64)).
template <int HALF>
__global__ __launch_bounds__(256) void k_rope(bf16_t* __restrict__ qkv, int ld, const float* __restrict__ table,
                                              long long T, int L, int heads, float sgn) {
  constexpr int CH = HALF / 8;   // 8-pair chunks of a head
  const long long n = T * heads * CH;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % CH);
    const long long rh = i / CH;
    const long long row = rh / heads;
    const int head = (int)(rh - row * heads);
    const int pos = (int)(row % L);
    bf16_t* p = qkv + row * ld + head * (2 * HALF) + c * 8;
    const float* tb = table + (long long)pos * (2 * HALF) + c * 8;
    const uint4 lo = *reinterpret_cast<const uint4*>(p);
    const uint4 hi = *reinterpret_cast<const uint4*>(p + HALF);
    const float4 c0 = *reinterpret_cast<const float4*>(tb), c1 = *reinterpret_cast<const float4*>(tb + 4);
    const float4 s0 = *reinterpret_cast<const float4*>(tb + HALF), s1 = *reinterpret_cast<const float4*>(tb + HALF + 4);
    const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    float a[8], b[8], oa[8], ob[8];
    unpack8(lo, a);
    unpack8(hi, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) kml_rope_pair(a[k], b[k], cs[k], sn[k] * sgn, oa[k], ob[k]);
    *reinterpret_cast<uint4*>(p) = pack8(oa);
    *reinterpret_cast<uint4*>(p + HALF) = pack8(ob);
  }
}

// ------------------------------------------------------------------------------ SwiGLU
// (sigmoidf_fast: kml_common.h, shared with the decode step's gated GEMM)
// gu [T, ldg]: gate in columns [0, I), up in [I, 2I); h [T, I] = silu(gate) * up
__global__ __launch_bounds__(256) void k_swiglu_fwd(const bf16_t* __restrict__ gu, int ldg, bf16_t* __restrict__ h,
                                                    long long T, int I) {
  const int I8 = I / 8;
  const long long n = T * I8;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long row = i / I8;
    const int c = (int)(i - row * I8) * 8;
    float g[8], u[8], o[8];
    unpack8(*reinterpret_cast<const uint4*>(gu + row * ldg + c), g);
    unpack8(*reinterpret_cast<const uint4*>(gu + row * ldg + I + c), u);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = g[k] * sigmoidf_fast(g[k]) * u[k];
    *reinterpret_cast<uint4*>(h + row * I + c) = pack8(o);
  }
}

// dgu = [dh u sig(g) (1 + g (1 - sig(g))) | dh silu(g)] from dh [T, I] and the saved gu
__global__ __launch_bounds__(256) void k_swiglu_bwd(const bf16_t* __restrict__ dh, const bf16_t* __restrict__ gu,
                                                    int ldg, bf16_t* __restrict__ dgu, long long T, int I) {
  const int I8 = I / 8;
  const long long n = T * I8;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long row = i / I8;
    const int c = (int)(i - row * I8) * 8;
    float d[8], g[8], u[8], og[8], ou[8];
    unpack8(*reinterpret_cast<const uint4*>(dh + row * I + c), d);
    unpack8(*reinterpret_cast<const uint4*>(gu + row * ldg + c), g);
    unpack8(*reinterpret_cast<const uint4*>(gu + row * ldg + I + c), u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float sg = sigmoidf_fast(g[k]);
      og[k] = d[k] * u[k] * sg * fmaf(g[k], 1.f - sg, 1.f);
      ou[k] = d[k] * g[k] * sg;
    }
    *reinterpret_cast<uint4*>(dgu + row * ldg + c) = pack8(og);
    *reinterpret_cast<uint4*>(dgu + row * ldg + I + c) = pack8(ou);
  }
}

bool al16(const void* p) { return (((unsigned long long)p) & 15ull) == 0; }

template <int HALF>
int rope_launch(bf16_t* qkv, int ld, const float* table, long long T, int L, int H, int Hkv, int max_pos,
                int backward, hipStream_t s) {
  if (T <= 0 || L <= 0 || T % L || L > max_pos || H <= 0 || Hkv <= 0 || ld % 8 ||
      ld < (H + 2 * Hkv) * 2 * HALF || !al16(qkv) || !al16(table))
    return (int)hipErrorInvalidValue;
  const int heads = H + Hkv;
  hipLaunchKernelGGL(k_rope<HALF>, dim3(kml_stream_grid(T * heads * (HALF / 8), 256)), dim3(256), 0, s, qkv, ld,
                     table, T, L, heads, backward ? -1.f : 1.f);
  KML_LAUNCH_CHECK();
}

}  // namespace

// y = RMSNorm(x [+ res]) * gamma over rows of N bf16; sum_out (optional) = x + res; rstd fp32 [M]
KML_API int kml_rmsnorm_fwd(const bf16_t* x, const bf16_t* res, const float* gamma, bf16_t* y, bf16_t* sum_out,
                            float* rstd, long long M, int N, float eps, hipStream_t s) {
  if (M <= 0 || N <= 0 || N % 4 || N > 64 * 4 * MAXV) return (int)hipErrorInvalidValue;
  const int nv = (N + 255) / 256;
#define KML_RMSF(NVv)                                                                                         \
  if (nv == NVv)                                                                                              \
    hipLaunchKernelGGL(k_rmsnorm_fwd<NVv>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, res, gamma, y, \
                       sum_out, rstd, M, N, eps);
  KML_RMSF(1) KML_RMSF(2) KML_RMSF(3) KML_RMSF(4) KML_RMSF(5) KML_RMSF(6) KML_RMSF(7) KML_RMSF(8)
#undef KML_RMSF
  KML_LAUNCH_CHECK();
}

// workspace floats of kml_rmsnorm_bwd: one partial row of N floats per block
KML_API long long kml_rmsnorm_bwd_ws_floats(long long M, int N) {
  int rpb;
  return (long long)rms_bwd_blocks(M, &rpb) * N;
}

// dx = RMSNorm backward (+ dx_add); dgamma += the column sums of dy * s * rstd.  ws: the
// workspace above; ticket: a zeroed device counter (the kernel resets it).
KML_API int kml_rmsnorm_bwd(const bf16_t* dy, const bf16_t* sin_, const float* rstd, const float* gamma, bf16_t* dx,
                            const bf16_t* dx_add, float* dgamma, float* ws, unsigned* ticket, long long M, int N,
                            hipStream_t s) {
  if (M <= 0 || N <= 0 || N % 4 || N > 64 * 4 * MAXV || !ws || !ticket || !al16(ws))
    return (int)hipErrorInvalidValue;
  int rpb;
  const int g = rms_bwd_blocks(M, &rpb);
  const int nv = (N + 255) / 256;
#define KML_RMSB(NVv)                                                                                          \
  if (nv == NVv)                                                                                               \
    hipLaunchKernelGGL(k_rmsnorm_bwd<NVv>, dim3(g), dim3(256), 0, s, dy, sin_, rstd, gamma, dx, dx_add, dgamma, \
                       ws, ticket, M, N, rpb);
  KML_RMSB(1) KML_RMSB(2) KML_RMSB(3) KML_RMSB(4) KML_RMSB(5) KML_RMSB(6) KML_RMSB(7) KML_RMSB(8)
#undef KML_RMSB
  KML_LAUNCH_CHECK();
}

// rotary embedding in place on qkv [T, ld] (H query heads, then Hkv key heads, then V); table:
// fp32 [max_pos][64] = cos(32) | sin(32); backward != 0: the transpose rotation (for dQ / dK)
KML_API int kml_rope(bf16_t* qkv, int ld, const float* table, long long T, int L, int H, int Hkv, int max_pos,
                     int backward, hipStream_t s) {
  return rope_launch<32>(qkv, ld, table, T, L, H, Hkv, max_pos, backward, s);
}

// the same on heads of 128 columns: pairs i and i + 64, table fp32 [max_pos][128] = cos(64) | sin(64)
KML_API int kml_rope128(bf16_t* qkv, int ld, const float* table, long long T, int L, int H, int Hkv, int max_pos,
                        int backward, hipStream_t s) {
  return rope_launch<64>(qkv, ld, table, T, L, H, Hkv, max_pos, backward, s);
}

// h [T, I] = silu(gu[:, :I]) * gu[:, I:2I]; gu rows ldg apart
KML_API int kml_swiglu_fwd(const bf16_t* gu, int ldg, bf16_t* h, long long T, int I, hipStream_t s) {
  if (T <= 0 || I <= 0 || I % 8 || ldg % 8 || ldg < 2 * I || !al16(gu) || !al16(h)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_swiglu_fwd, dim3(kml_stream_grid(T * (I / 8), 256)), dim3(256), 0, s, gu, ldg, h, T, I);
  KML_LAUNCH_CHECK();
}

// dgu [T, ldg] (both halves) from dh [T, I] and the forward's gu
KML_API int kml_swiglu_bwd(const bf16_t* dh, const bf16_t* gu, int ldg, bf16_t* dgu, long long T, int I,
                           hipStream_t s) {
  if (T <= 0 || I <= 0 || I % 8 || ldg % 8 || ldg < 2 * I || !al16(dh) || !al16(gu) || !al16(dgu))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_swiglu_bwd, dim3(kml_stream_grid(T * (I / 8), 256)), dim3(256), 0, s, dh, gu, ldg, dgu, T, I);
  KML_LAUNCH_CHECK();
}
