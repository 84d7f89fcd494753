// decode.hip — one-token-at-a-time inference for the decoder LMs (models/gpt.py) on gfx950:
//   kml_kv_append       K / V columns of a token-major fused QKV buffer -> head-major cache
//   kml_attn_decode     one query per (sequence, head) against the cached keys, split over the key
//                       range in chunks of a FIXED number of keys; the last block of a (b, h) to
//                       finish folds the chunk partials in chunk order
//   kml_gemm_skinny     y[M <= 16][N] = act(x · wᵀ + bias): every weight byte read once, the 16 x rows
//                       are the second MFMA operand, K split over waves and blocks, folded in order
//   kml_embed2_at       word[ids[b]] + pos[lens[b]]
//   kml_decode_advance  greedy / Gumbel-max token choice, eos bookkeeping, lens and step advance
//   kml_decode_sample   the same choice after a repetition penalty, top-k and top-p (nucleus)
//                       filtering of the row, every parameter read from device memory
//   speculative decoding, k draft tokens verified per round (Q = k + 1 rows a sequence):
//   kml_embed2_multi / kml_attn_decode_multi   the rows at positions lens[b] .. lens[b] + k, each
//                       bit-identical to the one-row kernels at that length
//   kml_draft_lookup    n-gram (prompt lookup) drafter over a sequence's own history
//   kml_verify_pick     the pick of every row, then accept / commit on the device
// Sequence lengths, the sampling temperature, seed, step and eos live in device memory, so one
// captured step replays for every token.  No float atomics anywhere: every reduction has a fixed
// order (lane butterflies, wave order in LDS, chunk / split order in the fold).
#include "kml_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// the counter hash of transformer.hip's dropout (same mixing)
__device__ __forceinline__ unsigned hash3(unsigned a, unsigned b, unsigned c) {
  unsigned h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ c * 0xC2B2AE3Du;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return h;
}

// Hand-off of partials to the last block of a group without fences (conv_igemm.hip's
// group_reduce_rows): partials are stored write-through (st_part), every storing wave drains
// before the barrier, one lane takes a relaxed agent-scope ticket, and the last of `expected`
// blocks reads them with agent-scope loads (ld_part: past its L1 and any stale L2 line) and puts
// the counter back to 0.  A release fence per block would write back its XCD's whole dirty L2.
// Returns true in every thread of that last block.
__device__ __forceinline__ void st_part(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_part(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool last_block(unsigned* __restrict__ counter, unsigned expected, unsigned* sh_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned l = (t == expected - 1u) ? 1u : 0u;
    if (l) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *sh_last = l;
  }
  __syncthreads();
  return *sh_last != 0u;
}

__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
  f[0] = lo_bf(v.x); f[1] = hi_bf(v.x); f[2] = lo_bf(v.y); f[3] = hi_bf(v.y);
  f[4] = lo_bf(v.z); f[5] = hi_bf(v.z); f[6] = lo_bf(v.w); f[7] = hi_bf(v.w);
}

// ------------------------------------------------------------------------------------ KV append
// One thread per 16 bytes: (token row, head, K | V, 8 columns).  Prefill: row t of sequence b goes
// to cache row t; decode: to cache row lens[b] + t (Lq = 1 in a plain step, the rows of a verify
// round otherwise).  Rows outside [0, Lcap) are dropped.
__global__ __launch_bounds__(256) void k_kv_append(const bf16_t* __restrict__ qkv, int ldq, bf16_t* __restrict__ kc,
                                                   bf16_t* __restrict__ vc, const int* __restrict__ lens, int B, int H,
                                                   int Lq, int Lcap, int decode) {
  const long long total = (long long)B * Lq * H * 16;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c8 = (int)(i & 7), isv = (int)((i >> 3) & 1);
  const long long rh = i >> 4;
  const int h = (int)(rh % H);
  const long long tr = rh / H;           // token row b * Lq + t
  const int b = (int)(tr / Lq), t = (int)(tr % Lq);
  const int row = decode ? lens[b] + t : t;
  if (row < 0 || row >= Lcap) return;
  const uint4 v = *reinterpret_cast<const uint4*>(qkv + tr * ldq + (long long)(1 + isv) * H * 64 + h * 64 + c8 * 8);
  bf16_t* dst = (isv ? vc : kc) + (((long long)b * H + h) * Lcap + row) * 64 + c8 * 8;
  *reinterpret_cast<uint4*>(dst) = v;
}

// ------------------------------------------------------------------------------ decode attention
// grid (ceil(Lcap / C), B * H), 256 threads.  Block (ch, bh) owns keys ch*C .. ch*C + C - 1 of one
// 128-byte-row key stream: lane = (key lane>>3, 16-byte column group lane&7), wave w and round i
// take key ch*C + 32 i + 8 w + (lane>>3).  Keys past lens[b] are never loaded: their score is
// -inf and their probability 0 by selection.  Partial per chunk: (max, sum, o[64]) in the exp2
// domain; the last block of the (b, h) folds chunks 0 .. lens[b] / C in that order.
constexpr int ATTN_WS = 66;   // floats per (b, h, chunk)

template <int C>
__global__ __launch_bounds__(256) void k_attn_decode(const bf16_t* __restrict__ q, int ldq,
                                                     const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                                                     const int* __restrict__ lens, float* __restrict__ ws,
                                                     unsigned* __restrict__ cnt, bf16_t* __restrict__ out, int ldo,
                                                     int H, int Lcap, float scale) {
  constexpr int R = C / 32;
  __shared__ float sm[4], ss[4], so[4][64];
  __shared__ unsigned sh_last;
  const int ch = blockIdx.x, bh = blockIdx.y, nch = gridDim.x;
  const int b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int len = lens[b];
  len = len < 0 ? 0 : (len > Lcap - 1 ? Lcap - 1 : len);
  const int n = len + 1, j0 = ch * C;
  float* part = ws + ((long long)bh * nch + ch) * ATTN_WS;
  if (j0 < n) {   // block-uniform: a chunk wholly past the sequence writes nothing
    const int c8 = lane & 7, kr = lane >> 3;
    float qf[8];
    unpack8(*reinterpret_cast<const uint4*>(q + (long long)b * ldq + h * 64 + c8 * 8), qf);
    const float sc = scale * LOG2E;
#pragma unroll
    for (int k = 0; k < 8; ++k) qf[k] *= sc;
    const long long base = (long long)bh * Lcap * 64 + c8 * 8;
    float s[R];
    uint4 kv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i * 32 + wv * 8 + kr;
      kv[i] = j < n ? *reinterpret_cast<const uint4*>(kc + base + (long long)j * 64) : make_uint4(0, 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i * 32 + wv * 8 + kr;
      float kf[8], d = 0.f;
      unpack8(kv[i], kf);
#pragma unroll
      for (int k = 0; k < 8; ++k) d = fmaf(qf[k], kf[k], d);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      s[i] = j < n ? d : -INFINITY;
      mx = fmaxf(mx, s[i]);
    }
    // V rows in flight while the maximum crosses the block
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i * 32 + wv * 8 + kr;
      kv[i] = j < n ? *reinterpret_cast<const uint4*>(vc + base + (long long)j * 64) : make_uint4(0, 0, 0, 0);
    }
    mx = wave_max(mx);
    if (lane == 0) sm[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));   // finite: key j0 is valid
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ls = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i * 32 + wv * 8 + kr;
      const float p = j < n ? __builtin_amdgcn_exp2f(s[i] - mx) : 0.f;
      float vf[8];
      unpack8(kv[i], vf);
      ls += p;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = fmaf(p, vf[k], o[k]);
    }
#pragma unroll
    for (int sh = 8; sh < 64; sh <<= 1) {
      ls += __shfl_xor(ls, sh, 64);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] += __shfl_xor(o[k], sh, 64);
    }
    if (lane < 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) so[wv][c8 * 8 + k] = o[k];
    }
    if (lane == 0) ss[wv] = ls;
    __syncthreads();
    if (threadIdx.x < 64)
      st_part(part + 2 + threadIdx.x,
              ((so[0][threadIdx.x] + so[1][threadIdx.x]) + so[2][threadIdx.x]) + so[3][threadIdx.x]);
    if (threadIdx.x == 64) {
      st_part(part, mx);
      st_part(part + 1, ((ss[0] + ss[1]) + ss[2]) + ss[3]);
    }
  }
  if (!last_block(cnt + bh, (unsigned)nch, &sh_last)) return;
  if (threadIdx.x >= 64) return;
  const float* p0 = ws + (long long)bh * nch * ATTN_WS;
  const int nv = len / C + 1;   // <= nch: len < Lcap
  float M = -INFINITY;
  for (int c = 0; c < nv; ++c) M = fmaxf(M, ld_part(p0 + c * ATTN_WS));
  float S = 0.f, O = 0.f;
  for (int c = 0; c < nv; ++c) {
    const float w = __builtin_amdgcn_exp2f(ld_part(p0 + c * ATTN_WS) - M);
    S = fmaf(w, ld_part(p0 + c * ATTN_WS + 1), S);
    O = fmaf(w, ld_part(p0 + c * ATTN_WS + 2 + threadIdx.x), O);
  }
  out[(long long)b * ldo + h * 64 + threadIdx.x] = f2bf(O / S);
}

// ------------------------------------------------------------------------------- skinny GEMM
// grid (ceil(N / 16), S), NW waves.  A block owns 16 weight rows and `cps` 64-wide K chunks;
// wave w takes chunks w, w + NW, ... of them.  v_mfma_f32_16x16x32_bf16 with the weight rows as
// the first operand and the (zero-padded to 16) x rows as the second; a lane's two fragments of a
// chunk are 32 contiguous bytes (k = 64 c + 16 (lane>>4) + 8 j), so a wave instruction pair reads
// 128 contiguous bytes of each of its 16 rows.  x comes straight from L2 into registers beside
// the weights.  Result: lane holds y[m = lane&15][n0 + 4 (lane>>4) + i].  The waves are summed in wave order through LDS; with S > 1 the block's partial
// goes to the workspace and the last block of the row group folds splits 0 .. S-1 in that order.
// The order of every sum depends on (N, K) alone, so a row's result does not depend on M or on
// the other rows.  Two shapes of block: 16 waves (the layer weights: K of 768 .. 3072 spread over
// the waves of one block, so N >= 1536 needs no block split) and 4 waves (vocabulary-sized N:
// thousands of blocks, 12 or 13 per CU, where a 16-wave block's tail would leave CUs idle).
constexpr int SK_NONE = 0, SK_GELU = 1, SK_GELU_TANH = 2;   // SK_GELU: erf form; SK_GELU_TANH: kml_gelu_tanh

template <int NW, int U>
__global__ __launch_bounds__(NW * 64) void k_gemm_skinny(const bf16_t* __restrict__ x, int ldx,
                                                         const bf16_t* __restrict__ w, int ldw,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                         int ldy, int M, int N, int K, int cps, int act,
                                                         float* __restrict__ ws, unsigned* __restrict__ cnt) {
  constexpr int NT = NW * 64, E = 256;
  __shared__ float red[NW][E];
  __shared__ unsigned sh_last;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int nb = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
  const int n0 = nb * 16;
  const int nk = (K + 63) >> 6;
  const int c0 = sp * cps;
  const int c1 = c0 + cps < nk ? c0 + cps : nk;
  const bool xok = r < M, wok = n0 + r < N;
  const bf16_t* wp = w + (long long)(wok ? n0 + r : 0) * ldw + g * 16;
  const bf16_t* xp = x + (long long)(xok ? r : 0) * ldx + g * 16;
  const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int cb = c0 + wv; cb < c1; cb += NW * U) {
    bf16x8_t a[U][2], bq[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = cb + NW * u;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool ok = c < c1 && c * 64 + g * 16 + j * 8 < K;   // K % 8 == 0: a fragment is in or out
        a[u][j] = ok && wok ? *reinterpret_cast<const bf16x8_t*>(wp + c * 64 + j * 8) : zero;
        bq[u][j] = ok && xok ? *reinterpret_cast<const bf16x8_t*>(xp + c * 64 + j * 8) : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][j], bq[u][j], acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wv][i * 64 + lane] = acc[i];
  __syncthreads();
  // element e = 64 i + lane of the block's 16 x 16 tile, as stored above
  auto finish = [&](int e, float v) {
    const int m = e & 15, n = n0 + ((e & 63) >> 4) * 4 + (e >> 6);
    if (m >= M || n >= N) return;
    if (bias) v += bias[n];
    if (act == SK_GELU) v = kml_gelu(v);
    else if (act == SK_GELU_TANH) v = kml_gelu_tanh(v);
    y[(long long)m * ldy + n] = f2bf(v);
  };
  float* mine = ws + ((long long)nb * S + sp) * E;
  for (int e = threadIdx.x; e < E; e += NT) {
    float v = red[0][e];
#pragma unroll
    for (int k = 1; k < NW; ++k) v += red[k][e];
    if (S > 1) st_part(mine + e, v);
    else finish(e, v);
  }
  if (S == 1) return;
  if (!last_block(cnt + nb, (unsigned)S, &sh_last)) return;
  const float* p0 = ws + (long long)nb * S * E;
  for (int e = threadIdx.x; e < E; e += NT) {
    float v = ld_part(p0 + e);
    for (int s2 = 1; s2 < S; ++s2) v += ld_part(p0 + (long long)s2 * E + e);
    finish(e, v);
  }
}

// Block shape and K split of an (N, K) weight — a function of (N, K) alone.  Vocabulary-sized N
// (>= 2048 row groups): blocks of 4 waves, no split.  Otherwise blocks of 16 waves; N >= 1536 gives
// enough blocks as it is, below that K is split until ~192 blocks stream, at least 12 chunks
// (one per wave of three quarters of the block) each.  splits > 0 overrides the split (tuning).
struct SkinnyPlan {
  int big, S, cps, groups;
};
static inline SkinnyPlan skinny_plan(int N, int K, int splits) {
  const int nk = (K + 63) / 64, n16 = (N + 15) / 16;
  SkinnyPlan p;
  p.big = n16 >= 2048;
  int S = 1;
  if (splits > 0) {
    S = splits;
  } else if (!p.big && n16 < 96) {
    S = (192 + n16 - 1) / n16;
    if (S > nk / 12) S = nk / 12;
  }
  if (S > nk) S = nk;
  if (S < 1) S = 1;
  p.cps = (nk + S - 1) / S;
  p.S = (nk + p.cps - 1) / p.cps;
  p.groups = n16;
  return p;
}

// ------------------------------------------------------------------------------- embedding at lens
__global__ __launch_bounds__(64) void k_embed2_at(const long long* __restrict__ ids, const int* __restrict__ lens,
                                                  const bf16_t* __restrict__ word, const bf16_t* __restrict__ pos,
                                                  bf16_t* __restrict__ out, int N, long long vocab, int max_pos) {
  const int b = blockIdx.x, lane = threadIdx.x;
  long long id = ids[b];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  int p = lens[b];
  p = p < 0 ? 0 : (p >= max_pos ? max_pos - 1 : p);
  for (int c = lane * 4; c < N; c += 256) {
    const uint2 a = *reinterpret_cast<const uint2*>(word + id * N + c);
    const uint2 e = *reinterpret_cast<const uint2*>(pos + (long long)p * N + c);
    uint2 o;
    o.x = pack_bf2(lo_bf(a.x) + lo_bf(e.x), hi_bf(a.x) + hi_bf(e.x));
    o.y = pack_bf2(lo_bf(a.y) + lo_bf(e.y), hi_bf(a.y) + hi_bf(e.y));
    *reinterpret_cast<uint2*>(out + (long long)b * N + c) = o;
  }
}

// ------------------------------------------------------------------------------- next token
// ctl = [seed, step, eos (-1: none), unused] int32; temp = [temperature] fp32 (read when sample).
// One block per sequence.  Key of column c: logit (greedy) or logit / T + Gumbel(u), u a 23-bit
// uniform in (0, 1) from hash(seed ^ mix(b), step, c).  Largest key wins, lowest column on ties.
// Every block reads the step before its ticket; the last one advances it.
__device__ __forceinline__ float gumbel_key(float v, float invT, unsigned sb, unsigned step, unsigned c) {
  // (k + 1/2) 2^-23, k < 2^23: exact in fp32, never 0 or 1
  const float u = ((float)(hash3(sb, step, c) >> 9) + 0.5f) * 1.1920928955078125e-7f;
  return fmaf(v, invT, -logf(-logf(u)));
}

// What one thread of block b does with the chosen column: eos, tokens, lens; the last block
// of the grid advances the step.
__device__ __forceinline__ void advance_tail(int b, int bi, int classes, int eos, unsigned step, int* __restrict__ ctl,
                                             long long* __restrict__ next_ids, long long* __restrict__ tokens,
                                             int* __restrict__ lens, int* __restrict__ finished, int Lcap,
                                             unsigned* __restrict__ ticket) {
  if (bi >= classes) bi = 0;   // a row without one comparable value (all NaN)
  long long tok = bi;
  if (eos >= 0 && finished[b]) tok = eos;
  if (eos >= 0 && tok == eos) finished[b] = 1;
  const int len = lens[b];
  next_ids[b] = tok;
  if (len >= -1 && len + 1 < Lcap) tokens[(long long)b * Lcap + len + 1] = tok;
  lens[b] = len + 1 < Lcap ? (len + 1 < 0 ? 0 : len + 1) : Lcap - 1;
  __threadfence();
  const unsigned tk = atomicAdd(ticket, 1u);
  if (tk == gridDim.x - 1) {
    ctl[1] = (int)(step + 1u);
    atomicExch(ticket, 0u);
  }
}

__global__ __launch_bounds__(256) void k_decode_advance(const bf16_t* __restrict__ logits, int ldl, int classes,
                                                        int sample, const float* __restrict__ temp,
                                                        int* __restrict__ ctl, long long* __restrict__ next_ids,
                                                        long long* __restrict__ tokens, int* __restrict__ lens,
                                                        int* __restrict__ finished, int Lcap,
                                                        unsigned* __restrict__ ticket) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned seed = (unsigned)ctl[0], step = (unsigned)ctl[1];
  const int eos = ctl[2];
  const float invT = sample ? 1.f / temp[0] : 1.f;
  const unsigned sb = seed ^ ((unsigned)b * 0x9E3779B9u + 0x67756D62u);
  const bf16_t* row = logits + (long long)b * ldl;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c0 = tid * 8; c0 < classes; c0 += 2048) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(row + c0), f);   // ldl % 8 == 0: the row covers c0 .. c0 + 7
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c0 + k;
      float v = f[k];
      if (sample) v = gumbel_key(v, invT, sb, step, (unsigned)c);
      if (c < classes && (v > best || (v == best && c < bi))) { best = v; bi = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { sv[wv] = best; si[wv] = bi; }
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 4; ++k)
    if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
  advance_tail(b, bi, classes, eos, step, ctl, next_ids, tokens, lens, finished, Lcap, ticket);
}

// ------------------------------------------------------------------ next token, filtered
// kml_decode_sample: k_decode_advance's choice after HF's processor chain on the row —
// repetition penalty, (temperature,) top-k, top-p — in one launch, one block of 1024 threads per
// sequence.  fpar = [temperature, top_p, penalty, fp32(1 / penalty)], ipar = [top_k].
//
// After the penalty a logit is a bf16 again, one of 65536 values, so selection is exact counting:
//   1. bitmap of the distinct ids in tokens[b, 0 .. lens[b]] (LDS, integer or);
//   2. histogram of the penalised row over a monotone 16-bit key (-0 folded into +0, NaN left
//      out): 65536 16-bit counts, two to a dword (a count is at most `classes` <= 65535);
//   3. thread t owns the 64 keys 65535 - 64 t .. 65472 - 64 t: block scans over the threads walk
//      the value classes in descending order.  Counts give the maximum and the k-th largest
//      value; the mass of a class is count * round(2^46 * exp2((v - vmax) log2e / T)) as a
//      64-bit integer (fp64 exp2; the sum over a row stays under 2^62), so the prefix masses
//      and the p * Z crossing do not depend on any order of arrival;
//   4. a second pass over the row picks the largest key among the columns at or above the
//      threshold value.
// The histogram is stored transposed (dword j of chunk ch at j * 1024 + ch) so that the
// per-thread walks of consecutive threads fall on consecutive banks.
// info[b] = [threshold value, kept columns, kept mass / mass of all non-NaN columns, vmax].
constexpr int SMP_THREADS = 1024;
constexpr int SMP_MAX_CLASSES = 65535;   // 16-bit counts; the id bitmap covers 65536 bits
constexpr int SMP_FX = 46;               // fixed-point bits of a class weight

__device__ __forceinline__ bool bf_is_nan(unsigned h) { return (h & 0x7fffu) > 0x7f80u; }
// monotone key of a non-NaN bf16: negative values 0 .. 0x7ffe, +-0 0x8000, positive up to 0xffff
__device__ __forceinline__ unsigned bf_key(unsigned h) {
  h = h == 0x8000u ? 0u : h;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
__device__ __forceinline__ float key_val(unsigned key) {
  const unsigned h = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return __uint_as_float(h << 16);
}
__device__ __forceinline__ unsigned hist_at(const unsigned* hist, unsigned key) {
  const unsigned d = key >> 1;
  return (hist[(d & 31u) * 1024u + (d >> 5)] >> ((key & 1u) * 16u)) & 0xffffu;
}
template <class V>
__device__ __forceinline__ V wave_scan(V v, int lane) {   // inclusive, lane order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

__global__ __launch_bounds__(SMP_THREADS) void k_decode_sample(
    const bf16_t* __restrict__ logits, int ldl, int classes, int sample, const float* __restrict__ fpar,
    const int* __restrict__ ipar, float* __restrict__ info, int* __restrict__ ctl, long long* __restrict__ next_ids,
    long long* __restrict__ tokens, int* __restrict__ lens, int* __restrict__ finished, int Lcap,
    unsigned* __restrict__ ticket) {
  __shared__ __attribute__((aligned(16))) unsigned hist[32768];
  __shared__ __attribute__((aligned(16))) unsigned bm[2048];
  __shared__ unsigned long long wmass[16], s_zall, s_pexm, s_keptm;
  __shared__ unsigned wcnt[16];
  __shared__ int s_kmax, s_keyk, s_nk, s_psel, s_pexc, s_thr, s_keptc;
  __shared__ float sv[16];
  __shared__ int si[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned seed = (unsigned)ctl[0], step = (unsigned)ctl[1];
  const int eos = ctl[2];
  const float T = fpar[0], topp = fpar[1], pen = fpar[2], ipen = fpar[3];
  const int topk = ipar[0];
  const bool penon = pen != 1.f;
  const bf16_t* row = logits + (long long)b * ldl;

  for (int i = tid; i < 8192; i += SMP_THREADS) reinterpret_cast<uint4*>(hist)[i] = make_uint4(0, 0, 0, 0);
  if (tid < 512) reinterpret_cast<uint4*>(bm)[tid] = make_uint4(0, 0, 0, 0);
  if (tid == 0) {
    s_zall = s_pexm = s_keptm = 0ull;
    s_kmax = -1; s_keyk = 0; s_nk = -1; s_psel = 0; s_pexc = 0; s_thr = 0; s_keptc = 0;
  }
  __syncthreads();
  if (penon) {   // block-uniform
    int n = lens[b];
    n = n > Lcap - 1 ? Lcap - 1 : n;
    for (int i = tid; i <= n; i += SMP_THREADS) {
      const long long id = tokens[(long long)b * Lcap + i];
      if (id >= 0 && id < classes) atomicOr(&bm[id >> 5], 1u << (id & 31));   // classes <= 65535
    }
    __syncthreads();
  }
  // the penalised bf16 of column c (raw bits h)
  auto penalised = [&](unsigned h, int c) -> unsigned {
    if (penon && ((bm[c >> 5] >> (c & 31)) & 1u)) {
      const float f = bf2f((bf16_t)h);
      h = f2bf(f > 0.f ? f * ipen : f * pen);
    }
    return h;
  };
  for (int c0 = tid * 8; c0 < classes; c0 += SMP_THREADS * 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + c0);   // ldl % 8 == 0: the row covers c0 .. c0 + 7
    const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c0 + k;
      if (c >= classes) continue;
      const unsigned h = penalised((w4[k >> 1] >> ((k & 1) * 16)) & 0xffffu, c);
      if (bf_is_nan(h)) continue;
      const unsigned key = bf_key(h), d = key >> 1;
      atomicAdd(&hist[(d & 31u) * 1024u + (d >> 5)], 1u << ((key & 1u) * 16u));
    }
  }
  __syncthreads();

  // ---- counts: the maximum and the k-th largest value
  const int ch = SMP_THREADS - 1 - tid;   // chunk: keys 64 ch .. 64 ch + 63
  unsigned cnt = 0;
  for (int j = 0; j < 32; ++j) {
    const unsigned hw = hist[j * 1024 + ch];
    cnt += (hw & 0xffffu) + (hw >> 16);
  }
  const unsigned cincl = wave_scan(cnt, lane);
  if (lane == 63) wcnt[wv] = cincl;
  __syncthreads();
  unsigned coff = 0, total = 0;
  for (int k = 0; k < 16; ++k) {
    const unsigned w = wcnt[k];
    coff += k < wv ? w : 0u;
    total += w;
  }
  const unsigned cexcl = coff + cincl - cnt;
  if (total == 0u) {   // no comparable value in the row: token 0
    if (tid == 0) {
      const float qnan = __uint_as_float(0x7fc00000u);
      info[b * 4 + 0] = qnan; info[b * 4 + 1] = 0.f; info[b * 4 + 2] = 0.f; info[b * 4 + 3] = qnan;
      advance_tail(b, 0x7fffffff, classes, eos, step, ctl, next_ids, tokens, lens, finished, Lcap, ticket);
    }
    return;
  }
  const bool kon = topk > 0 && topk < classes && (unsigned)topk <= total;
  const bool first = cnt > 0u && cexcl == 0u;
  const bool kth = kon && cexcl < (unsigned)topk && (unsigned)topk <= cexcl + cnt;
  if (first || kth) {
    unsigned run = cexcl;
    bool fdone = !first, kdone = !kth;
    for (int q = 63; q >= 0 && !(fdone && kdone); --q) {
      const unsigned key = (unsigned)(ch * 64 + q), c = hist_at(hist, key);
      if (!c) continue;
      run += c;
      if (!fdone) { s_kmax = (int)key; fdone = true; }
      if (!kdone && run >= (unsigned)topk) { s_keyk = (int)key; s_nk = (int)run; kdone = true; }
    }
  }
  if (!kon && cnt > 0u && cexcl + cnt == total) {   // top-k off: the threshold is the smallest value
    for (int q = 0; q < 64; ++q) {
      const unsigned key = (unsigned)(ch * 64 + q);
      if (hist_at(hist, key)) { s_keyk = (int)key; break; }
    }
  }
  __syncthreads();

  // ---- masses: Z over the top-k survivors, the total over every non-NaN column
  const int kmax = s_kmax, keyk = s_keyk;
  const double vmax = (double)key_val((unsigned)kmax);
  const double sc = 1.4426950408889634 / (double)T;
  // the class weight of a value as a 2^-46 fixed-point number; the maximum's is exactly 1
  auto weight = [&](unsigned key) -> unsigned long long {
    if ((int)key == kmax) return 1ull << SMP_FX;
    return (unsigned long long)__double2ll_rn(exp2(((double)key_val(key) - vmax) * sc) * (double)(1ull << SMP_FX));
  };
  unsigned long long mk = 0ull, mall = 0ull;
  if (cnt) {
    for (int q = 63; q >= 0; --q) {
      const unsigned key = (unsigned)(ch * 64 + q), c = hist_at(hist, key);
      if (!c) continue;
      const unsigned long long wi = weight(key);
      mall += c * wi;
      if ((int)key >= keyk) mk += c * wi;
    }
  }
  if (mall) atomicAdd(&s_zall, mall);
  const unsigned long long mincl = wave_scan(mk, lane);
  if (lane == 63) wmass[wv] = mincl;
  __syncthreads();
  unsigned long long moff = 0ull, Z = 0ull;
  for (int k = 0; k < 16; ++k) {
    const unsigned long long w = wmass[k];
    moff += k < wv ? w : 0ull;
    Z += w;
  }
  const unsigned long long mexcl = moff + mincl - mk;
  const bool pon = topp < 1.f;
  unsigned long long tgt = 0ull;
  if (pon) {   // the smallest prefix of whole classes with mass >= p Z; Z >= 2^46: the maximum's class
    tgt = (unsigned long long)ceil((double)topp * (double)Z);
    tgt = tgt < 1ull ? 1ull : (tgt > Z ? Z : tgt);
    if (mk && mexcl < tgt && tgt <= mexcl + mk) { s_psel = ch; s_pexm = mexcl; s_pexc = (int)cexcl; }
  } else if (tid == 0) {
    s_thr = keyk; s_keptc = s_nk < 0 ? (int)total : s_nk; s_keptm = Z;
  }
  __syncthreads();
  if (pon && wv == 0) {   // the crossing inside the selected chunk: one key per lane, descending
    const unsigned key = (unsigned)(s_psel * 64 + 63 - lane), c = hist_at(hist, key);
    unsigned long long m = 0ull;
    if (c && (int)key >= keyk) {
      const unsigned long long wi = weight(key);
      m = c * wi;
    }
    const unsigned long long mi = s_pexm + wave_scan(m, lane);
    const unsigned ci = (unsigned)s_pexc + wave_scan(c, lane);
    const unsigned long long hit = __ballot(m != 0ull && mi >= tgt);
    if (hit && lane == __ffsll((long long)hit) - 1) { s_thr = (int)key; s_keptc = (int)ci; s_keptm = mi; }
  }
  if (pon) __syncthreads();
  const unsigned thr = (unsigned)s_thr;

  // ---- the pick among the kept columns
  const float invT = sample ? 1.f / T : 1.f;
  const unsigned sb = seed ^ ((unsigned)b * 0x9E3779B9u + 0x67756D62u);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c0 = tid * 8; c0 < classes; c0 += SMP_THREADS * 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + c0);
    const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c0 + k;
      if (c >= classes) continue;
      const unsigned h = penalised((w4[k >> 1] >> ((k & 1) * 16)) & 0xffffu, c);
      if (bf_is_nan(h) || bf_key(h) < thr) continue;
      float v = bf2f((bf16_t)h);
      if (sample) v = gumbel_key(v, invT, sb, step, (unsigned)c);
      if (v > best || (v == best && c < bi)) { best = v; bi = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { sv[wv] = best; si[wv] = bi; }
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 16; ++k)
    if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
  info[b * 4 + 0] = key_val(thr);
  info[b * 4 + 1] = (float)s_keptc;
  info[b * 4 + 2] = (float)((double)s_keptm / (double)s_zall);
  info[b * 4 + 3] = (float)vmax;
  advance_tail(b, bi, classes, eos, step, ctl, next_ids, tokens, lens, finished, Lcap, ticket);
}

// ============================================================ speculative decoding (verify rounds)
// A round feeds Q = k + 1 rows per sequence — next_ids[b] and k draft tokens at positions
// lens[b] .. lens[b] + k — through the decode step and keeps the longest prefix of the drafts that
// the model itself would have picked.  Row j of a sequence is computed exactly as a plain step at
// length lens[b] + j computes it (same order of every sum), so the committed tokens are the ones
// plain decoding gives.

// ------------------------------------------------------------------- embedding of a round's rows
// out[b Q + j] = word[x_j] + pos[clamp(lens[b] + j)], x_0 = next_ids[b], x_j = draft[b, j - 1]
__global__ __launch_bounds__(64) void k_embed2_multi(const long long* __restrict__ next_ids,
                                                     const long long* __restrict__ draft,
                                                     const int* __restrict__ lens, const bf16_t* __restrict__ word,
                                                     const bf16_t* __restrict__ pos, bf16_t* __restrict__ out, int Q,
                                                     int N, long long vocab, int max_pos) {
  const int r = blockIdx.x, b = r / Q, j = r % Q, lane = threadIdx.x;
  long long id = j == 0 ? next_ids[b] : draft[(long long)b * (Q - 1) + j - 1];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  int p = lens[b] + j;
  p = p < 0 ? 0 : (p >= max_pos ? max_pos - 1 : p);
  for (int c = lane * 4; c < N; c += 256) {
    const uint2 a = *reinterpret_cast<const uint2*>(word + id * N + c);
    const uint2 e = *reinterpret_cast<const uint2*>(pos + (long long)p * N + c);
    uint2 o;
    o.x = pack_bf2(lo_bf(a.x) + lo_bf(e.x), hi_bf(a.x) + hi_bf(e.x));
    o.y = pack_bf2(lo_bf(a.y) + lo_bf(e.y), hi_bf(a.y) + hi_bf(e.y));
    *reinterpret_cast<uint2*>(out + (long long)r * N + c) = o;
  }
}

// ------------------------------------------------------------- decode attention, Q queries a head
// k_attn_decode for Q <= 16 queries per (sequence, head): query j sees keys 0 .. lens[b] + j.
// Same chunks and lane -> key map; grid (ceil(Lcap / C), B * H, ceil(Q / ATTN_QG)): a block serves a
// group of up to ATTN_QG consecutive queries.  It loads its chunk's K and V rows ONCE (up to its last
// query's length) and keeps them in registers; its queries then take turns.  For query j every
// sum is k_attn_decode's at length lens[b] + j: a key past that length scores -inf, has
// probability 0 and a zero V row by selection, a chunk wholly past it writes no partial, and the
// fold runs over chunks 0 .. (lens[b] + j) / C.  Partials: ws[((bh Q + j) nch + ch) * ATTN_WS];
// one ticket per (b, h, group).  The queries of a block are serial (a block-wide maximum each),
// which is why 16 of them are spread over four blocks and not given to one
// (profiles/r14/prompt_lookup.md).
constexpr int ATTN_QG = 4;   // queries per block: one per wave in the partial store and the fold
template <int C>
__global__ __launch_bounds__(256) void k_attn_decode_multi(const bf16_t* __restrict__ q, int ldq,
                                                           const bf16_t* __restrict__ kc,
                                                           const bf16_t* __restrict__ vc, const int* __restrict__ lens,
                                                           float* __restrict__ ws, unsigned* __restrict__ cnt,
                                                           bf16_t* __restrict__ out, int ldo, int H, int Lcap, int Q,
                                                           float scale) {
  constexpr int R = C / 32;
  static_assert(ATTN_QG == 4, "one query per wave of the 256-thread block");
  __shared__ float sm[ATTN_QG][4], ss[ATTN_QG][4], so[ATTN_QG][4][64];
  __shared__ unsigned sh_last;
  const int ch = blockIdx.x, bh = blockIdx.y, nch = gridDim.x;
  const int b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l0 = lens[b];
  auto qlen = [&](int qi) {
    const int l = l0 + qi;
    return l < 0 ? 0 : (l > Lcap - 1 ? Lcap - 1 : l);
  };
  const int q0 = blockIdx.z * ATTN_QG, q1 = q0 + ATTN_QG < Q ? q0 + ATTN_QG : Q;   // this block's queries
  const int nmax = qlen(q1 - 1) + 1, j0 = ch * C;
  if (j0 < nmax) {   // block-uniform
    const int c8 = lane & 7, kr = lane >> 3;
    const float sc = scale * LOG2E;
    const long long base = (long long)bh * Lcap * 64 + c8 * 8;
    uint4 kk[R], vv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i * 32 + wv * 8 + kr;
      kk[i] = j < nmax ? *reinterpret_cast<const uint4*>(kc + base + (long long)j * 64) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i * 32 + wv * 8 + kr;
      vv[i] = j < nmax ? *reinterpret_cast<const uint4*>(vc + base + (long long)j * 64) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll 1
    for (int qi = q0; qi < q1; ++qi) {
      const int n = qlen(qi) + 1, g = qi - q0;
      if (j0 >= n) continue;   // block-uniform: this query ends before the chunk
      float qf[8];
      unpack8(*reinterpret_cast<const uint4*>(q + ((long long)b * Q + qi) * ldq + h * 64 + c8 * 8), qf);
#pragma unroll
      for (int k = 0; k < 8; ++k) qf[k] *= sc;
      float s[R];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int j = j0 + i * 32 + wv * 8 + kr;
        float kf[8], d = 0.f;
        unpack8(kk[i], kf);
#pragma unroll
        for (int k = 0; k < 8; ++k) d = fmaf(qf[k], kf[k], d);
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        s[i] = j < n ? d : -INFINITY;
        mx = fmaxf(mx, s[i]);
      }
      mx = wave_max(mx);
      if (lane == 0) sm[g][wv] = mx;
      __syncthreads();
      mx = fmaxf(fmaxf(sm[g][0], sm[g][1]), fmaxf(sm[g][2], sm[g][3]));   // finite: key j0 is valid
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ls = 0.f;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int j = j0 + i * 32 + wv * 8 + kr;
        const bool ok = j < n;
        const float p = ok ? __builtin_amdgcn_exp2f(s[i] - mx) : 0.f;
        float vf[8];
        unpack8(vv[i], vf);
        ls += p;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = fmaf(p, ok ? vf[k] : 0.f, o[k]);   // a later query's row: 0, as unloaded
      }
#pragma unroll
      for (int sh = 8; sh < 64; sh <<= 1) {
        ls += __shfl_xor(ls, sh, 64);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] += __shfl_xor(o[k], sh, 64);
      }
      if (lane < 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) so[g][wv][c8 * 8 + k] = o[k];
      }
      if (lane == 0) ss[g][wv] = ls;
    }
    __syncthreads();
    const int qi = q0 + wv, g = wv;   // wave w stores query q0 + w (ATTN_QG == waves of a block)
    if (qi < q1 && j0 < qlen(qi) + 1) {   // wave-uniform
      float* part = ws + (((long long)bh * Q + qi) * nch + ch) * ATTN_WS;
      st_part(part + 2 + lane, ((so[g][0][lane] + so[g][1][lane]) + so[g][2][lane]) + so[g][3][lane]);
      if (lane == 0) {
        st_part(part, fmaxf(fmaxf(sm[g][0], sm[g][1]), fmaxf(sm[g][2], sm[g][3])));
        st_part(part + 1, ((ss[g][0] + ss[g][1]) + ss[g][2]) + ss[g][3]);
      }
    }
  }
  if (!last_block(cnt + (long long)bh * gridDim.z + blockIdx.z, (unsigned)nch, &sh_last)) return;
  const int qi = q0 + wv;
  if (qi < q1) {
    const float* p0 = ws + ((long long)bh * Q + qi) * nch * ATTN_WS;
    const int nv = qlen(qi) / C + 1;   // <= nch
    float M = -INFINITY;
    for (int c = 0; c < nv; ++c) M = fmaxf(M, ld_part(p0 + c * ATTN_WS));
    float S = 0.f, O = 0.f;
    for (int c = 0; c < nv; ++c) {
      const float w = __builtin_amdgcn_exp2f(ld_part(p0 + c * ATTN_WS) - M);
      S = fmaf(w, ld_part(p0 + c * ATTN_WS + 1), S);
      O = fmaf(w, ld_part(p0 + c * ATTN_WS + 2 + lane), O);
    }
    out[((long long)b * Q + qi) * ldo + h * 64 + lane] = f2bf(O / S);
  }
}

// --------------------------------------------------------------------------- n-gram drafter
// Prompt lookup: one block per sequence over its history tokens[b, 0 .. L], L = lens[b].  For
// g = min(G, L) .. 1: the suffix of g tokens ending at L is searched at the starts s <= L - g (an
// earlier occurrence with at least one token after it); the LARGEST such s wins — each thread keeps
// its largest, the block takes the maximum, so the result does not depend on any arrival order.
// The draft is the K tokens after the occurrence, the index clamped to L (the tail repeats the
// last copied token); with no match at any g every slot is tokens[b, L].
__global__ __launch_bounds__(256) void k_draft_lookup(const long long* __restrict__ tokens,
                                                      const int* __restrict__ lens, long long* __restrict__ draft,
                                                      int Lcap, int K, int G) {
  __shared__ int sw[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long* row = tokens + (long long)b * Lcap;
  int L = lens[b];
  L = L < 0 ? 0 : (L > Lcap - 1 ? Lcap - 1 : L);
  int from = L;   // first token to copy
  for (int g = G < L ? G : L; g >= 1; --g) {   // block-uniform
    int best = -1;
    for (int s = tid; s <= L - g; s += 256) {
      bool ok = true;
      for (int i = 0; i < g && ok; ++i) ok = row[s + i] == row[L - g + 1 + i];
      if (ok) best = s;   // s grows: the last hit is this thread's largest
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int ov = __shfl_xor(best, o, 64);
      best = ov > best ? ov : best;
    }
    if (lane == 0) sw[wv] = best;
    __syncthreads();
    const int a0 = sw[0] > sw[1] ? sw[0] : sw[1], a1 = sw[2] > sw[3] ? sw[2] : sw[3];
    best = a0 > a1 ? a0 : a1;
    __syncthreads();   // sw is written again at the next g
    if (best >= 0) { from = best + g; break; }
  }
  for (int j = tid; j < K; j += 256) {
    const int src = from + j < L ? from + j : L;
    draft[(long long)b * K + j] = row[src];
  }
}

// ----------------------------------------------------------------------- verify: pick and commit
// grid B * Q, one block per row r = b Q + j: k_decode_advance's scan (argmax, or the Gumbel key
// with lowest column on ties) with the noise step lens[b] + j - start[b] — the step plain decoding
// has when it reaches that position.  The picks go to pick[r] write-through; the last block of the
// grid (ticket, as in last_block) then commits every sequence in one thread:
//   p = lens[b]; frozen when p >= limit[b].  Otherwise pick j lands at tokens[b, p + j + 1] while
//   that is <= limit[b]; after pick j the walk goes on only if draft[b, j] == pick j and it was
//   not eos.  A sequence finished before the round commits eos in every slot.  next_ids[b] = the
//   last committed token, lens[b] = p + committed.
// stats int32 = [accepted drafts (sum), committed tokens (sum), max over b of limit - lens, 0].
__global__ __launch_bounds__(256) void k_verify_pick(const bf16_t* __restrict__ logits, int ldl, int classes, int sample,
                                                     const float* __restrict__ temp, const int* __restrict__ ctl,
                                                     const int* __restrict__ start, const int* __restrict__ limit,
                                                     const long long* __restrict__ draft, int* __restrict__ pick,
                                                     long long* __restrict__ next_ids, long long* __restrict__ tokens,
                                                     int* __restrict__ lens, int* __restrict__ finished,
                                                     int* __restrict__ stats, int B, int Q, int Lcap,
                                                     unsigned* __restrict__ ticket) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int r = blockIdx.x, b = r / Q, jr = r % Q;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned seed = (unsigned)ctl[0];
  const unsigned step = (unsigned)(lens[b] + jr - start[b]);   // read before the ticket: the commit moves lens
  const int eos = ctl[2];
  const float invT = sample ? 1.f / temp[0] : 1.f;
  const unsigned sb = seed ^ ((unsigned)b * 0x9E3779B9u + 0x67756D62u);
  const bf16_t* row = logits + (long long)r * ldl;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c0 = tid * 8; c0 < classes; c0 += 2048) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(row + c0), f);   // ldl % 8 == 0: the row covers c0 .. c0 + 7
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c0 + k;
      float v = f[k];
      if (sample) v = gumbel_key(v, invT, sb, step, (unsigned)c);
      if (c < classes && (v > best || (v == best && c < bi))) { best = v; bi = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { sv[wv] = best; si[wv] = bi; }
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 4; ++k)
    if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
  if (bi >= classes) bi = 0;   // a row without one comparable value (all NaN)
  __hip_atomic_store(pick + r, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tk != gridDim.x - 1) return;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int acc = 0, com = 0, rem = 0;
  for (int s = 0; s < B; ++s) {
    const int p = lens[s], lim = limit[s];
    int m = 0;
    if (p < lim) {
      int fin = finished[s];
      const bool was = eos >= 0 && fin;
      long long last = 0;
      for (int j = 0; j < Q; ++j) {
        const int at = p + j + 1;
        if (at > lim) break;
        const int pk = __hip_atomic_load(pick + s * Q + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long tok = was ? (long long)eos : (long long)pk;
        if (at >= 0 && at < Lcap) tokens[(long long)s * Lcap + at] = tok;
        last = tok;
        m = j + 1;
        if (was) continue;
        if (eos >= 0 && tok == eos) { fin = 1; break; }
        if (j == Q - 1 || draft[(long long)s * (Q - 1) + j] != tok) break;
      }
      finished[s] = fin;
      next_ids[s] = last;
      lens[s] = p + m;
      com += m;
      if (!was) acc += m - 1;
    }
    rem = lim - (p + m) > rem ? lim - (p + m) : rem;
  }
  stats[0] += acc;
  stats[1] += com;
  stats[2] = rem;
}

}  // namespace

// ========================================================================================= C ABI
KML_API int kml_kv_append(const bf16_t* qkv, int ldq, bf16_t* kc, bf16_t* vc, const int* lens, int B, int H, int Lq,
                          int Lcap, int decode, hipStream_t s) {
  if (!qkv || !kc || !vc || B < 1 || H < 1 || Lq < 1 || Lcap < 64 || Lcap % 64 || ldq % 8 || ldq < 3 * H * 64)
    return (int)hipErrorInvalidValue;
  if (decode && (Lq > 16 || !lens)) return (int)hipErrorInvalidValue;
  if (!decode && Lq > Lcap) return (int)hipErrorInvalidValue;
  const long long total = (long long)B * Lq * H * 16;
  hipLaunchKernelGGL(k_kv_append, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, qkv, ldq, kc, vc, lens, B, H,
                     Lq, Lcap, decode);
  KML_LAUNCH_CHECK();
}

// keys per chunk of kml_attn_decode (profiles/r12/kv_decode.md has the sweep)
#define KML_DECODE_CHUNK 256

KML_API int kml_attn_decode_chunk(void) { return KML_DECODE_CHUNK; }

// floats of workspace for a (B, H, Lcap) cache, sized for the smallest chunk any entry point takes
KML_API long long kml_attn_decode_ws_floats(int B, int H, int Lcap) {
  return (long long)B * H * ((Lcap + 63) / 64) * ATTN_WS;
}

static int attn_decode_launch(int chunk, const bf16_t* q, int ldq, const bf16_t* kc, const bf16_t* vc, const int* lens,
                              float* ws, unsigned* cnt, bf16_t* out, int ldo, int B, int H, int Lcap, float scale,
                              hipStream_t s) {
  if (!q || !kc || !vc || !lens || !ws || !cnt || !out || B < 1 || H < 1 || Lcap < 64 || Lcap % 64 || ldq % 8 ||
      ldq < H * 64 || ldo < H * 64 || (long long)B * H > 65535)
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((Lcap + chunk - 1) / chunk), (unsigned)(B * H));
#define KML_AD(CC)                                                                                                  \
  hipLaunchKernelGGL(k_attn_decode<CC>, grid, dim3(256), 0, s, q, ldq, kc, vc, lens, ws, cnt, out, ldo, H, Lcap, scale)
  switch (chunk) {
    case 64: KML_AD(64); break;
    case 128: KML_AD(128); break;
    case 256: KML_AD(256); break;
    case 512: KML_AD(512); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef KML_AD
  KML_LAUNCH_CHECK();
}

// q: row b of a [B, ldq] buffer, head h at columns 64h (the Q third of a fused QKV row);
// kc / vc [B, H, Lcap, 64]; ws from kml_attn_decode_ws_floats; cnt: B*H zeroed tickets
KML_API int kml_attn_decode(const bf16_t* q, int ldq, const bf16_t* kc, const bf16_t* vc, const int* lens, float* ws,
                            unsigned* cnt, bf16_t* out, int ldo, int B, int H, int Lcap, float scale, hipStream_t s) {
  return attn_decode_launch(KML_DECODE_CHUNK, q, ldq, kc, vc, lens, ws, cnt, out, ldo, B, H, Lcap, scale, s);
}

// the same kernel at another chunk size (64 / 128 / 256 / 512): the sweep of tools/bench_gpt_decode.py
KML_API int kml_attn_decode_sweep(int chunk, const bf16_t* q, int ldq, const bf16_t* kc, const bf16_t* vc,
                                  const int* lens, float* ws, unsigned* cnt, bf16_t* out, int ldo, int B, int H,
                                  int Lcap, float scale, hipStream_t s) {
  return attn_decode_launch(chunk, q, ldq, kc, vc, lens, ws, cnt, out, ldo, B, H, Lcap, scale, s);
}

// K splits kml_gemm_skinny takes for an (N, K) weight by default.  With S > 1 splits the caller
// provides a workspace of ceil(N / 16) * S * 256 floats and ceil(N / 16) zeroed tickets.
KML_API int kml_gemm_skinny_splits(int N, int K) {
  if (N < 1 || K < 8) return 0;
  return skinny_plan(N, K, 0).S;
}

// splits: 0 = the default plan, > 0 = that many K splits (the tuning sweep)
KML_API int kml_gemm_skinny(const bf16_t* x, int ldx, const bf16_t* w, int ldw, const float* bias, bf16_t* y, int ldy,
                            int M, int N, int K, int act, int splits, float* ws, unsigned* cnt, hipStream_t s) {
  if (!x || !w || !y || M < 1 || M > 16 || N < 1 || K < 8 || K % 8 || ldx % 8 || ldw % 8 || ldx < K || ldw < K ||
      ldy < N || (act != SK_NONE && act != SK_GELU && act != SK_GELU_TANH) || splits < 0)
    return (int)hipErrorInvalidValue;
  const SkinnyPlan p = skinny_plan(N, K, splits);
  if (p.S > 1 && (!ws || !cnt)) return (int)hipErrorInvalidValue;
  if (p.S > 65535) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)p.groups, (unsigned)p.S);
  if (p.big)
    hipLaunchKernelGGL((k_gemm_skinny<4, 4>), grid, dim3(256), 0, s, x, ldx, w, ldw, bias, y, ldy, M, N, K, p.cps,
                       act, ws, cnt);
  else
    hipLaunchKernelGGL((k_gemm_skinny<16, 4>), grid, dim3(1024), 0, s, x, ldx, w, ldw, bias, y, ldy, M, N, K, p.cps,
                       act, ws, cnt);
  KML_LAUNCH_CHECK();
}

KML_API int kml_embed2_at(const long long* ids, const int* lens, const bf16_t* word, const bf16_t* pos, bf16_t* out,
                          int B, int N, long long vocab, int max_pos, hipStream_t s) {
  if (!ids || !lens || !word || !pos || !out || B < 1 || N < 4 || N % 4 || vocab < 1 || max_pos < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed2_at, dim3((unsigned)B), dim3(64), 0, s, ids, lens, word, pos, out, N, vocab, max_pos);
  KML_LAUNCH_CHECK();
}

KML_API int kml_decode_advance(const bf16_t* logits, int ldl, int classes, int sample, const float* temp, int* ctl,
                               long long* next_ids, long long* tokens, int* lens, int* finished, int B, int Lcap,
                               unsigned* ticket, hipStream_t s) {
  if (!logits || !ctl || !next_ids || !tokens || !lens || !finished || !ticket || B < 1 || classes < 1 ||
      ldl % 8 || ldl < classes || Lcap < 1 || (sample && !temp))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_decode_advance, dim3((unsigned)B), dim3(256), 0, s, logits, ldl, classes, sample, temp, ctl,
                     next_ids, tokens, lens, finished, Lcap, ticket);
  KML_LAUNCH_CHECK();
}

// the largest `classes` kml_decode_sample takes (16-bit counts per value, 65536-bit id bitmap)
KML_API int kml_decode_sample_max_classes(void) { return SMP_MAX_CLASSES; }

// kml_decode_advance behind a repetition penalty, top-k and top-p: fpar fp32 [temperature, top_p,
// penalty, 1 / penalty], ipar int32 [top_k], info fp32 [B, 4] (written every call)
KML_API int kml_decode_sample(const bf16_t* logits, int ldl, int classes, int sample, const float* fpar,
                              const int* ipar, float* info, int* ctl, long long* next_ids, long long* tokens,
                              int* lens, int* finished, int B, int Lcap, unsigned* ticket, hipStream_t s) {
  if (!logits || !fpar || !ipar || !info || !ctl || !next_ids || !tokens || !lens || !finished || !ticket || B < 1 ||
      classes < 1 || classes > SMP_MAX_CLASSES || ldl % 8 || ldl < classes || Lcap < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_decode_sample, dim3((unsigned)B), dim3(SMP_THREADS), 0, s, logits, ldl, classes, sample, fpar,
                     ipar, info, ctl, next_ids, tokens, lens, finished, Lcap, ticket);
  KML_LAUNCH_CHECK();
}

// ------------------------------------------------------------------- verify rounds (Q rows a sequence)
// floats of workspace kml_attn_decode_multi needs: kml_attn_decode_ws_floats for each of Q queries
KML_API long long kml_attn_decode_multi_ws_floats(int B, int H, int Lcap, int Q) {
  return (long long)B * H * Q * ((Lcap + 63) / 64) * ATTN_WS;
}

// q: row b * Q + j of a [B * Q, ldq] buffer is query j of sequence b and sees keys 0 .. lens[b] + j;
// out [B * Q, ldo] likewise.  Row j is bit-identical to kml_attn_decode at lens[b] + j.  ws from
// kml_attn_decode_multi_ws_floats; cnt: B*H*Q zeroed tickets (one per (b, h) and group of queries is used).
KML_API int kml_attn_decode_multi(const bf16_t* q, int ldq, const bf16_t* kc, const bf16_t* vc, const int* lens,
                                  float* ws, unsigned* cnt, bf16_t* out, int ldo, int B, int H, int Lcap, int Q,
                                  float scale, hipStream_t s) {
  if (!q || !kc || !vc || !lens || !ws || !cnt || !out || B < 1 || H < 1 || Q < 1 || Q > 16 || Lcap < 64 ||
      Lcap % 64 || ldq % 8 || ldq < H * 64 || ldo < H * 64 || (long long)B * H > 65535)
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((Lcap + KML_DECODE_CHUNK - 1) / KML_DECODE_CHUNK), (unsigned)(B * H),
                  (unsigned)((Q + ATTN_QG - 1) / ATTN_QG));
  hipLaunchKernelGGL(k_attn_decode_multi<KML_DECODE_CHUNK>, grid, dim3(256), 0, s, q, ldq, kc, vc, lens, ws, cnt, out,
                     ldo, H, Lcap, Q, scale);
  KML_LAUNCH_CHECK();
}

// out [B * Q, N]: row b * Q + j = word[x_j] + pos[lens[b] + j], x_0 = next_ids[b], x_j = draft[b, j - 1]
// (draft int64 [B, Q - 1]; may be null when Q == 1)
KML_API int kml_embed2_multi(const long long* next_ids, const long long* draft, const int* lens, const bf16_t* word,
                             const bf16_t* pos, bf16_t* out, int B, int Q, int N, long long vocab, int max_pos,
                             hipStream_t s) {
  if (!next_ids || !lens || !word || !pos || !out || B < 1 || Q < 1 || Q > 16 || (Q > 1 && !draft) || N < 4 || N % 4 ||
      vocab < 1 || max_pos < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed2_multi, dim3((unsigned)(B * Q)), dim3(64), 0, s, next_ids, draft, lens, word, pos, out, Q,
                     N, vocab, max_pos);
  KML_LAUNCH_CHECK();
}

// draft int64 [B, K] from the history tokens[b, 0 .. lens[b]] (tokens int64 [B, Lcap]); G: longest n-gram tried
KML_API int kml_draft_lookup(const long long* tokens, const int* lens, long long* draft, int B, int Lcap, int K, int G,
                             hipStream_t s) {
  if (!tokens || !lens || !draft || B < 1 || Lcap < 1 || K < 1 || G < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_draft_lookup, dim3((unsigned)B), dim3(256), 0, s, tokens, lens, draft, Lcap, K, G);
  KML_LAUNCH_CHECK();
}

// logits [B * Q, ldl]; start / limit int32 [B]; draft int64 [B, Q - 1] (may be null when Q == 1); pick int32
// [B * Q] (written); stats int32 [4] (accumulated); ticket: one zeroed counter
KML_API int kml_verify_pick(const bf16_t* logits, int ldl, int classes, int sample, const float* temp, const int* ctl,
                            const int* start, const int* limit, const long long* draft, int* pick,
                            long long* next_ids, long long* tokens, int* lens, int* finished, int* stats, int B, int Q,
                            int Lcap, unsigned* ticket, hipStream_t s) {
  if (!logits || !ctl || !start || !limit || !pick || !next_ids || !tokens || !lens || !finished || !stats ||
      !ticket || B < 1 || Q < 1 || Q > 16 || (Q > 1 && !draft) || classes < 1 || ldl % 8 || ldl < classes || Lcap < 1 ||
      (sample && !temp))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_verify_pick, dim3((unsigned)(B * Q)), dim3(256), 0, s, logits, ldl, classes, sample, temp, ctl,
                     start, limit, draft, pick, next_ids, tokens, lens, finished, stats, B, Q, Lcap, ticket);
  KML_LAUNCH_CHECK();
}
