// attention_d128.hip — flash attention for head dim 128 on gfx950: the Llama-2/3, Mistral and
// Qwen2 head size.  Semantics of kml_attn_gqa_fwd / _bwd (attention.hip): token-major [B*L, ld]
// bf16 buffers used in place on the fused QKV / dQKV buffer, head h at column 128 h, K/V head
// h / G, additive key bias [B, L], any L >= 1 with tails masked, compile-time <BIAS, CAUSAL, GQA>,
// base-2 LSE, dQ / dKV recomputing P from it, no atomics, a fixed summation order.  No attention
// dropout.  MFMA layout, the C-layout -> operand reuse of P / dS through the k-permutation and the
// XCD block order are attention.hip's (its header); what differs is how the work is cut.
//
// Split.  A 64-row operand tile is 16 KB at this head size, so the D = 64 layouts (Q + double-
// buffered K and V, or double-buffered Q and dO) would take 80 / 64 KB and leave one or two blocks
// on a CU.  Here every kernel keeps its own 64 rows (queries, or keys in dKV) in registers, read
// straight from global as MFMA fragments (4 k-steps: 16 VGPRs per operand), and walks the other
// side in 32-row tiles: two operands x two buffers x 8 KB = 32 KB of LDS, one barrier per tile,
// the next tile's global loads in flight during this tile's MFMAs.
//
//   fwd  : block = (64 queries, b, query head), wave = 16 queries; per 32-key tile S^T = K Q^T
//          (2 key sub-tiles x 4 k-steps), online softmax (exp2 domain, lazy rescale), O^T += V^T P^T
//          (8 d-tiles x 1 k-step: the 32 keys of the tile are exactly one permuted MFMA k).
//          Causal: key tiles 0 .. 2 xt + 1; the two tiles on the diagonal take the general path.
//   dQ   : the same walk; S and dP = V dO^T per tile, dS in registers, dQ^T += K^T dS^T; also
//          writes D = rowsum(dO o O).
//   dKV  : block = (64 keys, b, K/V head), K and V fragments in registers (32 VGPRs), walks
//          (query head of the group, 32-query tile) as one flat sequence into one set of
//          accumulators adk[8] / adv[8].  Causal: from query tile 2 xt.
//
// LDS tile: 32 rows x 256 B, 16-byte chunk c of row r at r * 256 + ((c ^ ((r & 7) << 1)) << 4).
// A row spans all 64 banks exactly once, so the bank group of an access is its physical chunk.
//  * row fragments (ds_read_b128, lane: row l & 15, chunk 4 ks + g): the hardware serves 16 lanes
//    at a time — rows {0-3, 12-15} of one g with rows {4-11} of g ^ 1.  Each half holds every
//    value of r & 7 once, so (r & 7) << 1 spreads it over the 8 even chunk pairs and the
//    low chunk bit, which the swizzle leaves alone, separates g from g ^ 1: 16 distinct chunks.
//  * transpose reads (ds_read_b64_tr_b16, 32 lanes at a time): 8 consecutive rows (8-aligned), 32
//    contiguous bytes = chunks 2m, 2m + 1 of each; XOR with (r & 7) << 1 sends the 8 rows to the 8
//    distinct chunk pairs: all 64 banks once.
// (bank model: tools/lds_banks.py — both patterns cost 1 cycle for every ks, d-tile and row half)
//
// Registers / occupancy (the compiler's resource remarks: profiles/r22/attn_d128.md): the forward
// is built for 4 waves per SIMD (124-126 VGPRs), dQ for 3 (158-164: S and dP live together), dKV
// (64 accumulator + 32 K/V fragment registers, 192-198) for 2; no instantiation uses scratch.
#include "kml_attn.h"

namespace {

constexpr int HD = 128;    // head dim
constexpr int TR = 32;     // rows of a staged tile

__device__ __forceinline__ int swz(int r, int c) { return r * 256 + ((c ^ ((r & 7) << 1)) << 4); }

struct TileRegs { uint4 v[2]; };   // a 32 x 256 B tile over 256 threads

__device__ __forceinline__ void tile_load(TileRegs& R, const bf16_t* base, int ld, int row0, int L, int tid) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (tid >> 4) + 16 * u, c = tid & 15, row = row0 + r;
    R.v[u] = row < L ? *reinterpret_cast<const uint4*>(base + (long long)row * ld + c * 8) : make_uint4(0, 0, 0, 0);
  }
}

__device__ __forceinline__ void tile_store(char* lds, const TileRegs& R, int tid) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (tid >> 4) + 16 * u, c = tid & 15;
    *reinterpret_cast<uint4*>(lds + swz(r, c)) = R.v[u];
  }
}

// rows row0 + (lane & 15), k = 32 ks + 8 (lane >> 4) + j, ks = 0..3
__device__ __forceinline__ bf16x8_t frag_rows(const char* lds, int row0, int ks, int lane) {
  return *reinterpret_cast<const bf16x8_t*>(lds + swz(row0 + (lane & 15), 4 * ks + (lane >> 4)));
}

// f[j] = T[row(j)][col0 + (lane & 15)], row(j) = 4g + j (j < 4), 16 + 4g + j - 4 (j >= 4): the 32
// rows of the tile in the permuted k order of pack_p
__device__ __forceinline__ bf16x8_t frag_tr(const char* lds, int col0, int lane) {
  const int il = lane & 15, g = lane >> 4;
  const int col = col0 + 4 * (il & 3);
  const int r0 = 4 * g + (il >> 2), r1 = r0 + 16;
  const char* p0 = lds + swz(r0, col >> 3) + (col & 7) * 2;
  const char* p1 = lds + swz(r1, col >> 3) + (col & 7) * 2;
  v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(p0));
  v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(p1));
  bf16x8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return f;
}

// BAND (causal, kml_attn128_band_fwd / _bwd): query t attends keys key_start[b][t] .. t, key_start
// non-decreasing along a sequence — the first row of t's document in a packed batch, or
// max(0, t - W + 1) for a window.  Every bound is read from device memory (the grid does not depend
// on it) and clamped to [0, t].
//   fwd / dQ : the walk starts at tile kb0 = key_start[q0] / 32, the block's minimum, and the double
//              buffer's parity runs on kb - kb0.  Tiles that begin before key_start of the block's
//              last query take the general path, where a key before the lane's own bound scores
//              -inf (dQ: probability exactly 0) like a key past the query; the tiles between those
//              and the diagonal keep the fast path.  A row always sees its own key: no empty rows.
//   dKV      : the walk ends at the tile of the last query whose bound is not past the block's last
//              key (band_end: a 64-ary search of the monotone row by every wave, so block-uniform);
//              the tile's bounds are staged with its LSE and D.
// With key_start = 0 every BAND kernel does the arithmetic of its CAUSAL twin in the same order.

// ------------------------------------------------------------------------------ forward
template <bool BIAS, bool CAUSAL, bool GQA, bool BAND = false>
__global__ __launch_bounds__(256, 4) void k_attn128_fwd(AttnArgs a) {
  static_assert(!BAND || CAUSAL, "BAND narrows the causal triangle");
  __shared__ __attribute__((aligned(16))) char sK2[2][TR * 256];
  __shared__ __attribute__((aligned(16))) char sV2[2][TR * 256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  int xt, bh;
  attn_blk<GQA>(a, xt, bh);
  const int b = bh / a.H, h = bh - b * a.H;
  const int hk = GQA ? h / a.G : h;   // K/V head
  const int L = a.L, q0 = xt * 64;
  const int qq = q0 + 16 * w + (lane & 15);   // this lane's query
  const bool qok = qq < L;
  const bf16_t* Kb = a.k + (long long)b * L * a.ldk + hk * HD;
  const bf16_t* Vb = a.v + (long long)b * L * a.ldv + hk * HD;
  const float sl2 = a.scale * LOG2E;
  const float* bias = BIAS ? a.bias + (long long)b * L : nullptr;
  // BAND: first tile of the walk, the bound of the block's last query, this lane's own bound
  int kb0 = 0, kse = 0, ksq = 0;
  if constexpr (BAND) {
    const int* ksr = a.key_start + (long long)b * L;
    const int qe = min(q0 + 63, L - 1);
    kb0 = band_clamp(ksr[q0], q0) / TR;
    kse = band_clamp(ksr[qe], qe);
    ksq = qok ? band_clamp(ksr[qq], qq) : 0;
  }

  TileRegs rk, rv;
  tile_load(rk, Kb, a.ldk, kb0 * TR, L, tid);
  tile_load(rv, Vb, a.ldv, kb0 * TR, L, tid);
  // Q: this lane's row as the B operand of the 4 k-steps, straight from global
  const bf16_t* qrow = a.q + (long long)(b * L + (qok ? qq : 0)) * a.ldq + h * HD;
  bf16x8_t qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = load_frag_g(qrow, ks, g, qok);
  tile_store(sK2[0], rk, tid);
  tile_store(sV2[0], rv, tid);
  const int nkb = (L + TR - 1) / TR;
  const int nk = CAUSAL ? min(nkb, 2 * xt + 2) : nkb;   // key tiles this block visits (causal: keys < q0 + 64)
  if (nk > kb0 + 1) {
    tile_load(rk, Kb, a.ldk, (kb0 + 1) * TR, L, tid);
    tile_load(rv, Vb, a.ldv, (kb0 + 1) * TR, L, tid);
  }
  __syncthreads();

  float m2 = -INFINITY, lsum = 0.f;
  f32x4_t acc[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) acc[d] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int kb = kb0; kb < nk; ++kb) {
    const char* sK = sK2[(kb - kb0) & 1];
    const char* sV = sV2[(kb - kb0) & 1];
    f32x4_t s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[t] = MFMA16(frag_rows(sK, 16 * t, ks, lane), qf[ks], s[t]);
    }
    // bias, key tail or a tile on the causal diagonal: scale + bias + mask every score; otherwise
    // the max of the raw scores (scale > 0) and one fma per probability below
    const bool gen = BIAS || kb * TR + TR > L || (CAUSAL && kb * TR + TR - 1 > q0) || (BAND && kb * TR < kse);
    float mx = -INFINITY;
    if (gen) {
      const int lim = qq - kb * TR - 4 * g;   // causal: 16t + i > lim is a key past the query
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = kb * TR + 16 * t + 4 * g + i;
          float v = s[t][i] * sl2;
          if (BIAS && key < L) v += bias[key] * LOG2E;
          if (key >= L) v = -INFINITY;
          if (CAUSAL && 16 * t + i > lim) v = -INFINITY;
          if (BAND && key < ksq) v = -INFINITY;
          s[t][i] = v;
          mx = fmaxf(mx, v);
        }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) mx = fmaxf(mx, fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])));
      mx *= sl2;
    }
    // lazy rescale (attention.hip): the running max moves only when a score exceeds it by 8; the
    // four lanes of a query column always agree on m2.  Causal: a column moves on its own scores
    // alone, so a row's bits do not depend on the later rows sharing its wave.
    if (__any(mx > m2 + 8.f)) {
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = CAUSAL ? (mx > m2 + 8.f ? mx : m2) : fmaxf(m2, mx);
      const float alpha = mn == -INFINITY ? 1.f : fexp2(m2 - mn);
      lsum *= alpha;
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[d] *= alpha;
      m2 = mn;
    }
    const float off = m2 == -INFINITY ? 0.f : m2;
    if (gen) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[t][i] = fexp2(s[t][i] - off);
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[t][i] = fexp2(fmaf(s[t][i], sl2, -off));
    }
    lsum += ((s[0][0] + s[0][1]) + (s[0][2] + s[0][3])) + ((s[1][0] + s[1][1]) + (s[1][2] + s[1][3]));
    const bf16x8_t p = pack_p(s[0], s[1]);
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = MFMA16(frag_tr(sV, 16 * d, lane), p, acc[d]);
    if (kb + 1 < nk) {   // buffer (kb+1)&1 last held tile kb-1: every wave left it at the last barrier
      tile_store(sK2[(kb + 1 - kb0) & 1], rk, tid);
      tile_store(sV2[(kb + 1 - kb0) & 1], rv, tid);
      if (kb + 2 < nk) {
        tile_load(rk, Kb, a.ldk, (kb + 2) * TR, L, tid);
        tile_load(rv, Vb, a.ldv, (kb + 2) * TR, L, tid);
      }
      __syncthreads();
    }
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (qok) {
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    bf16_t* op = a.out + (long long)(b * L + qq) * a.ldout + h * HD;
#pragma unroll
    for (int d = 0; d < 8; ++d) store4(op + 16 * d + 4 * g, acc[d], inv);
    if (g == 0) a.lse[(long long)bh * L + qq] = lsum > 0.f ? m2 + log2f(lsum) : INFINITY;
  }
}

// ------------------------------------------------------------------------------ backward: dQ (+D)
template <bool BIAS, bool CAUSAL, bool GQA, bool BAND = false>
__global__ __launch_bounds__(256, 3) void k_attn128_bwd_dq(AttnArgs a) {
  static_assert(!BAND || CAUSAL, "BAND narrows the causal triangle");
  __shared__ __attribute__((aligned(16))) char sK2[2][TR * 256];
  __shared__ __attribute__((aligned(16))) char sV2[2][TR * 256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  int xt, bh;
  attn_blk<GQA>(a, xt, bh);
  const int b = bh / a.H, h = bh - b * a.H;
  const int hk = GQA ? h / a.G : h;   // K/V head
  const int L = a.L, q0 = xt * 64;
  const int q = q0 + 16 * w + (lane & 15);
  const bool qok = q < L;
  const bf16_t* Kb = a.k + (long long)b * L * a.ldk + hk * HD;
  const bf16_t* Vb = a.v + (long long)b * L * a.ldv + hk * HD;
  const float sl2 = a.scale * LOG2E;
  const float* bias = BIAS ? a.bias + (long long)b * L : nullptr;
  int kb0 = 0, kse = 0, ksq = 0;   // BAND: as in k_attn128_fwd
  if constexpr (BAND) {
    const int* ksr = a.key_start + (long long)b * L;
    const int qe = min(q0 + 63, L - 1);
    kb0 = band_clamp(ksr[q0], q0) / TR;
    kse = band_clamp(ksr[qe], qe);
    ksq = qok ? band_clamp(ksr[q], q) : 0;
  }

  TileRegs rk, rv;
  tile_load(rk, Kb, a.ldk, kb0 * TR, L, tid);
  tile_load(rv, Vb, a.ldv, kb0 * TR, L, tid);
  const bf16_t* qrow = a.q + (long long)(b * L + (qok ? q : 0)) * a.ldq + h * HD;
  const bf16_t* dorow = a.dout + (long long)(b * L + (qok ? q : 0)) * a.lddo + h * HD;
  const bf16_t* orow = a.o + (long long)(b * L + (qok ? q : 0)) * a.ldo + h * HD;
  bf16x8_t qf[4], df[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qf[ks] = load_frag_g(qrow, ks, g, qok);
    df[ks] = load_frag_g(dorow, ks, g, qok);
  }
  // D = rowsum(dO * O): lane covers d = 32g .. 32g+31
  float D = 0.f;
  if (qok) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint4 x = *reinterpret_cast<const uint4*>(dorow + 32 * g + 8 * u);
      const uint4 y = *reinterpret_cast<const uint4*>(orow + 32 * g + 8 * u);
      D += lo_bf(x.x) * lo_bf(y.x) + hi_bf(x.x) * hi_bf(y.x) + lo_bf(x.y) * lo_bf(y.y) + hi_bf(x.y) * hi_bf(y.y) +
           lo_bf(x.z) * lo_bf(y.z) + hi_bf(x.z) * hi_bf(y.z) + lo_bf(x.w) * lo_bf(y.w) + hi_bf(x.w) * hi_bf(y.w);
    }
  }
  D += __shfl_xor(D, 16, 64);
  D += __shfl_xor(D, 32, 64);
  if (qok && g == 0) a.dsum[(long long)bh * L + q] = D;
  const float lse = qok ? a.lse[(long long)bh * L + q] : INFINITY;

  f32x4_t acc[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) acc[d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nkb = (L + TR - 1) / TR;
  const int nk = CAUSAL ? min(nkb, 2 * xt + 2) : nkb;   // key tiles this block visits (k_attn128_fwd)
  tile_store(sK2[0], rk, tid);
  tile_store(sV2[0], rv, tid);
  if (nk > kb0 + 1) {
    tile_load(rk, Kb, a.ldk, (kb0 + 1) * TR, L, tid);
    tile_load(rv, Vb, a.ldv, (kb0 + 1) * TR, L, tid);
  }
  __syncthreads();
  for (int kb = kb0; kb < nk; ++kb) {
    const char* sK = sK2[(kb - kb0) & 1];
    const char* sV = sV2[(kb - kb0) & 1];
    f32x4_t s[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      dp[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s[t] = MFMA16(frag_rows(sK, 16 * t, ks, lane), qf[ks], s[t]);
        dp[t] = MFMA16(frag_rows(sV, 16 * t, ks, lane), df[ks], dp[t]);
      }
    }
    // dS = P (.) (dP - D); bias / key tail / causal diagonal only on the general path.  A masked
    // probability (key > q) is exactly 0: the LSE excludes it
    const bool gen = BIAS || kb * TR + TR > L || (CAUSAL && kb * TR + TR - 1 > q0) || (BAND && kb * TR < kse);
    const int lim = q - kb * TR - 4 * g;   // causal: 16t + i > lim is a key past the query
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kb * TR + 16 * t + 4 * g + i;
        float p = 0.f;
        if (gen) {
          float v = s[t][i] * sl2;
          if (BIAS && key < L) v += bias[key] * LOG2E;
          if (key < L && !(CAUSAL && 16 * t + i > lim) && !(BAND && key < ksq)) p = fexp2(v - lse);
        } else {
          p = fexp2(fmaf(s[t][i], sl2, -lse));
        }
        s[t][i] = p * (dp[t][i] - D);
      }
    const bf16x8_t ds = pack_p(s[0], s[1]);
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = MFMA16(frag_tr(sK, 16 * d, lane), ds, acc[d]);
    if (kb + 1 < nk) {
      tile_store(sK2[(kb + 1 - kb0) & 1], rk, tid);
      tile_store(sV2[(kb + 1 - kb0) & 1], rv, tid);
      if (kb + 2 < nk) {
        tile_load(rk, Kb, a.ldk, (kb + 2) * TR, L, tid);
        tile_load(rv, Vb, a.ldv, (kb + 2) * TR, L, tid);
      }
      __syncthreads();
    }
  }
  if (qok) {
    bf16_t* op = a.dq + (long long)(b * L + q) * a.lddq + h * HD;
#pragma unroll
    for (int d = 0; d < 8; ++d) store4(op + 16 * d + 4 * g, acc[d], a.scale);
  }
}

// ------------------------------------------------------------------------------ backward: dK, dV
// grid.y = B * Hkv: one block per (64-key tile, b, K/V head), wave = 16 keys.  The walk is one flat
// sequence of (head of the group, 32-query tile) steps, head by head in ascending order and, within
// a head, the query tiles from 0 (causal: from 2 xt, the first tile that sees this key tile), so
// the Q / dO / LSE / D double buffer runs on across the head boundary.  Every step adds into the
// same fp32 accumulators, rounded to bf16 once at the end: a fixed order, bit-reproducible.
// Without a bias the keys past L score 0 instead of -inf: their rows are never stored and no other
// key's rows read them.
template <bool BIAS, bool CAUSAL, bool GQA, bool BAND = false>
__global__ __launch_bounds__(256, 2) void k_attn128_bwd_dkv(AttnArgs a) {
  static_assert(!BAND || CAUSAL, "BAND narrows the causal triangle");
  __shared__ __attribute__((aligned(16))) char sQ2[2][TR * 256];
  __shared__ __attribute__((aligned(16))) char sO2[2][TR * 256];   // dO tile
  __shared__ __attribute__((aligned(16))) float sL2[2][TR];
  __shared__ __attribute__((aligned(16))) float sD2[2][TR];
  __shared__ __attribute__((aligned(16))) int sS2[2][BAND ? TR : 4];   // BAND: the tile's key_start
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  int xt, bkv;   // bkv: b * Hkv + K/V head
  attn_blk(a, xt, bkv);
  const int G = GQA ? a.G : 1;
  const int Hkv = GQA ? a.H / G : a.H;
  const int b = bkv / Hkv, hk = bkv - b * Hkv;
  const int bh0 = b * a.H + hk * G;   // query bh of the group's first head
  const int L = a.L;
  const int kl = 16 * w + (lane & 15), key = xt * 64 + kl;
  const bool kok = key < L;
  const bf16_t* Qb = a.q + (long long)b * L * a.ldq + hk * G * HD;
  const bf16_t* Ob = a.dout + (long long)b * L * a.lddo + hk * G * HD;
  const float sl2 = a.scale * LOG2E;
  const bf16_t* krow = a.k + (long long)(b * L + (kok ? key : 0)) * a.ldk + hk * HD;
  const bf16_t* vrow = a.v + (long long)(b * L + (kok ? key : 0)) * a.ldv + hk * HD;
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    kf[ks] = load_frag_g(krow, ks, g, kok);
    vf[ks] = load_frag_g(vrow, ks, g, kok);
  }
  const float kb2 = BIAS ? (!kok ? -INFINITY : a.bias[(long long)b * L + key] * LOG2E) : 0.f;

  f32x4_t adk[8], adv[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) { adk[d] = f32x4_t{0.f, 0.f, 0.f, 0.f}; adv[d] = adk[d]; }
  const int nqb = (L + TR - 1) / TR;
  const int qs = CAUSAL ? 2 * xt : 0;   // 64 xt < L, so qs < nqb
  // BAND: the walk ends with the last query that still sees this block's last key (> qs tiles)
  const int* ksr = BAND ? a.key_start + (long long)b * L : nullptr;
  const int qe = BAND ? (band_end(ksr, min(xt * 64 + 63, L - 1), L, lane) + TR - 1) / TR : nqb;
  const int nit = G * (qe - qs);
  TileRegs rq, ro;
  float pl = 0.f, pd = 0.f;
  int pks = 0;
  int fh = 0, fq = qs;
  auto fetch = [&]() {   // request the next step's operands and move on, across the head boundary too
    const int nq0 = fq * TR, bh = bh0 + fh;
    tile_load(rq, Qb + fh * HD, a.ldq, nq0, L, tid);
    tile_load(ro, Ob + fh * HD, a.lddo, nq0, L, tid);
    if (tid < TR) {
      const int qq = nq0 + tid;
      pl = qq < L ? a.lse[(long long)bh * L + qq] : INFINITY;
      pd = qq < L ? a.dsum[(long long)bh * L + qq] : 0.f;
      if constexpr (BAND) pks = qq < L ? band_clamp(ksr[qq], qq) : 0;
    }
    ++fq;
    if (GQA && fq == qe) { fq = qs; ++fh; }
  };
  auto stage = [&](int j) {
    tile_store(sQ2[j], rq, tid);
    tile_store(sO2[j], ro, tid);
    if (tid < TR) {
      sL2[j][tid] = pl;
      sD2[j][tid] = pd;
      if constexpr (BAND) sS2[j][tid] = pks;
    }
  };
  fetch();
  stage(0);
  if (1 < nit) fetch();
  __syncthreads();
  int qb = qs;   // this step's query tile
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1;
    // the two tiles on the causal diagonal: queries 16t + i < lim come before this lane's key
    const int lim = CAUSAL && qb < 2 * xt + 2 ? key - qb * TR - 4 * g : 0;
    const char* sQ = sQ2[cur];
    const char* sO = sO2[cur];
    const float* sL = sL2[cur];
    const float* sD = sD2[cur];
    f32x4_t s[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      dp[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s[t] = MFMA16(frag_rows(sQ, 16 * t, ks, lane), kf[ks], s[t]);
        dp[t] = MFMA16(frag_rows(sO, 16 * t, ks, lane), vf[ks], dp[t]);
      }
    }
    // s[t][i] = S[q = 16t + 4g + i][key]; a query past L has LSE = +inf: probability exactly 0
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 l4 = *reinterpret_cast<const float4*>(sL + 16 * t + 4 * g);
      const float4 d4 = *reinterpret_cast<const float4*>(sD + 16 * t + 4 * g);
      const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
      const int4 s4 = BAND ? *reinterpret_cast<const int4*>(sS2[cur] + 16 * t + 4 * g) : make_int4(0, 0, 0, 0);
      const int sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float p = fexp2(fmaf(s[t][i], sl2, BIAS ? kb2 - lv[i] : -lv[i]));
        // diagonal: query < key is masked, its probability (and dS) exactly 0 — the LSE excludes it
        if (CAUSAL && 16 * t + i < lim) p = 0.f;
        if (BAND && key < sv[i]) p = 0.f;   // a key before the query's bound, likewise
        s[t][i] = p;
        dp[t][i] = p * (dp[t][i] - dv[i]);
      }
    }
    const bf16x8_t p = pack_p(s[0], s[1]), ds = pack_p(dp[0], dp[1]);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      adv[d] = MFMA16(frag_tr(sO, 16 * d, lane), p, adv[d]);
      adk[d] = MFMA16(frag_tr(sQ, 16 * d, lane), ds, adk[d]);
    }
    if (it + 1 < nit) {   // buffer cur^1 last held step it-1: every wave left it at the last barrier
      stage(cur ^ 1);
      if (it + 2 < nit) fetch();
      __syncthreads();
    }
    ++qb;
    if (GQA && qb == qe) qb = qs;
  }
  if (kok) {
    bf16_t* kp = a.dk + (long long)(b * L + key) * a.lddk + hk * HD;
    bf16_t* vp = a.dv + (long long)(b * L + key) * a.lddv + hk * HD;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      store4(kp + 16 * d + 4 * g, adk[d], a.scale);
      store4(vp + 16 * d + 4 * g, adv[d], 1.f);
    }
  }
}

template <bool CAUSAL, bool GQA, bool BAND = false>
int fwd_launch(const AttnArgs& a, hipStream_t s) {
  const dim3 grid((a.L + 63) / 64, a.B * a.H);
  if (a.bias) hipLaunchKernelGGL((k_attn128_fwd<true, CAUSAL, GQA, BAND>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_attn128_fwd<false, CAUSAL, GQA, BAND>), grid, dim3(256), 0, s, a);
  KML_LAUNCH_CHECK();
}

template <bool CAUSAL, bool GQA, bool BAND = false>
int bwd_launch(const AttnArgs& a, hipStream_t s) {
  const dim3 grid((a.L + 63) / 64, a.B * a.H);
  const dim3 grid_kv((a.L + 63) / 64, a.B * (a.H / a.G));   // dKV: one block per (key tile, b, K/V head)
  if (a.bias) {
    hipLaunchKernelGGL((k_attn128_bwd_dq<true, CAUSAL, GQA, BAND>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_attn128_bwd_dkv<true, CAUSAL, GQA, BAND>), grid_kv, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((k_attn128_bwd_dq<false, CAUSAL, GQA, BAND>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_attn128_bwd_dkv<false, CAUSAL, GQA, BAND>), grid_kv, dim3(256), 0, s, a);
  }
  KML_LAUNCH_CHECK();
}

// the argument checks and the launch table of kml_attn128_fwd / kml_attn128_band_fwd.  key_start:
// the BAND kernels (causal; the grouped-query instantiation serves Hkv == H too, with G = 1)
int fwd128(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, float* lse, const float* bias,
           const int* key_start, int ldq, int ldk, int ldv, int ldout, int B, int H, int Hkv, int L, float scale,
           int causal, hipStream_t s) {
  if (B <= 0 || L <= 0 || H <= 0 || Hkv <= 0 || H % Hkv) return (int)hipErrorInvalidValue;
  if (ldq % 8 || ldk % 8 || ldv % 8 || ldout % 4 || !aligned16(q) || !aligned16(k) || !aligned16(v))
    return (int)hipErrorInvalidValue;
  AttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse; a.bias = bias; a.key_start = key_start;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldout = ldout;
  a.B = B; a.H = H; a.L = L; a.scale = scale; a.xcd = 1; a.G = H / Hkv;
  if (key_start) return fwd_launch<true, true, true>(a, s);
  if (a.G == 1) return causal ? fwd_launch<true, false>(a, s) : fwd_launch<false, false>(a, s);
  return causal ? fwd_launch<true, true>(a, s) : fwd_launch<false, true>(a, s);
}

int bwd128(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* o, const bf16_t* dout, const float* lse,
           float* dsum, const float* bias, const int* key_start, bf16_t* dq, bf16_t* dk, bf16_t* dv, int ldq, int ldk,
           int ldv, int ldo, int lddo, int lddq, int lddk, int lddv, int B, int H, int Hkv, int L, float scale,
           int causal, hipStream_t s) {
  if (B <= 0 || L <= 0 || H <= 0 || Hkv <= 0 || H % Hkv) return (int)hipErrorInvalidValue;
  if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8 || lddo % 8 || lddq % 4 || lddk % 4 || lddv % 4)
    return (int)hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(dout))
    return (int)hipErrorInvalidValue;
  AttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.lse = const_cast<float*>(lse); a.dsum = dsum;
  a.bias = bias; a.key_start = key_start; a.dq = dq; a.dk = dk; a.dv = dv;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
  a.B = B; a.H = H; a.L = L; a.scale = scale; a.xcd = 1; a.G = H / Hkv;
  if (key_start) return bwd_launch<true, true, true>(a, s);
  if (a.G == 1) return causal ? bwd_launch<true, false>(a, s) : bwd_launch<false, false>(a, s);
  return causal ? bwd_launch<true, true>(a, s) : bwd_launch<false, true>(a, s);
}

}  // namespace

// Head dim 128 with the argument list of kml_attn_gqa_fwd: q/k/v/out token-major [B*L, ld*] bf16,
// query head h at column 128 h, k / v hold Hkv heads (H % Hkv == 0; Hkv == H allowed), lse fp32
// [B*H, L] (base 2).  ctr / salt / pdrop / keep are kept for symmetry: attention dropout is not
// implemented at this head size, pdrop > 0 is refused.
KML_API int kml_attn128_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, float* lse,
                            const float* bias, int ldq, int ldk, int ldv, int ldout, int B, int H, int Hkv, int L,
                            float scale, const float* ctr, int salt, float pdrop, unsigned char* keep, int causal,
                            hipStream_t s) {
  (void)ctr; (void)salt; (void)keep;
  if (!(pdrop == 0.f)) return (int)hipErrorInvalidValue;
  return fwd128(q, k, v, out, lse, bias, nullptr, ldq, ldk, ldv, ldout, B, H, Hkv, L, scale, causal, s);
}

// Causal attention with a per-query key start (the BAND kernels): key_start int32 [B, L] on the
// device, query t attends keys key_start[b][t] .. t; 0 <= key_start[b][t] <= t, non-decreasing in t
// (values are clamped to [0, t] as read).  The other arguments as kml_attn128_fwd; no dropout.
KML_API int kml_attn128_band_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, float* lse,
                                 const float* bias, const int* key_start, int ldq, int ldk, int ldv, int ldout,
                                 int B, int H, int Hkv, int L, float scale, hipStream_t s) {
  if (!key_start) return (int)hipErrorInvalidValue;
  return fwd128(q, k, v, out, lse, bias, key_start, ldq, ldk, ldv, ldout, B, H, Hkv, L, scale, 1, s);
}

// Head dim 128 with the argument list of kml_attn_gqa_bwd: dq / dk / dv may point into one fused
// [B*L, (H + 2 Hkv) * 128] buffer; dk / dv have Hkv * 128 columns, each head the sum over its group's
// query heads; dsum: [B*H*L] fp32 scratch (written by the dQ kernel, read by the dKV kernel).
KML_API int kml_attn128_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* o, const bf16_t* dout,
                            const float* lse, float* dsum, const float* bias, bf16_t* dq, bf16_t* dk, bf16_t* dv,
                            int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv, int B, int H,
                            int Hkv, int L, float scale, const float* ctr, int salt, float pdrop,
                            const unsigned char* keep, int causal, hipStream_t s) {
  (void)ctr; (void)salt; (void)keep;
  if (!(pdrop == 0.f)) return (int)hipErrorInvalidValue;
  return bwd128(q, k, v, o, dout, lse, dsum, bias, nullptr, dq, dk, dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, B,
                H, Hkv, L, scale, causal, s);
}

// The backward of kml_attn128_band_fwd (same key_start); the other arguments as kml_attn128_bwd.
KML_API int kml_attn128_band_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* o,
                                 const bf16_t* dout, const float* lse, float* dsum, const float* bias,
                                 const int* key_start, bf16_t* dq, bf16_t* dk, bf16_t* dv, int ldq, int ldk, int ldv,
                                 int ldo, int lddo, int lddq, int lddk, int lddv, int B, int H, int Hkv, int L,
                                 float scale, hipStream_t s) {
  if (!key_start) return (int)hipErrorInvalidValue;
  return bwd128(q, k, v, o, dout, lse, dsum, bias, key_start, dq, dk, dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                B, H, Hkv, L, scale, 1, s);
}
