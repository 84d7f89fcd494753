// kml_attn.h — what the flash-attention kernels share whatever the head size
// (attention.hip: head dim 64, attention_d128.hip: head dim 128): the argument block, the
// XCD-aware block order, the MFMA / conversion helpers of the C-layout -> operand reuse.
#pragma once
#include "kml_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short v4s_t;
constexpr float LOG2E = 1.4426950408889634f;

struct AttnArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* o; const bf16_t* dout;
  bf16_t* out; bf16_t* dq; bf16_t* dk; bf16_t* dv;
  float* lse;          // [B*H][L] base-2 log-sum-exp of scaled scores
  float* dsum;         // [B*H][L] D = rowsum(dO * O)
  const float* bias;   // [B][L] additive key bias (natural-log units) or null
  int ldq, ldk, ldv, ldo, lddo, ldout, lddq, lddk, lddv;
  int B, H, L;
  float scale;         // softmax scale (1/sqrt(head dim))
  const float* ctr;    // [seed, step] (device) for attention dropout, or null
  unsigned salt;
  float pdrop;         // dropout probability (0: off)
  int xcd;             // XCD-aware block order (attn_blk); 0: plain grid order (A/B switch)
  unsigned char* keep; // dropout keep bits written by the forward, read by the backward (Drop), or null
  int G;               // grouped-query attention: query heads per K/V head (H = Hkv * G); 1: one K/V head each
  const int* key_start;   // [B][L] first key each query attends (BAND kernels: packed documents, windows) or null
};

// BAND kernels: a bound as read from key_start[b][t], held to the contract 0 <= key_start <= t, so
// that no tensor, whatever it holds, moves a walk or a mask outside the causal triangle
__device__ __forceinline__ int band_clamp(int v, int t) { return min(max(v, 0), t); }

// number of leading queries of the sequence row ks[0 .. L) whose bound is <= klast, for a dKV block
// whose last key is klast: the end of its query walk.  At least klast + 1 (key_start[q] <= q), so
// the search covers klast + 1 .. L.  Every wave runs it on its own, 64 probes a round (a 64-ary
// search over the monotone row: two dependent loads up to L = 4096, against twelve for a binary
// one), the verdicts gathered by a ballot, so the result is block-uniform without LDS.  Every probe
// lies in [lo, hi - 1], inside the row, and a round leaves less than 1/64 of the range, whatever
// the row holds.  Call with all 64 lanes active.
__device__ __forceinline__ int band_end(const int* ks, int klast, int L, int lane) {
  int lo = klast + 1, hi = L;   // the answer lies in [lo, hi]
  while (lo < hi) {
    const int step = (hi - lo + 63) >> 6;
    const int idx = min(lo + (lane + 1) * step, hi) - 1;   // lane 63 probes row hi - 1
    const unsigned long long past = __ballot(ks[idx] > klast);
    if (!past) return hi;   // rows lo .. hi - 1 all see klast
    const int c = __ffsll((long long)past) - 1;   // the first probe past klast
    hi = min(lo + (c + 1) * step, hi) - 1;   // its row: the answer is at most that
    lo = min(lo + c * step, hi);             // the row of the probe before it still sees klast
  }
  return lo;
}

// XCD-aware block order.  Blocks are dealt round-robin over the 8 XCDs (b and b + 8 share
// one), so with the plain (tile, b*h) grid the 8 tiles of one head land on 8 different L2s
// and each XCD fetches that head's K/V (or Q/dO) again.  Renumbered so each XCD runs a
// contiguous range of ids, tile fastest: the tiles of one head share one L2.
//
// GROUP (grouped-query forward / dQ, grid.y = B * H): the G query heads of a K/V head read the
// same K/V tiles.  Their ids stay inside one XCD's contiguous range (bh = kvbh * G + hg), and
// within the group the head runs fastest and the tile next: id = (kvbh * gx + xt) * G + hg, so the
// G blocks of one (K/V head, tile) are dispatched back to back on that XCD and walk the same K/V
// lines of its L2 together (causal: they also carry the same amount of work).
template <bool GROUP = false>
__device__ __forceinline__ void attn_blk(const AttnArgs& a, int& xt, int& bh) {
  const int gx = (int)gridDim.x, nwg = gx * (int)gridDim.y;
  const int lin = (int)blockIdx.y * gx + (int)blockIdx.x;
  if (!a.xcd) { xt = (int)blockIdx.x; bh = (int)blockIdx.y; return; }
  const int q = nwg >> 3, r = nwg & 7, x = lin & 7, k = lin >> 3;
  const int id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
  if constexpr (GROUP) {
    const int t = id / a.G, hg = id - t * a.G;
    const int kvbh = t / gx;
    xt = t - kvbh * gx;
    bh = kvbh * a.G + hg;
  } else {
    bh = id / gx;
    xt = id - bh * gx;
  }
}

// bf16 operand from 8 accumulator values of tiles 2ks, 2ks+1 (the permuted k order)
// (v_cvt_pk_bf16_f32: round-to-nearest-even, NaN stays NaN — one instruction per pair)
typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt2(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t{a, b}), bf16x2_hw));
}
__device__ __forceinline__ bf16x8_t pack_p(const f32x4_t& t0, const f32x4_t& t1) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
  const u32x4_t u = {cvt2(t0[0], t0[1]), cvt2(t0[2], t0[3]), cvt2(t1[0], t1[1]), cvt2(t1[2], t1[3])};
  return __builtin_bit_cast(bf16x8_t, u);
}
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32

// operand fragment straight from global: k = 32 ks + 8 g + j of the row at row_ptr
__device__ __forceinline__ bf16x8_t load_frag_g(const bf16_t* row_ptr, int ks, int g, bool ok) {
  if (!ok) { bf16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0}; return z; }
  return *reinterpret_cast<const bf16x8_t*>(row_ptr + 32 * ks + 8 * g);
}

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ void store4(bf16_t* p, const f32x4_t& v, float s) {
  uint2 w;
  w.x = pack_bf2(v[0] * s, v[1] * s);
  w.y = pack_bf2(v[2] * s, v[3] * s);
  *reinterpret_cast<uint2*>(p) = w;
}

inline bool aligned16(const void* p) { return (((unsigned long long)p) & 15ull) == 0; }

}  // namespace
