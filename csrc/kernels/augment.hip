// augment.hip — on-device image batch preparation (gfx950).
//
// The dataset stays resident in HBM as raw uint8 NHWC (CIFAR-10 is 150 MB; 288 GB of
// HBM holds any of the reference's datasets many times over).  One kernel turns a
// contiguous range of samples into the network input:
//   random crop with zero padding (RandomCrop(32, 4)), random horizontal flip,
//   ToTensor (/255) + Normalize(mean, std), cast to bf16, NHWC with channels padded
//   to a multiple of 8 (the conv kernels' 16-byte vector width).
// Randomness is a counter-based hash of (seed, step, sample) where seed/step are read
// from device memory, so a hipGraph replay draws fresh crops every step.
// Reference transform chain: function_resnet34.py:17-30 (train) / :27-30 (val).
// kml_augment_mix is the same launch with mixup / CutMix: a per-step mix plan drawn from the
// same counters, a second gather (mixup) or a choice of sample (CutMix) per pixel, and packed
// (label, partner label, lam) targets for the soft cross-entropy (loss.hip).
// kml_augment_resample feeds the network another size than the stored one, the ImageNet chain:
// RandomResizedCrop + flip (train) or Resize + CenterCrop (eval) with the antialiased bilinear
// filter, mixing included; kml_rrc_plan reads the crop boxes back.
#include "kml_common.h"

namespace {

__device__ __forceinline__ unsigned hash3(unsigned a, unsigned b, unsigned c) {
  unsigned h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ (c + 0x165667B1u) * 0xC2B2AE3Du;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return h;
}

struct AugArgs {
  const unsigned char* src;  // [N][H][W][C] uint8
  const long long* labels_src;
  bf16_t* dst;               // [B][H][W][CP]
  long long* labels_dst;
  const float* ctr;          // device [seed, step, start]
  int N, H, W, C, CP, B;
  int pad, flip, train;
  float mean[4], inv_std[4];
};

// normalised channels v[0 .. C) of source sample sidx at output pixel (x, y), under that
// sample's own crop / flip draw
__device__ __forceinline__ void sample_pixel(const AugArgs& a, unsigned seed, unsigned step, long long sidx, int x,
                                             int y, float* v) {
  int dx = 0, dy = 0, fl = 0;
  if (a.train) {
    const unsigned h = hash3(seed, step, (unsigned)sidx);
    const int span = 2 * a.pad + 1;
    dy = (int)(h % span) - a.pad;
    dx = (int)((h / span) % span) - a.pad;
    fl = a.flip ? (int)((h >> 24) & 1) : 0;
  }
  int sx = fl ? (a.W - 1 - x) : x;
  sx += dx;
  const int sy = y + dy;
  if ((unsigned)sx < (unsigned)a.W && (unsigned)sy < (unsigned)a.H) {
    const unsigned char* p = a.src + ((sidx * a.H + sy) * a.W + sx) * a.C;
    for (int c = 0; c < a.C && c < 4; ++c) v[c] = ((float)p[c] * (1.f / 255.f) - a.mean[c]) * a.inv_std[c];
  } else {
    // zero padding happens BEFORE normalisation in the reference chain (pad on the uint8 image)
    for (int c = 0; c < a.C && c < 4; ++c) v[c] = (0.f - a.mean[c]) * a.inv_std[c];
  }
}

// v[0 .. 8) -> the pixel's CP channels (pad channels 0): one 16-byte store when CP == 8
__device__ __forceinline__ void store_pixel(bf16_t* o, int CP, const float* v) {
  if (CP == 8) {
    uint4 q;
    q.x = pack_bf2(v[0], v[1]); q.y = pack_bf2(v[2], v[3]); q.z = pack_bf2(v[4], v[5]); q.w = pack_bf2(v[6], v[7]);
    *reinterpret_cast<uint4*>(o) = q;
  } else {
    for (int c = 0; c < CP; ++c) o[c] = f2bf(c < 8 ? v[c] : 0.f);
  }
}

// one thread per output pixel (all CP channels -> one 16-byte store when CP == 8)
__global__ void k_augment(AugArgs a) {
  const long long total = (long long)a.B * a.H * a.W;
  const unsigned seed = (unsigned)a.ctr[0], step = (unsigned)a.ctr[1];
  const long long start = (long long)a.ctr[2];
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % a.W);
    const int y = (int)((t / a.W) % a.H);
    const int b = (int)(t / ((long long)a.W * a.H));
    const long long sidx = (start + b) % a.N;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    sample_pixel(a, seed, step, sidx, x, y, v);
    store_pixel(a.dst + t * a.CP, a.CP, v);
    if (x == 0 && y == 0 && a.labels_dst) a.labels_dst[b] = a.labels_src[sidx];
  }
}

// ---- mixup / CutMix ------------------------------------------------------------------------
// One mix plan per step, a function of (seed, step) alone, so every block of the augment launch
// (and kml_mix_plan) derives the same one and a graph replay draws a new one.  Its draws are
// hash3(seed ^ MIX_SALT, step, k): the salted seed keeps them apart from the per-sample
// crop / flip draws hash3(seed, step, sample).
enum { MIX_NONE = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2 };
struct MixCfg { float mixup_alpha, cutmix_alpha, mix_prob, switch_prob; };
struct MixPlan {
  int mode, r;          // r: sample b is mixed with batch row (b + r) % B
  float lam;            // weight of the sample's own label
  int x0, y0, x1, y1;   // CutMix box [x0, x1) x [y0, y1), clipped to the image
  int applied;
};

constexpr unsigned MIX_SALT = 0x4D495853u;
constexpr int MIX_GAMMA_TRIES = 16;
// draw indices: fixed ones, then one block of 3 * MIX_GAMMA_TRIES + 1 per gamma variate
enum { MIX_K_APPLY = 0, MIX_K_SWITCH = 1, MIX_K_SHIFT = 2, MIX_K_CX = 3, MIX_K_CY = 4, MIX_K_GAMMA = 8 };

__device__ __forceinline__ unsigned mix_bits(unsigned seed, unsigned step, unsigned k) {
  return hash3(seed ^ MIX_SALT, step, k);
}
// uniform in the open interval (0, 1): 23 bits, exact in fp32
__device__ __forceinline__ float mix_u01(unsigned seed, unsigned step, unsigned k) {
  return ((float)(mix_bits(seed, step, k) >> 9) + 0.5f) * (1.f / 8388608.f);
}

// log of a Gamma(a, 1) variate, a > 0: Marsaglia-Tsang rejection for a >= 1, and
// G(a) = G(a + 1) * U^(1/a) below 1 (taken in the log domain: U^(1/a) underflows fp32 for small
// a).  One try accepts with probability > 0.95; after MIX_GAMMA_TRIES rejections (< 1e-20) the
// variate is d = a - 1/3, the centre of the proposal, so the loop is bounded.
__device__ float mix_log_gamma(unsigned seed, unsigned step, unsigned k0, float a) {
  const float a1 = a < 1.f ? a + 1.f : a;
  const float d = a1 - (1.f / 3.f), c = rsqrtf(9.f * d);
  float g = d;
  for (int i = 0; i < MIX_GAMMA_TRIES; ++i) {
    const float u1 = mix_u01(seed, step, k0 + 3 * i), u2 = mix_u01(seed, step, k0 + 3 * i + 1);
    const float u3 = mix_u01(seed, step, k0 + 3 * i + 2);
    const float n = sqrtf(-2.f * __logf(u1)) * __builtin_amdgcn_cosf(u2);   // Box-Muller; v_cos takes revolutions
    const float t = 1.f + c * n;
    if (t <= 0.f) continue;
    const float v = t * t * t;
    if (__logf(u3) < 0.5f * n * n + d - d * v + d * __logf(v)) { g = d * v; break; }
  }
  float lg = __logf(g);
  if (a < 1.f) lg += __logf(mix_u01(seed, step, k0 + 3 * MIX_GAMMA_TRIES)) / a;
  return lg;
}

__device__ MixPlan mix_plan(unsigned seed, unsigned step, int B, int H, int W, const MixCfg& m) {
  MixPlan p = {MIX_NONE, 0, 1.f, 0, 0, 0, 0, 0};
  const bool mu = m.mixup_alpha > 0.f, cm = m.cutmix_alpha > 0.f;
  if (B < 2 || !(mu || cm)) return p;
  p.r = 1 + (int)(mix_bits(seed, step, MIX_K_SHIFT) % (unsigned)(B - 1));
  if (!(mix_u01(seed, step, MIX_K_APPLY) < m.mix_prob)) return p;
  p.applied = 1;
  const bool cut = cm && (!mu || mix_u01(seed, step, MIX_K_SWITCH) < m.switch_prob);
  // lam ~ Beta(alpha, alpha) = Ga / (Ga + Gb) = 1 / (1 + exp(log Gb - log Ga))
  const float alpha = cut ? m.cutmix_alpha : m.mixup_alpha;
  const float la = mix_log_gamma(seed, step, MIX_K_GAMMA, alpha);
  const float lb = mix_log_gamma(seed, step, MIX_K_GAMMA + 3 * MIX_GAMMA_TRIES + 1, alpha);
  const float lam = 1.f / (1.f + __expf(lb - la));
  if (!cut) {
    p.mode = MIX_MIXUP;
    p.lam = lam;
    return p;
  }
  const float ratio = sqrtf(1.f - lam);
  const int cw = (int)((float)W * ratio), ch = (int)((float)H * ratio);
  const int cx = (int)(mix_bits(seed, step, MIX_K_CX) % (unsigned)W);
  const int cy = (int)(mix_bits(seed, step, MIX_K_CY) % (unsigned)H);
  p.mode = MIX_CUTMIX;
  p.x0 = max(cx - cw / 2, 0); p.x1 = min(cx + cw / 2, W);
  p.y0 = max(cy - ch / 2, 0); p.y1 = min(cy + ch / 2, H);
  p.lam = 1.f - (float)((p.x1 - p.x0) * (p.y1 - p.y0)) / (float)(H * W);   // from the clipped box
  return p;
}

// k_augment with the step's mix plan (one thread computes it, LDS broadcasts it).  mixup: the
// sample's and the partner's pixel, each under its own crop / flip, blended in fp32 before the
// one store; CutMix: inside the box the partner's pixel at the same output coordinate.  The
// thread of pixel (0, 0) writes the packed target (label, partner label, lam).
__global__ void k_augment_mix(AugArgs a, float* __restrict__ targets, MixCfg m) {
  const long long total = (long long)a.B * a.H * a.W;
  const unsigned seed = (unsigned)a.ctr[0], step = (unsigned)a.ctr[1];
  const long long start = (long long)a.ctr[2];
  __shared__ MixPlan plan;
  if (threadIdx.x == 0) plan = mix_plan(seed, step, a.B, a.H, a.W, m);
  __syncthreads();
  const MixPlan p = plan;
  // start % N + batch row < 2^32: the two sample indices take 32-bit divisions
  const unsigned s0 = (unsigned)(start % a.N);
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % a.W);
    const int y = (int)((t / a.W) % a.H);
    const int b = (int)(t / ((long long)a.W * a.H));
    const int pb = b + p.r < a.B ? b + p.r : b + p.r - a.B;   // r < B
    const long long sidx = (s0 + (unsigned)b) % (unsigned)a.N;
    const long long pidx = (s0 + (unsigned)pb) % (unsigned)a.N;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.mode == MIX_CUTMIX) {
      const bool inside = x >= p.x0 && x < p.x1 && y >= p.y0 && y < p.y1;
      sample_pixel(a, seed, step, inside ? pidx : sidx, x, y, v);
    } else {
      sample_pixel(a, seed, step, sidx, x, y, v);
      if (p.mode == MIX_MIXUP) {
        float w[4] = {0, 0, 0, 0};
        sample_pixel(a, seed, step, pidx, x, y, w);
        // blend the two pixels as k_augment would store them (bf16): the mixed batch is then the
        // blend of two plain batches up to its one final rounding
        const unsigned a2[2] = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        const unsigned b2[2] = {pack_bf2(w[0], w[1]), pack_bf2(w[2], w[3])};
        const float om = 1.f - p.lam;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          v[2 * c] = fmaf(p.lam, lo_bf(a2[c]), om * lo_bf(b2[c]));
          v[2 * c + 1] = fmaf(p.lam, hi_bf(a2[c]), om * hi_bf(b2[c]));
        }
      }
    }
    store_pixel(a.dst + t * a.CP, a.CP, v);
    if (x == 0 && y == 0) {
      float* tg = targets + 3 * (long long)b;
      tg[0] = (float)a.labels_src[sidx];
      tg[1] = (float)a.labels_src[pidx];
      tg[2] = p.lam;
    }
  }
}

// plans of steps ctr[1] .. ctr[1] + n - 1 as rows (mode, r, lam, x0, y0, x1, y1, applied)
__global__ void k_mix_plan(const float* __restrict__ ctr, float* __restrict__ out, int n, int B, int H, int W,
                           MixCfg m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MixPlan p = mix_plan((unsigned)ctr[0], (unsigned)ctr[1] + (unsigned)i, B, H, W, m);
  float* o = out + 8 * (long long)i;
  o[0] = (float)p.mode; o[1] = (float)p.r; o[2] = p.lam;
  o[3] = (float)p.x0; o[4] = (float)p.y0; o[5] = (float)p.x1; o[6] = (float)p.y1;
  o[7] = (float)p.applied;
}

static bool mix_cfg_ok(const MixCfg& m) {
  return m.mixup_alpha >= 0.f && m.cutmix_alpha >= 0.f && m.mixup_alpha < INFINITY && m.cutmix_alpha < INFINITY &&
         m.mix_prob >= 0.f && m.mix_prob <= 1.f && m.switch_prob >= 0.f && m.switch_prob <= 1.f;
}

// ---- RandomResizedCrop / Resize + CenterCrop -------------------------------------------------
// The source is stored at one size [N][Hs][Ws][C] and the network is fed another [B][Ho][Wo][CP].
// A sample's view is an integer source box (i, j, h, w), a resized size (Rh, Rw), an integer
// window offset (oy, ox) into the resized image and a flip flag: output pixel (y, x) is resized
// pixel (y + oy, xf + ox), xf = Wo - 1 - x under a flip.  Train: the box and the flip are the
// sample's RandomResizedCrop plan below, (Rh, Rw) = (Ho, Wo), offset 0.  Eval: the box is the
// whole image and (Rh, Rw, oy, ox) come from the host (Resize + CenterCrop); nothing random.
//
// The filter is torch's antialiased bilinear one (F.interpolate(mode="bilinear", antialias=True,
// align_corners=False), which is PIL's), applied to the box: taps are clamped to the box and the
// weights renormalised there ("crop, then resize").  Per axis, n_in box pixels to n_out:
//   scale = n_in / n_out, support = max(scale, 1), centre(o) = scale * (o + 0.5),
//   lo = max(int(centre - support + 0.5), 0), hi = min(int(centre + support + 0.5), n_in),
//   w(k) = max(0, 1 - |(k - centre + 0.5) / support|) for k in [lo, hi), divided by their sum.
// The raw 0 .. 255 values are resampled in fp32, then normalised as sample_pixel does, then
// stored once as bf16: no rounding to uint8 in between (PIL rounds there).
struct RrcCfg { float s0, s1, r0, r1; };
struct View { int i, j, h, w, flip, fallback; };

// The plan's draws are hash3(hash3(seed ^ RRC_SALT, step, sample), k, RRC_SALT): apart from the
// crop / flip draws hash3(seed, step, sample) and from the mix plan's hash3(seed ^ MIX_SALT, ..).
constexpr unsigned RRC_SALT = 0x52524331u;
constexpr int RRC_TRIES = 10;
// draw indices: four per try, then the flip
enum { RRC_K_AREA = 0, RRC_K_RATIO = 1, RRC_K_I = 2, RRC_K_J = 3, RRC_K_FLIP = 4 * RRC_TRIES };

__device__ __forceinline__ unsigned rrc_bits(unsigned base, unsigned k) { return hash3(base, k, RRC_SALT); }
__device__ __forceinline__ float rrc_u01(unsigned base, unsigned k) {
  return ((float)(rrc_bits(base, k) >> 9) + 0.5f) * (1.f / 8388608.f);
}

// torchvision's RandomResizedCrop.get_params as a function of (seed, step, sample) and the
// parameters alone: not of the batch row, the batch size or the grid.
__device__ View rrc_plan(unsigned seed, unsigned step, unsigned sidx, int Hs, int Ws, const RrcCfg& c, int flip) {
  const unsigned base = hash3(seed ^ RRC_SALT, step, sidx);
  View v;
  v.flip = flip ? (int)((rrc_bits(base, RRC_K_FLIP) >> 24) & 1) : 0;
  v.fallback = 0;
  const float full = (float)Hs * (float)Ws, lr0 = __logf(c.r0), lr1 = __logf(c.r1);
  for (int t = 0; t < RRC_TRIES; ++t) {
    const float area = full * fmaf(c.s1 - c.s0, rrc_u01(base, 4 * t + RRC_K_AREA), c.s0);
    const float ratio = __expf(fmaf(lr1 - lr0, rrc_u01(base, 4 * t + RRC_K_RATIO), lr0));
    const float wf = rintf(sqrtf(area * ratio)), hf = rintf(sqrtf(area / ratio));
    if (wf >= 1.f && wf <= (float)Ws && hf >= 1.f && hf <= (float)Hs) {   // false for NaN too
      v.w = (int)wf; v.h = (int)hf;
      v.i = (int)(rrc_bits(base, 4 * t + RRC_K_I) % (unsigned)(Hs - v.h + 1));
      v.j = (int)(rrc_bits(base, 4 * t + RRC_K_J) % (unsigned)(Ws - v.w + 1));
      return v;
    }
  }
  // central crop at the nearest allowed aspect ratio
  const float in_ratio = (float)Ws / (float)Hs;
  v.fallback = 1;
  v.w = Ws; v.h = Hs;
  if (in_ratio < c.r0) v.h = (int)rintf((float)Ws / c.r0);
  else if (in_ratio > c.r1) v.w = (int)rintf((float)Hs * c.r1);
  v.h = min(max(v.h, 1), Hs); v.w = min(max(v.w, 1), Ws);   // the box stays inside whatever the rounding
  v.i = (Hs - v.h) / 2; v.j = (Ws - v.w) / 2;
  return v;
}

struct RsArgs {
  const unsigned char* src;  // [N][Hs][Ws][C] uint8
  const long long* labels_src;
  bf16_t* dst;               // [B][Ho][Wo][CP]
  long long* labels_dst;
  const float* ctr;          // device [seed, step, start]
  int N, Hs, Ws, CP, B, Ho, Wo;
  int train, flip;
  int Rh, Rw, oy, ox;        // train: (Ho, Wo, 0, 0)
  RrcCfg rrc;
  float mean[4], inv_std[4];
};

// A block owns one sample and a tile of RS_TH output rows x RS_TW output columns; the tap range
// and the weight parameters of every row and column of the tile are worked out once per block.
constexpr int RS_TH = 16, RS_TW = 256, RS_THREADS = 256;
// taps lo .. lo + n - 1 of the box; weight(k) = max(0, 1 - |k - c| / support) * inv, c = centre - 0.5
struct Taps { int lo, n; float c, inv; };
// a sample's view with the inverse filter supports of its two axes
struct RsView { View v; float isx, isy; };

__device__ __forceinline__ float tap_w(int k, float c, float isup) {
  return fmaxf(0.f, 1.f - fabsf(((float)k - c) * isup));
}

// output coordinate o (of n_out) over n_in box pixels
__device__ __forceinline__ Taps make_taps(int o, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out, support = fmaxf(scale, 1.f), isup = 1.f / support;
  const float centre = scale * ((float)o + 0.5f);
  Taps t;
  t.lo = max((int)(centre - support + 0.5f), 0);
  const int hi = min((int)(centre + support + 0.5f), n_in);
  t.n = hi - t.lo;
  t.c = centre - 0.5f;
  float s = 0.f;
  for (int k = t.lo; k < hi; ++k) s += tap_w(k, t.c, isup);
  t.inv = 1.f / s;           // the tap nearest the centre weighs more than 1/2: s > 0
  return t;
}

// normalised channels v[0 .. C) of one output pixel: the direct gather over its ty.n x tx.n taps
template <int C>
__device__ __forceinline__ void resample_pixel(const RsArgs& a, const unsigned char* img, const RsView& rv,
                                               const Taps tx, const Taps ty, float* v) {
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  const long long pitch = (long long)a.Ws * C;
  const unsigned char* row = img + (long long)(rv.v.i + ty.lo) * pitch + (long long)(rv.v.j + tx.lo) * C;
  for (int ky = 0; ky < ty.n; ++ky, row += pitch) {
    float r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = 0.f;
    for (int kx = 0; kx < tx.n; ++kx) {
      const float wx = tap_w(tx.lo + kx, tx.c, rv.isx);
#pragma unroll
      for (int c = 0; c < C; ++c) r[c] = fmaf(wx, (float)row[kx * C + c], r[c]);
    }
    const float wy = tap_w(ty.lo + ky, ty.c, rv.isy);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(wy, r[c], acc[c]);
  }
  const float nrm = tx.inv * ty.inv;
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = ((acc[c] * nrm) * (1.f / 255.f) - a.mean[c]) * a.inv_std[c];
}

// One thread per output pixel of the tile (one 16-byte store at CP == 8).  MIX: the step's mix
// plan over the output size, with k_augment_mix's semantics: CutMix takes the partner's pixel
// (under the partner's own box and flip) at the same output coordinate inside the box, mixup
// blends the two pixels as they would be stored; the thread of pixel (0, 0) writes the labels or
// the packed targets.
template <int C, bool MIX>
__global__ void __launch_bounds__(RS_THREADS) k_augment_resample(RsArgs a, float* __restrict__ targets, MixCfg m) {
  __shared__ RsView views[2];
  __shared__ MixPlan plan;
  __shared__ Taps tx[2][RS_TW], ty[2][RS_TH];
  const unsigned seed = (unsigned)a.ctr[0], step = (unsigned)a.ctr[1];
  const long long start = (long long)a.ctr[2];
  const int ntx = (a.Wo + RS_TW - 1) / RS_TW, nty = (a.Ho + RS_TH - 1) / RS_TH;
  const int b = (int)(blockIdx.x / (unsigned)(ntx * nty));
  const int tile = (int)(blockIdx.x % (unsigned)(ntx * nty));
  const int x0 = (tile % ntx) * RS_TW, y0 = (tile / ntx) * RS_TH;
  const int cols = min(RS_TW, a.Wo - x0), rows = min(RS_TH, a.Ho - y0);
  // start % N + batch row < 2^32
  const unsigned s0 = (unsigned)(start % a.N);
  const unsigned sidx = (s0 + (unsigned)b) % (unsigned)a.N;
  unsigned pidx = sidx;
  if (MIX) {
    if (threadIdx.x == 0) plan = mix_plan(seed, step, a.B, a.Ho, a.Wo, m);
    __syncthreads();
    const int r = plan.r;
    const int pb = b + r < a.B ? b + r : b + r - a.B;   // r < B
    pidx = (s0 + (unsigned)pb) % (unsigned)a.N;
  }
  const int nset = MIX && plan.mode != MIX_NONE ? 2 : 1;
  if ((int)threadIdx.x < nset) {
    View v = {0, 0, a.Hs, a.Ws, 0, 0};
    if (a.train) v = rrc_plan(seed, step, threadIdx.x ? pidx : sidx, a.Hs, a.Ws, a.rrc, a.flip);
    RsView rv;
    rv.v = v;
    rv.isx = 1.f / fmaxf((float)v.w / (float)a.Rw, 1.f);
    rv.isy = 1.f / fmaxf((float)v.h / (float)a.Rh, 1.f);
    views[threadIdx.x] = rv;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nset * (cols + rows); e += RS_THREADS) {
    const int set = e / (cols + rows), l = e - set * (cols + rows);
    const View v = views[set].v;
    if (l < cols) {
      const int x = x0 + l;
      tx[set][l] = make_taps((v.flip ? a.Wo - 1 - x : x) + a.ox, v.w, a.Rw);
    } else {
      ty[set][l - cols] = make_taps(y0 + l - cols + a.oy, v.h, a.Rh);
    }
  }
  __syncthreads();
  const MixPlan p = MIX ? plan : MixPlan{MIX_NONE, 0, 1.f, 0, 0, 0, 0, 0};
  const long long img_bytes = (long long)a.Hs * a.Ws * C;
  const unsigned char* own = a.src + sidx * img_bytes;
  const unsigned char* partner = a.src + pidx * img_bytes;
  for (int t = threadIdx.x; t < rows * cols; t += RS_THREADS) {
    const int ly = t / cols, lx = t - ly * cols;
    const int x = x0 + lx, y = y0 + ly;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int set = MIX && p.mode == MIX_CUTMIX && x >= p.x0 && x < p.x1 && y >= p.y0 && y < p.y1 ? 1 : 0;
    resample_pixel<C>(a, set ? partner : own, views[set], tx[set][lx], ty[set][ly], v);
    if (MIX && p.mode == MIX_MIXUP) {
      float w[4] = {0, 0, 0, 0};
      resample_pixel<C>(a, partner, views[1], tx[1][lx], ty[1][ly], w);
      // the two pixels as the plain launch would store them (bf16), as in k_augment_mix
      const unsigned a2[2] = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
      const unsigned b2[2] = {pack_bf2(w[0], w[1]), pack_bf2(w[2], w[3])};
      const float om = 1.f - p.lam;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        v[2 * c] = fmaf(p.lam, lo_bf(a2[c]), om * lo_bf(b2[c]));
        v[2 * c + 1] = fmaf(p.lam, hi_bf(a2[c]), om * hi_bf(b2[c]));
      }
    }
    store_pixel(a.dst + (((long long)b * a.Ho + y) * a.Wo + x) * a.CP, a.CP, v);
  }
  if (tile == 0 && threadIdx.x == 0) {
    if (MIX) {
      float* tg = targets + 3 * (long long)b;
      tg[0] = (float)a.labels_src[sidx];
      tg[1] = (float)a.labels_src[pidx];
      tg[2] = p.lam;
    } else if (a.labels_dst) {
      a.labels_dst[b] = a.labels_src[sidx];
    }
  }
}

// plans of steps ctr[1] .. ctr[1] + n - 1 for the samples (ctr[2] + b) % N of batch rows b < B,
// as rows (i, j, h, w, flip, fallback)
__global__ void k_rrc_plan(const float* __restrict__ ctr, float* __restrict__ out, int n, int B, int N, int Hs,
                           int Ws, RrcCfg c, int flip) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * B) return;
  const int i = t / B, b = t - i * B;
  const unsigned sidx = ((unsigned)((long long)ctr[2] % N) + (unsigned)b) % (unsigned)N;
  const View v = rrc_plan((unsigned)ctr[0], (unsigned)ctr[1] + (unsigned)i, sidx, Hs, Ws, c, flip);
  float* o = out + 6 * (long long)t;
  o[0] = (float)v.i; o[1] = (float)v.j; o[2] = (float)v.h; o[3] = (float)v.w;
  o[4] = (float)v.flip; o[5] = (float)v.fallback;
}

static bool rrc_cfg_ok(const RrcCfg& c) {
  return c.s0 > 0.f && c.s0 <= c.s1 && c.s1 < INFINITY && c.r0 > 0.f && c.r0 <= c.r1 && c.r1 < INFINITY;
}

}  // namespace

static AugArgs aug_args(const unsigned char* src, const long long* labels_src, bf16_t* dst, long long* labels_dst,
                        const float* ctr, int N, int H, int W, int C, int CP, int B, int pad, int flip, int train,
                        const float* mean, const float* std) {
  AugArgs a;
  a.src = src; a.labels_src = labels_src; a.dst = dst; a.labels_dst = labels_dst; a.ctr = ctr;
  a.N = N; a.H = H; a.W = W; a.C = C; a.CP = CP; a.B = B; a.pad = pad; a.flip = flip; a.train = train;
  for (int i = 0; i < 4; ++i) {
    a.mean[i] = i < C ? mean[i] : 0.f;
    a.inv_std[i] = i < C ? 1.f / std[i] : 0.f;
  }
  return a;
}

KML_API int kml_augment(const unsigned char* src, const long long* labels_src, bf16_t* dst, long long* labels_dst,
                        const float* ctr, int N, int H, int W, int C, int CP, int B, int pad, int flip, int train,
                        const float* mean, const float* std, hipStream_t s) {
  if (C > 4 || CP < C) return (int)hipErrorInvalidValue;
  const AugArgs a = aug_args(src, labels_src, dst, labels_dst, ctr, N, H, W, C, CP, B, pad, flip, train, mean, std);
  long long total = (long long)B * H * W;
  hipLaunchKernelGGL(k_augment, dim3(kml_stream_grid(total, 256)), dim3(256), 0, s, a);
  KML_LAUNCH_CHECK();
}

// kml_augment with the step's mixup / CutMix plan; targets: fp32 [B, 3] rows (label, partner
// label, lam) for kml_ce_soft_*.  An alpha of 0 switches that mode off; mix_prob: probability that
// a step mixes at all; switch_prob: share of CutMix when both alphas are > 0.
KML_API int kml_augment_mix(const unsigned char* src, const long long* labels_src, bf16_t* dst, float* targets,
                            const float* ctr, int N, int H, int W, int C, int CP, int B, int pad, int flip, int train,
                            const float* mean, const float* std, float mixup_alpha, float cutmix_alpha,
                            float mix_prob, float switch_prob, hipStream_t s) {
  const MixCfg m = {mixup_alpha, cutmix_alpha, mix_prob, switch_prob};
  if (C < 1 || C > 4 || CP < C || N < 1 || B < 1 || H < 1 || W < 1 || pad < 0 || !labels_src || !targets ||
      !mix_cfg_ok(m))
    return (int)hipErrorInvalidValue;
  const AugArgs a = aug_args(src, labels_src, dst, nullptr, ctr, N, H, W, C, CP, B, pad, flip, train, mean, std);
  long long total = (long long)B * H * W;
  hipLaunchKernelGGL(k_augment_mix, dim3(kml_stream_grid(total, 256)), dim3(256), 0, s, a, targets, m);
  KML_LAUNCH_CHECK();
}

// out: fp32 [n, 8] rows (mode, r, lam, x0, y0, x1, y1, applied), the plans kml_augment_mix uses
// at steps ctr[1] .. ctr[1] + n - 1 for a batch of B images of H x W (tests, debugging)
KML_API int kml_mix_plan(const float* ctr, float* out, int n, int B, int H, int W, float mixup_alpha,
                         float cutmix_alpha, float mix_prob, float switch_prob, hipStream_t s) {
  const MixCfg m = {mixup_alpha, cutmix_alpha, mix_prob, switch_prob};
  if (n < 1 || B < 1 || H < 1 || W < 1 || !mix_cfg_ok(m)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mix_plan, dim3((n + 255) / 256), dim3(256), 0, s, ctr, out, n, B, H, W, m);
  KML_LAUNCH_CHECK();
}

// RandomResizedCrop (train) or Resize + CenterCrop (eval) of the samples (ctr[2] + b) % N into
// dst [B, Ho, Wo, CP], with flip, normalisation and the bf16 cast, in one launch.  Train: the
// crop scale range [s0, s1] and aspect-ratio range [r0, r1] of the plan; (Rh, Rw, oy, ox) are
// not read.  Eval: the whole image resized to (Rh, Rw), window (oy, ox).  targets != null with a
// mixup / CutMix alpha > 0 (train only) mixes as kml_augment_mix does and writes the packed
// targets; otherwise labels_dst gets the int64 labels.
KML_API int kml_augment_resample(const unsigned char* src, const long long* labels_src, bf16_t* dst,
                                 long long* labels_dst, float* targets, const float* ctr, int N, int Hs, int Ws,
                                 int C, int CP, int B, int Ho, int Wo, int train, int flip, float s0, float s1,
                                 float r0, float r1, int Rh, int Rw, int oy, int ox, const float* mean,
                                 const float* std, float mixup_alpha, float cutmix_alpha, float mix_prob,
                                 float switch_prob, hipStream_t s) {
  const MixCfg m = {mixup_alpha, cutmix_alpha, mix_prob, switch_prob};
  RsArgs a;
  a.rrc = {s0, s1, r0, r1};
  if (C < 1 || C > 4 || CP < C || N < 1 || B < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || !src || !labels_src ||
      !dst || !ctr || !mix_cfg_ok(m))
    return (int)hipErrorInvalidValue;
  if (train) {
    if (!rrc_cfg_ok(a.rrc)) return (int)hipErrorInvalidValue;
    Rh = Ho; Rw = Wo; oy = 0; ox = 0;
  } else if (Rh < 1 || Rw < 1 || oy < 0 || ox < 0 || oy > Rh - Ho || ox > Rw - Wo) {
    return (int)hipErrorInvalidValue;
  }
  const bool mix = train && targets && (mixup_alpha > 0.f || cutmix_alpha > 0.f);
  if (!mix && !labels_dst) return (int)hipErrorInvalidValue;
  const long long blocks = (long long)B * ((Ho + RS_TH - 1) / RS_TH) * ((Wo + RS_TW - 1) / RS_TW);
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  a.src = src; a.labels_src = labels_src; a.dst = dst; a.labels_dst = labels_dst; a.ctr = ctr;
  a.N = N; a.Hs = Hs; a.Ws = Ws; a.CP = CP; a.B = B; a.Ho = Ho; a.Wo = Wo; a.train = train; a.flip = flip;
  a.Rh = Rh; a.Rw = Rw; a.oy = oy; a.ox = ox;
  for (int i = 0; i < 4; ++i) {
    a.mean[i] = i < C ? mean[i] : 0.f;
    a.inv_std[i] = i < C ? 1.f / std[i] : 0.f;
  }
  const dim3 grid((unsigned)blocks), block(RS_THREADS);
#define KML_RS_LAUNCH(CC)                                                                             \
  case CC:                                                                                            \
    if (mix) hipLaunchKernelGGL((k_augment_resample<CC, true>), grid, block, 0, s, a, targets, m);    \
    else hipLaunchKernelGGL((k_augment_resample<CC, false>), grid, block, 0, s, a, targets, m);       \
    break;
  switch (C) {
    KML_RS_LAUNCH(1) KML_RS_LAUNCH(2) KML_RS_LAUNCH(3) KML_RS_LAUNCH(4)
  }
#undef KML_RS_LAUNCH
  KML_LAUNCH_CHECK();
}

// out: fp32 [n, B, 6] rows (i, j, h, w, flip, fallback): the boxes kml_augment_resample draws in
// train mode at steps ctr[1] .. ctr[1] + n - 1 for the samples (ctr[2] + b) % N, b < B, of an
// Hs x Ws source (tests, debugging)
KML_API int kml_rrc_plan(const float* ctr, float* out, int n, int B, int N, int Hs, int Ws, float s0, float s1,
                         float r0, float r1, int flip, hipStream_t s) {
  const RrcCfg c = {s0, s1, r0, r1};
  if (n < 1 || B < 1 || N < 1 || Hs < 1 || Ws < 1 || (long long)n * B > 0x7fffffffLL || !rrc_cfg_ok(c))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rrc_plan, dim3((n * B + 255) / 256), dim3(256), 0, s, ctr, out, n, B, N, Hs, Ws, c, flip);
  KML_LAUNCH_CHECK();
}

// advance the data-pipeline counters in place: ctr = [seed, step, start]
__global__ void k_advance(float* ctr, float batch, float n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    ctr[1] += 1.f;
    float s = ctr[2] + batch;
    if (s >= n) s -= n;
    ctr[2] = s;
  }
}

KML_API int kml_advance_counter(float* ctr, float batch, float n, hipStream_t s) {
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, s, ctr, batch, n);
  KML_LAUNCH_CHECK();
}
