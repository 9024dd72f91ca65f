// BatchNorm statistics of the fused ResNet-20 kernels (resnet.hip, resnet_head.hip, resnet_sgd.hip):
// exact fixed-point channel sums in NSLOT slots per layer, the forward / backward BN coefficients
// rebuilt from them, and the block-level reduction that feeds them.
#pragma once
#include "conv_common.h"
#include "api_resnet.h"

namespace dmlc {
namespace rn {

constexpr int RT = 256;                       // threads per workgroup of every ResNet-20 kernel
constexpr int NSLOT = DMLC_RN_NSLOT;          // statistics copies per layer: [NSLOT][hi 128 | lo 128] int64
constexpr double BN_EPS = 1e-3;

// Fixed-point BN statistics.  A slot holds, per statistic e (0..63 sum / R1, 64..127 sum of squares /
// R2), an int64 integer part at [e] and a uint64 fraction in units of 2^-48 at [128 + e].  One add
// splits x = floor(x) + f exactly (|x| < 2^50, so x - floor(x) and f * 2^48 are exact in fp64) and
// rounds f * 2^48 to an integer (error <= 2^-49 per add, far below the fp32 partial's own rounding).
// A non-finite or absurd partial adds the poison 2^56 to the integer part; legitimate slot totals stay
// below 2^55 in magnitude (<= 32 adds of < 2^50 each at B = 256), so the decoder turns any slot at or
// beyond 2^55 into NaN -- a diverged step still shows up as NaN downstream.
constexpr double FX_ONE = 281474976710656.0;             // 2^48
constexpr double FX_LIM = 1125899906842624.0;            // 2^50
constexpr long long FX_POISON = 1LL << 56;
constexpr long long FX_BAD = 1LL << 55;

DEV void fx_add(long long* slot, int e, float v) {
  const double x = (double)v;
  long long hi;
  unsigned long long lo;
  if (__builtin_fabs(x) < FX_LIM) {
    const double f = __builtin_floor(x);
    hi = (long long)f;
    lo = (unsigned long long)__builtin_rint((x - f) * FX_ONE);   // in [0, 2^48]
  } else {
    hi = FX_POISON;
    lo = 0;
  }
  atomicAdd(reinterpret_cast<unsigned long long*>(slot + e), (unsigned long long)hi);
  atomicAdd(reinterpret_cast<unsigned long long*>(slot + 128 + e), lo);
}

// channel c's two block partials (sum / R1, sum of squares / R2) into block blk's slot of a layer
template <class I>
DEV void slot_flush(long long* dst, I blk, int c, float t1, float t2) {
  long long* d = dst + (blk & (NSLOT - 1)) * 256;
  fx_add(d, c, t1);
  fx_add(d, 64 + c, t2);
}

// total of statistic e over the NSLOT copies of one layer's slotted accumulator (all loads first)
DEV double fx_total(const long long* st, int e) {
  long long h[NSLOT];
  unsigned long long l[NSLOT];
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) {
    h[k] = st[k * 256 + e];
    l[k] = (unsigned long long)st[k * 256 + 128 + e];
  }
  long long hs = 0;
  unsigned long long ls = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) {
    hs += h[k];
    ls += l[k];
    bad |= h[k] >= FX_BAD || h[k] <= -FX_BAD;
  }
  return bad ? __builtin_nan("") : (double)hs + (double)ls * (1.0 / FX_ONE);
}

// channel c of a slotted accumulator: (sum, sum of squares) or (R1, R2)
DEV void slot_sums(const long long* st, int c, double& s1, double& s2) {
  s1 = fx_total(st, c);
  s2 = fx_total(st, 64 + c);
}

// (no FMA contraction in the coefficient math: the backend's -ffp-contract=fast choices depend on
// the surrounding kernel, and every kernel that rebuilds these coefficients must get the same bits)
DEV void bn_mean_rstd(const long long* stat, int c, float inv_n, float& mean, float& rstd) {
#pragma clang fp contract(off)
  double s1, s2;
  slot_sums(stat, c, s1, s2);
  const double m = s1 * (double)inv_n;
  double var = s2 * (double)inv_n - m * m;
  var = var > 0.0 ? var : 0.0;
  mean = (float)m;
  rstd = (float)(1.0 / sqrt(var + BN_EPS));
}

// BN backward: g_z = A*g_y + Bc*z + Cc  with  A = gamma*rstd, Bc = -gamma*rstd^2*R2/N, Cc = -A*R1/N - Bc*mean
DEV void bnb_coeffs(const long long* stat, const long long* red, const float* gamma, int c, float inv_n, float& A,
                    float& Bc, float& Cc) {
#pragma clang fp contract(off)
  float mean, rstd;
  bn_mean_rstd(stat, c, inv_n, mean, rstd);
  double r1, r2;
  slot_sums(red, c, r1, r2);
  A = gamma[c] * rstd;
  Bc = -A * rstd * (float)(r2 * (double)inv_n);
  Cc = -A * (float)(r1 * (double)inv_n) - Bc * mean;
}

// g_z = A*g_y + Bc*z + Cc with the rounding pinned (two explicit FMAs): the dgrad, the wgrad and the
// per-image backward each rebuild g_z from the same bf16 inputs and must agree bit for bit
DEV float bnb_apply(float A, float Bc, float Cc, float gy, float z) {
  return __builtin_fmaf(A, gy, __builtin_fmaf(Bc, z, Cc));
}

// block-level channel reduction of per-lane partials (lanes with equal li share a channel group), then
// one fixed-point add per statistic into this block's slot
template <int CT, int C>
DEV void reduce_flush(float (&s1)[4], float (&s2)[4], float* red, long long* dst, int w, int g, int li,
                      int tid) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { s1[r] += __shfl_xor(s1[r], o); s2[r] += __shfl_xor(s2[r], o); }
  const int ct = w % CT;
  if (li == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[(w * 2 + 0) * 64 + 16 * ct + 4 * g + r] = s1[r];
      red[(w * 2 + 1) * 64 + 16 * ct + 4 * g + r] = s2[r];
    }
  }
  __syncthreads();
  float t1 = 0.f, t2 = 0.f;
  if (tid < C) {
#pragma unroll
    for (int ww = 0; ww < 4; ++ww)
      if (ww % CT == tid / 16) { t1 += red[(ww * 2) * 64 + tid]; t2 += red[(ww * 2 + 1) * 64 + tid]; }
  }
  if (tid < C) slot_flush(dst, blockIdx.x, tid, t1, t2);
}

}  // namespace rn
}  // namespace dmlc
