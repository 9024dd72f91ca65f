// SGD of the fused ResNet-20 step (see resnet.hip): slab reduction, parameter and BN running-statistics
// update, bf16 weight shadows and the device step counter in one launch.
#include "rn_stats.h"

namespace dmlc {
namespace rn {

DEV float4 add4r(float4 x, float4 y) { return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w); }

// thread (sp = tid / O, idx = tid % O) sums slabs q = sp, sp+S, ...; the block folds the S splits
// in fixed order -> threads tid < O return the total of output idx (deterministic)
DEV float4 split_reduce(const float* p, size_t stride, int n, int S, float4* lds) {
  const int O = RT / S, sp = threadIdx.x / O, idx = threadIdx.x - sp * O;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int q = sp;
  for (; q + 7 * S < n; q += 8 * S) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(q + u * S) * stride);
#pragma unroll
    for (int u = 0; u < 8; ++u) s = add4r(s, v[u]);
  }
  for (; q < n; q += S) s = add4r(s, *reinterpret_cast<const float4*>(p + (size_t)q * stride));
  lds[threadIdx.x] = s;
  __syncthreads();
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (threadIdx.x < O)
    for (int k = 0; k < S; ++k) t = add4r(t, lds[k * O + idx]);
  return t;
}

// The parameter update of every applying site (conv, fc, BN gamma / beta).  plain (no velocity
// buffer, no weight decay): w - lr * g, the expression this kernel always had.  Otherwise
// v <- mu * v + (g + wd * w), w <- w - lr * v with the rounding pinned by explicit fmaf, so modes 0
// and 2 and every site round alike (g is materialised by the caller; wd = 0 for rank-1 parameters;
// without a velocity buffer mu is 0 and v comes in as 0)
DEV float sgd_update(float w, float g, float lr, float wd, float mu, float& v, bool plain) {
  if (plain) return w - lr * g;
  v = fmaf(mu, v, fmaf(wd, w, g));
  return fmaf(-lr, v, w);
}

// modes: 0 reduce slabs + apply (1 GPU); 1 reduce slabs into `grad` (DP, before the all-reduce);
//        2 apply grad_scale * `grad` (DP, after it); 3 refresh the bf16 shadows from the master only
// blocks: [conv layer 0..18 | fc | BN layer 0..18]
__global__ __launch_bounds__(RT) void k_rn_sgd(DmlcRnSgdArgs a) {
  __shared__ float4 lds[RT];
  __shared__ float lred[2][4];
  const int64_t step = *a.step_rd;
  const float lr0 = a.staircase ? a.lr0 * powf(a.decay, floorf((float)step / a.decay_steps)) : a.lr0;
  const float lr = a.warmup > 0.f && (float)step < a.warmup ? lr0 * ((float)step + 1.f) / a.warmup : lr0;
  const int mode = a.mode;
  const bool reduce = mode <= 1, apply = mode == 0 || mode == 2;
  const float mu = a.momentum, wdec = a.weight_decay;
  const bool plain = a.vel == nullptr && wdec == 0.f;     // the update without momentum / decay
  const int blk = blockIdx.x, tid = threadIdx.x;
  constexpr int NL = DMLC_RN_LAYERS;
  // (the BN blocks dispatched first instead of last measured no better: 612.0-612.9 vs 608.4-611.3
  // us/step, profiles/r6s3_rn_sgd_bn_first_ab.txt -- they are not the launch's tail)
  // block role: every range start compared at once (21 independent kernarg loads, one latency; the
  // search loop paid one dependent scalar load per range -- ~20 in a row for the BN blocks)
  int l = 0;
#pragma unroll
  for (int i = 1; i <= NL + 1; ++i) l += blk >= a.blk_start[i] ? 1 : 0;
  if (l < NL) {                                  // conv layer l
    const int S = a.split[l], O = RT / S;
    const int cin = a.cin[l], cout = a.cout[l], cinp = cin < 8 ? 8 : cin;
    const int kp = (9 * cinp + 31) / 32 * 32, kpd = (9 * cout + 31) / 32 * 32;
    const int n4 = 9 * cin * cout / 4, co4n = cout / 4;
    const int o4 = (blk - a.blk_start[l]) * O + tid % O;
    const bool valid = o4 < n4;
    const int oc = valid ? o4 : 0;
    const int row = oc / co4n, co = (oc - row * co4n) * 4;          // HWIO row = tap*cin + ci
    const int tap = row / cin, ci = row - tap * cin, k = tap * cinp + ci;
    const size_t off = (size_t)a.conv_off[l] + (size_t)row * cout + co;
    float4 gsum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (reduce) gsum = split_reduce(a.part[l] + (size_t)k * cout + co, (size_t)kp * cout, a.G[l], S, lds);
    if (tid < O && valid) {
      if (mode == 1) {
        *reinterpret_cast<float4*>(a.grad + off) = gsum;
      } else {
        if (mode == 2) {
          const float4 gv = *reinterpret_cast<const float4*>(a.grad + off);
          gsum = make_float4(gv.x * a.grad_scale, gv.y * a.grad_scale, gv.z * a.grad_scale, gv.w * a.grad_scale);
        }
        float* m = a.master + off;
        float4 wv = *reinterpret_cast<float4*>(m);
        if (apply) {
          float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
          if (a.vel) vv = *reinterpret_cast<const float4*>(a.vel + off);
          wv.x = sgd_update(wv.x, gsum.x, lr, wdec, mu, vv.x, plain);
          wv.y = sgd_update(wv.y, gsum.y, lr, wdec, mu, vv.y, plain);
          wv.z = sgd_update(wv.z, gsum.z, lr, wdec, mu, vv.z, plain);
          wv.w = sgd_update(wv.w, gsum.w, lr, wdec, mu, vv.w, plain);
          *reinterpret_cast<float4*>(m) = wv;
          if (a.vel) *reinterpret_cast<float4*>(a.vel + off) = vv;
        }
        bf16* wf = reinterpret_cast<bf16*>(a.wf[l]);
        wf[(co + 0) * kp + k] = (bf16)wv.x; wf[(co + 1) * kp + k] = (bf16)wv.y;
        wf[(co + 2) * kp + k] = (bf16)wv.z; wf[(co + 3) * kp + k] = (bf16)wv.w;
        if (a.wd[l])
          *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(a.wd[l]) + (size_t)ci * kpd + (8 - tap) * cout + co) =
              pack4(wv.x, wv.y, wv.z, wv.w);
      }
    }
  } else if (l == NL) {                          // fc: 164 float4 of [640 dW | 10 db | pad], split over images
    const int S = a.split[NL], O = RT / S;
    const int o4 = (blk - a.blk_start[l]) * O + tid % O;
    const bool valid = o4 < 164;
    float4 gsum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (reduce) gsum = split_reduce(a.fc_part + 4 * (valid ? o4 : 0), 656, a.B, S, lds);
    if (tid < O && valid && mode != 3) {
      const float gv[4] = {gsum.x, gsum.y, gsum.z, gsum.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = 4 * o4 + j;
        if (e < 650) {
          const size_t off = e < 640 ? (size_t)a.fcw_off + e : (size_t)a.fcb_off + e - 640;
          if (mode == 1) {
            a.grad[off] = gv[j];
          } else {                               // the weight matrix (e < 640) decays, the bias does not
            const float g = mode == 2 ? a.grad[off] * a.grad_scale : gv[j];
            float v = a.vel ? a.vel[off] : 0.f;
            a.master[off] = sgd_update(a.master[off], g, lr, e < 640 ? wdec : 0.f, mu, v, plain);
            if (a.vel) a.vel[off] = v;
          }
        }
      }
    }
  } else if (mode != 3 && a.tail) {               // BN layer L: gamma/beta + running statistics
    const int L = blk - a.blk_start[NL + 1];
    const int c = tid;
    // every load of this block first (gradient and statistics slots, master gamma / beta, running
    // statistics, layer 0: the per-image loss / accuracy), then the arithmetic and the stores: the
    // chain of dependent round trips made these 19 blocks the launch's tail
    const bool act = c < a.cout[L];
    const int cc = act ? c : 0;
    const size_t og = (size_t)a.gamma_off[L] + cc, ob = (size_t)a.beta_off[L] + cc;
    const long long* rp = a.red + (size_t)L * NSLOT * 256;
    const long long* sp = a.stat + (size_t)L * NSLOT * 256;
    // (fx_total issues its 16 loads before any arithmetic; the four totals are independent)
    const double r1 = fx_total(rp, cc), r2 = fx_total(rp, 64 + cc);
    const double s1 = fx_total(sp, cc), s2 = fx_total(sp, 64 + cc);
    float* mm = a.state + a.mm_off[L] + cc;
    float* mv = a.state + a.mv_off[L] + cc;
    // (a.grad exists only in the data-parallel modes 1/2; the running statistics are only updated
    // by the applying modes)
    float mg = 0.f, mb = 0.f, gg = 0.f, gb = 0.f, mmv = 0.f, mvv = 0.f, vg = 0.f, vb = 0.f;
    if (mode != 1) { mg = a.master[og]; mb = a.master[ob]; mmv = *mm; mvv = *mv; }
    if (mode != 1 && a.vel) { vg = a.vel[og]; vb = a.vel[ob]; }
    if (mode == 2) { gg = a.grad[og]; gb = a.grad[ob]; }
    float lsv = 0.f, csv = 0.f;
    if (L == 0 && apply)
      for (int q = tid; q < a.B; q += RT) { lsv += a.loss_img[q]; csv += (float)a.correct_img[q]; }
    if (act) {
      if (mode == 1) {
        a.grad[og] = (float)r2;
        a.grad[ob] = (float)r1;
      } else {
        a.master[og] = sgd_update(mg, mode == 2 ? gg * a.grad_scale : (float)r2, lr, 0.f, mu, vg, plain);   // rank 1:
        a.master[ob] = sgd_update(mb, mode == 2 ? gb * a.grad_scale : (float)r1, lr, 0.f, mu, vb, plain);   // no decay
        if (a.vel) { a.vel[og] = vg; a.vel[ob] = vb; }
        const double inv = (double)a.inv_n[L];
        const double mean = s1 * inv;
        double var = s2 * inv - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double nn = 1.0 / inv;
        const float m = a.bn_momentum;
        *mm = (1.f - m) * mmv + m * (float)mean;
        *mv = (1.f - m) * mvv + m * (float)(var * nn / (nn - 1.0));
      }
    }
    if (L == 0 && apply) {                       // batch loss / accuracy -> stats ring (fields 1, 2)
      float ls = lsv, cs = csv;
      ls = wave_sum(ls);
      cs = wave_sum(cs);
      if ((tid & 63) == 0) { lred[0][tid >> 6] = ls; lred[1][tid >> 6] = cs; }
      __syncthreads();
      if (tid == 0) {
        float* st = a.stats + (size_t)(step % a.stats_len) * 4;
        st[1] = (lred[0][0] + lred[0][1] + lred[0][2] + lred[0][3]) / (float)a.nvalid;
        st[2] = (lred[1][0] + lred[1][1] + lred[1][2] + lred[1][3]) / (float)a.nvalid;
        if (a.step_rd != a.step) {               // no block reads *a.step: publish + bump here
          st[0] = (float)(step + 1);
          st[3] = lr;
          *a.step = step + 1;
        }
      }
    }
  }
  if (!apply || !a.tail || a.step_rd != a.step) return;   // partial launch / ticketless: nothing more
  __syncthreads();
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (last_arrival(a.ticket, blockIdx.x, gridDim.x)) {   // last block: publish the step
      float* st = a.stats + (size_t)(step % a.stats_len) * 4;
      st[0] = (float)(step + 1);
      st[3] = lr;
      *a.step = step + 1;
    }
  }
}

}  // namespace rn
}  // namespace dmlc

using namespace dmlc::rn;

static int split_for(int n) {                 // slabs per thread <= 8
  int S = 4;
  while (S < 64 && S * 8 < n) S <<= 1;
  return S;
}

extern "C" hipError_t dmlc_rn_sgd(DmlcRnSgdArgs* a, hipStream_t s) {
  if (a->layer_lo < 0 || a->layer_hi > DMLC_RN_LAYERS || a->layer_lo > a->layer_hi) return hipErrorInvalidValue;
  if (!a->tail && (a->mode == 1 || a->mode == 2 || a->mode == 3)) return hipErrorInvalidValue;   // partial: mode 0
  if (a->momentum != 0.f && !a->vel && (a->mode == 0 || a->mode == 2)) return hipErrorInvalidValue;   // no velocity
  int blocks = 0;
  for (int l = 0; l < DMLC_RN_LAYERS; ++l) {      // layers outside the range get no blocks
    a->split[l] = split_for(a->G[l]);
    a->blk_start[l] = blocks;
    const int O = RT / a->split[l];
    if (l >= a->layer_lo && l < a->layer_hi) blocks += (9 * a->cin[l] * a->cout[l] / 4 + O - 1) / O;
  }
  a->split[DMLC_RN_LAYERS] = split_for(a->B);
  a->blk_start[DMLC_RN_LAYERS] = blocks;                     // fc
  if (a->tail) blocks += (164 + RT / a->split[DMLC_RN_LAYERS] - 1) / (RT / a->split[DMLC_RN_LAYERS]);
  a->blk_start[DMLC_RN_LAYERS + 1] = blocks;                 // BN, one block per layer
  if (a->tail) blocks += DMLC_RN_LAYERS;
  a->blk_start[DMLC_RN_LAYERS + 2] = blocks;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rn_sgd, dim3(blocks), dim3(RT), 0, s, *a);
  return hipGetLastError();
}
