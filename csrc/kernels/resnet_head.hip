// Head of the fused ResNet-20 step (see resnet.hip): the last BN-apply + residual, global average
// pool, fc 64x10, softmax cross-entropy and their backward down to g_y of layer 18, one launch.
#include "rn_stats.h"

namespace dmlc {
namespace rn {

// per image: a18 = relu(bn(z18) + x_in) -> mean pool -> fc 64x10 -> softmax-xent -> backward to g_y18
__global__ __launch_bounds__(RT) void k_rn_head(DmlcRnHeadArgs a) {
  if (a.step_copy && blockIdx.x == 0 && threadIdx.x == 0) *a.step_copy = *a.step;
  __shared__ float pool_part[4][64];
  __shared__ float pooled[64], dlog[16], gpool[64], cf[2][64];
  __shared__ float redl[2][4][64];
  __shared__ float fcw_s[650];                  // fc weight [64][10] + bias [10]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int c = lane;                           // thread -> channel c, pixels w, w+4, ... (16 each)
  // every small operand of the later phases is loaded at entry, beside the activations: the fc
  // weights / bias into LDS, gamma / beta into registers (each was one more exposed memory latency
  // on the serial chain pool -> logits -> dlogits -> pooled gradient)
  float fv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = tid + i * RT;                 // clamped addresses: every load in bounds
    const float wv = a.fcw[e < 640 ? e : 0], bv = a.fcb[e >= 640 && e < 650 ? e - 640 : 0];
    fv[i] = e < 640 ? wv : (e < 650 ? bv : 0.f);
  }
  const float gam = a.gamma[c], bet = a.beta[c];
  if (tid < 64) {
    float mean, rstd;
    bn_mean_rstd(a.stat, tid, a.inv_n, mean, rstd);
    cf[0][tid] = mean; cf[1][tid] = rstd;
  }
  const bf16* zp = reinterpret_cast<const bf16*>(a.z) + (size_t)b * 4096;
  const bf16* sp = reinterpret_cast<const bf16*>(a.sc) + (size_t)b * 4096;
  float zv[16], sv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int px = w + 4 * k;
    zv[k] = (float)zp[px * 64 + c];
    sv[k] = (float)sp[px * 64 + c];
  }
  int label = 0;
  if (tid == 0) label = a.labels[batch_index(a.src, a.B, b)];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = tid + i * RT;
    if (e < 650) fcw_s[e] = fv[i];
  }
  __syncthreads();
  const float mean = cf[0][c], rstd = cf[1][c];
  const float sc = gam * rstd, sh = bet - mean * sc;
  float av[16];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    av[k] = fmaxf(zv[k] * sc + sh + sv[k], 0.f);
    s += av[k];
  }
  pool_part[w][c] = s;
  __syncthreads();
  if (tid < 64) pooled[tid] = (pool_part[0][tid] + pool_part[1][tid] + pool_part[2][tid] + pool_part[3][tid]) * (1.f / 64.f);
  __syncthreads();
  if (tid < 64) {                               // wave 0: logits / softmax / dlogits
    float lg = 0.f;
    if (lane < 10) {
      lg = fcw_s[640 + lane];
      for (int k = 0; k < 64; ++k) lg += pooled[k] * fcw_s[k * 10 + lane];
    }
    const float lgm = lane < 10 ? lg : -INFINITY;
    float m = lgm;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float e = lane < 10 ? __expf(lg - m) : 0.f;
    float se = e;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    const int lab = __shfl(label, 0);
    int am = lane < 10 && lg == m ? lane : 64;  // first maximum (accuracy)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o));
    const float lse = m + __logf(se);
    const float lgl = __shfl(lg, lab);
    const bool real = b < a.nvalid;             // batch padding: no loss, accuracy or gradient
    if (lane == 0) { a.loss_img[b] = real ? lse - lgl : 0.f; a.correct_img[b] = real && am == lab ? 1 : 0; }
    if (lane < 10) {
      if (a.logits_out) a.logits_out[b * 10 + lane] = lg;
      dlog[lane] = real ? (e / se - (lane == lab ? 1.f : 0.f)) * a.inv_batch : 0.f;
    }
  }
  __syncthreads();
  if (tid < 64) {
    float gp = 0.f;
#pragma unroll
    for (int n = 0; n < 10; ++n) gp += fcw_s[tid * 10 + n] * dlog[n];
    gpool[tid] = gp * (1.f / 64.f);
    float* fp = a.fc_part + (size_t)b * 656;
#pragma unroll
    for (int n = 0; n < 10; ++n) fp[tid * 10 + n] = pooled[tid] * dlog[n];
    if (tid < 10) fp[640 + tid] = dlog[tid];
  }
  __syncthreads();
  const float gpc = gpool[c];
  bf16* gyo = reinterpret_cast<bf16*>(a.gy) + (size_t)b * 4096;
  float r1 = 0.f, r2 = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int px = w + 4 * k;
    const float gy = av[k] > 0.f ? gpc : 0.f;
    gyo[px * 64 + c] = (bf16)gy;
    r1 += gy;
    r2 += gy * (zv[k] - mean) * rstd;
  }
  redl[0][w][c] = r1;
  redl[1][w][c] = r2;
  __syncthreads();
  const float t1 = tid < 64 ? redl[0][0][tid] + redl[0][1][tid] + redl[0][2][tid] + redl[0][3][tid] : 0.f;
  const float t2 = tid < 64 ? redl[1][0][tid] + redl[1][1][tid] + redl[1][2][tid] + redl[1][3][tid] : 0.f;
  if (tid < 64) slot_flush(a.red, b, tid, t1, t2);
}

}  // namespace rn
}  // namespace dmlc

extern "C" hipError_t dmlc_rn_head(const DmlcRnHeadArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(dmlc::rn::k_rn_head, dim3(a->B), dim3(dmlc::rn::RT), 0, s, *a);
  return hipGetLastError();
}
