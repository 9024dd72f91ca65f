// Whole-network eval-mode ResNet-20 inference for gfx950: one launch carries N images from uint8 pixels
// to logits (models/resnet.py with training=False).  The training forward (resnet.hip k_rn_fwd) is one
// launch per layer because train-mode BatchNorm needs every image's statistics before the next layer;
// in eval mode BatchNorm is a per-channel affine map of constants and no image depends on another, so
// ONE 256-thread workgroup takes an image through all 19 convs, the 9 residual adds and the head with
// the activations resident in LDS, and loops over images b = blockIdx.x, + gridDim.x, ...  There is
// no communication between workgroups; the only synchronisation is one __syncthreads() per layer.
//
// LDS (103,104 B, one workgroup per CU):
//   r0, r1  36,992 B each   the largest zero-padded image, stage 1: [34][34][16] bf16
//   r2      20,736 B        a stage-2 image [18][18][32]; also the stem input [34][34][8] (18,496 B)
//   tb      [2][688] fp32   BN scale / shift of all 19 layers, built once per workgroup from the fp32
//                           master and state buffers: sc = gamma * rsqrt(mv + eps), sh = beta - mm * sc
//   fcw     [656] fp32      fc weights [64][10] + bias [10];   pooled [64] fp32
// Every image is stored with a halo of 1 on all sides; a stride-2 conv reads it at offset (+1, +1), which
// is TF-SAME's (0, 1) padding.  Roles (X block input, Y a-conv output), per image:
//   stem            r2 -> r0
//   stage 1         a: r0 -> r1      b: r1 (+ r0) -> r0, in place: a lane reads and writes the same element
//   stage 2 block 0 a: r0 -> r2      b: r2 (+ option A of r0) -> r1
//   stage 2         a: r1 -> r2      b: r2 (+ r1) -> r1
//   stage 3 block 0 a: r1 -> r2      b: r2 (+ option A of r1) -> r0
//   stage 3         a: r0 -> r2      b: r2 (+ r0) -> r0;  the last b-conv pools its fp32 outputs instead
// A layer only writes the interior of its output, so the halo of a region is zeroed whenever the region
// takes a new geometry (zero_halo: at the start of the layer that writes it, and of r0 / r1 per image).
//
// Math: the implicit GEMM of k_rn_fwd (MFMA 16x16x32 bf16, K order (tap, channel), one 16-B LDS read
// per B fragment, stem channels padded to 8); A fragments come from the engine's forward shadows, and
// the NEXT layer's fragments are requested before the current layer's epilogue so their L2 latency
// hides under it.  BN scale / shift, the shortcut and ReLU are applied to the fp32 accumulators;
// activations are rounded to bf16 only when stored as the next layer's operand.
#include "rn_conv_core.h"

namespace dmlc {
namespace rn {

constexpr int INF_CH = 688;                               // BN channels of all layers: 7*16 + 6*32 + 6*64
constexpr size_t INF_RBIG = 34 * 34 * 16 * 2, INF_RSML = 18 * 18 * 32 * 2;
constexpr size_t INF_LDS = 2 * INF_RBIG + INF_RSML + (2 * INF_CH + 656 + 64) * 4;
__host__ __device__ constexpr int inf_cout(int l) { return l < 7 ? 16 : (l < 13 ? 32 : 64); }
__host__ __device__ constexpr int inf_tb(int l) {       // layer l's first row of the table
  return l < 7 ? 16 * l : (l < 13 ? 112 + 32 * (l - 7) : 304 + 64 * (l - 13));
}

// geometry of one conv over pad-1 LDS images: input [HPI][HPI][CINP], output [HPO][HPO][COUT]
template <int CIN_, int COUT_, int HIN_, int S_>
struct Inf {
  static constexpr int CIN = CIN_, COUT = COUT_, HIN = HIN_, S = S_;
  static constexpr int CINP = CIN < 8 ? 8 : CIN, HOUT = HIN / S, HPI = HIN + 2, HPO = HOUT + 2;
  static constexpr int OFF = S == 1 ? 0 : 1;              // tap 0 of output pixel 0 on the padded input
  static constexpr int KP = round32(9 * CINP), KS = KP / 32;
  static constexpr int CT = COUT / 16, WPC = 4 / CT, NPT = HOUT * HOUT / 16 / WPC;
};

// the wave's rows of the forward shadow [COUT][KP], all k-steps
template <class L>
DEV void inf_wfrags(const void* wf, int w, int g, int li, bf16x8 (&wa)[L::KS]) {
  const bf16* W = reinterpret_cast<const bf16*>(wf) + (16 * (w % L::CT) + li) * L::KP + 8 * g;
#pragma unroll
  for (int ks = 0; ks < L::KS; ++ks) wa[ks] = glb_b128(W + 32 * ks);
}

// zero the border pixels of a padded [HP][HP][C] image
template <int HP, int C>
DEV void zero_halo(bf16* img, int tid) {
  constexpr int C8 = C / 8, NBP = 4 * HP - 4;
  for (int e = tid; e < NBP * C8; e += RT) {
    const int pb = e / C8, c8 = e - pb * C8;
    int y, x;
    if (pb < HP) { y = 0; x = pb; }
    else if (pb < 2 * HP) { y = HP - 1; x = pb - HP; }
    else { const int q = pb - 2 * HP; y = 1 + (q >> 1); x = (q & 1) ? HP - 1 : 0; }
    reinterpret_cast<uint4*>(img)[(y * HP + x) * C8 + c8] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// One conv + BN (+ shortcut) + ReLU, LDS to LDS.  SC: 0 none (stem, a-convs), 1 identity shortcut from
// scp (same geometry as the output; scp may be the output itself), 2 option A from the previous stage's
// block input scp [2*HOUT + 2][..][COUT / 2]: x[2y][2x][c] for c < COUT / 2, zero above.  ZH: the output
// region takes a new geometry.  LAST: no output image; the 8x8 mean of every channel goes to pooled[].
// wn: the next layer's (N) weight fragments, requested before the epilogue.
template <class L, class N, int SC, bool ZH, bool LAST = false>
DEV void inf_layer(const bf16* in, bf16* out, const bf16* scp, const float* tb, const bf16x8 (&wa)[L::KS],
                   bf16x8 (&wn)[N::KS], const void* wnext, float* pooled, int tid, int w, int g, int li) {
  constexpr int CINP = L::CINP, COUT = L::COUT, HOUT = L::HOUT, HPI = L::HPI, HPO = L::HPO, S = L::S;
  static_assert(!LAST || L::WPC == 1, "the pooled layer: a wave holds every pixel of its channels");
  if constexpr (ZH) zero_halo<HPO, COUT>(out, tid);
  const int ct = w % L::CT, pt0 = w / L::CT;
  f32x4 acc[L::NPT];
#pragma unroll
  for (int i = 0; i < L::NPT; ++i) acc[i] = zero4();
#pragma unroll
  for (int i = 0; i < L::NPT; ++i) {
    const int px = 16 * (pt0 + L::WPC * i) + li;
    const int oy = px / HOUT, ox = px - oy * HOUT;
    const int base = (oy * S + L::OFF) * HPI + ox * S + L::OFF;
#pragma unroll
    for (int ks = 0; ks < L::KS; ++ks) {
      const int k0 = 32 * ks + 8 * g;
      const int tap = min(k0 / CINP, 8), ci0 = k0 % CINP;   // taps past 8: K padding (zero weights)
      const int kh = tap / 3, kw = tap - 3 * kh;
      acc[i] = mfma16(wa[ks], lds_b128(in + (base + kh * HPI + kw) * CINP + ci0), acc[i]);
    }
  }
  inf_wfrags<N>(wnext, w, g, li, wn);
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue: rows co0 .. co0 + 3 of the wave's channel tile, one pixel per tile ----
  const int co0 = 16 * ct + 4 * g;
  const float4 sc = *reinterpret_cast<const float4*>(tb + co0);
  const float4 sh = *reinterpret_cast<const float4*>(tb + INF_CH + co0);
  [[maybe_unused]] float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < L::NPT; ++i) {
    const int px = 16 * (pt0 + L::WPC * i) + li;
    const int oy = px / HOUT, ox = px - oy * HOUT;
    const int po = ((oy + 1) * HPO + ox + 1) * COUT + co0;
    float v[4] = {acc[i][0] * sc.x + sh.x, acc[i][1] * sc.y + sh.y, acc[i][2] * sc.z + sh.z, acc[i][3] * sc.w + sh.w};
    uint2 s = make_uint2(0u, 0u);
    if constexpr (SC == 1) s = *reinterpret_cast<const uint2*>(scp + po);
    if constexpr (SC == 2) {
      if (ct < L::CT / 2)                                   // wave-uniform: the lower half of the channels
        s = *reinterpret_cast<const uint2*>(scp + ((2 * oy + 1) * (2 * HOUT + 2) + 2 * ox + 1) * (COUT / 2) + co0);
    }
    if constexpr (SC != 0) { v[0] += bf16_lo(s.x); v[1] += bf16_hi(s.x); v[2] += bf16_lo(s.y); v[3] += bf16_hi(s.y); }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
    if constexpr (LAST) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ps[r] += v[r];
    } else {
      *reinterpret_cast<bf16x4*>(out + po) = pack4(v[0], v[1], v[2], v[3]);
    }
  }
  if constexpr (LAST) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) ps[r] += __shfl_xor(ps[r], o);
      if (li == 0) pooled[co0 + r] = ps[r] * (1.f / (HOUT * HOUT));
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(RT) void k_rn_infer(DmlcRnInferArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* r0 = reinterpret_cast<bf16*>(smem);
  bf16* r1 = reinterpret_cast<bf16*>(smem + INF_RBIG);
  bf16* r2 = reinterpret_cast<bf16*>(smem + 2 * INF_RBIG);
  float* tb = reinterpret_cast<float*>(smem + 2 * INF_RBIG + INF_RSML);   // [2][688] scale | shift
  float* fcw = tb + 2 * INF_CH;                                            // [640] weights + [10] bias
  float* pooled = fcw + 656;                                               // [64]
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), g = lane >> 4, li = lane & 15;

  using LS = Inf<3, 16, 32, 1>;      // stem
  using L1 = Inf<16, 16, 32, 1>;     // stage 1
  using D2 = Inf<16, 32, 32, 2>;     // stage 2, first a-conv
  using L2 = Inf<32, 32, 16, 1>;
  using D3 = Inf<32, 64, 16, 2>;     // stage 3, first a-conv
  using L3 = Inf<64, 64, 8, 1>;

  bf16x8 f0[LS::KS];
  inf_wfrags<LS>(a.wf[0], w, g, li, f0);

  // ---- once per workgroup: BN scale / shift of every layer, the fc weights (all loads unpredicated:
  // a thread past the layer's channels reads the last one and stores nothing) ----
#pragma unroll
  for (int l = 0; l < DMLC_RN_LAYERS; ++l) {
    const int co = inf_cout(l), c = min(tid, co - 1);
    const float gam = a.master[a.gamma_off[l] + c], bet = a.master[a.beta_off[l] + c];
    const float mm = a.state[a.mm_off[l] + c], mv = a.state[a.mv_off[l] + c];
    const float sc = gam * (1.f / sqrtf(mv + (float)BN_EPS));
    if (tid < co) { tb[inf_tb(l) + tid] = sc; tb[INF_CH + inf_tb(l) + tid] = bet - mm * sc; }
  }
  for (int e = tid; e < 650; e += RT) fcw[e] = e < 640 ? a.master[a.fcw_off + e] : a.master[a.fcb_off + e - 640];

  for (int b = blockIdx.x; b < a.N; b += gridDim.x) {
    const int row = min(max(a.idx ? a.idx[b] : b, 0), a.nrows - 1);
    const uint8_t* img = a.data + (size_t)row * 3072;
    // r2 was last read by the previous image's final conv, r0 / r1 before that (each behind a barrier)
    stage_stem<LS::HPI * LS::HPI, LS::HPI, 1, 32>(r2, 0, 0, tid, [&](int e, int& e1) { e1 = e; return img; });
    zero_halo<34, 16>(r0, tid);
    zero_halo<34, 16>(r1, tid);
    __syncthreads();

    bf16x8 f1[L1::KS], f2[L1::KS], f3[L1::KS], f4[L1::KS], f5[L1::KS], f6[L1::KS], f7[D2::KS];
    bf16x8 f8[L2::KS], f9[L2::KS], f10[L2::KS], f11[L2::KS], f12[L2::KS], f13[D3::KS];
    bf16x8 f14[L3::KS], f15[L3::KS], f16[L3::KS], f17[L3::KS], f18[L3::KS];
#define INF_ARGS(l, f, fn) tb + inf_tb(l), f, fn, a.wf[(l + 1) % DMLC_RN_LAYERS], pooled, tid, w, g, li
    inf_layer<LS, L1, 0, false>(r2, r0, nullptr, INF_ARGS(0, f0, f1));
    inf_layer<L1, L1, 0, false>(r0, r1, nullptr, INF_ARGS(1, f1, f2));
    inf_layer<L1, L1, 1, false>(r1, r0, r0, INF_ARGS(2, f2, f3));
    inf_layer<L1, L1, 0, false>(r0, r1, nullptr, INF_ARGS(3, f3, f4));
    inf_layer<L1, L1, 1, false>(r1, r0, r0, INF_ARGS(4, f4, f5));
    inf_layer<L1, L1, 0, false>(r0, r1, nullptr, INF_ARGS(5, f5, f6));
    inf_layer<L1, D2, 1, false>(r1, r0, r0, INF_ARGS(6, f6, f7));
    inf_layer<D2, L2, 0, true>(r0, r2, nullptr, INF_ARGS(7, f7, f8));
    inf_layer<L2, L2, 2, true>(r2, r1, r0, INF_ARGS(8, f8, f9));
    inf_layer<L2, L2, 0, false>(r1, r2, nullptr, INF_ARGS(9, f9, f10));
    inf_layer<L2, L2, 1, false>(r2, r1, r1, INF_ARGS(10, f10, f11));
    inf_layer<L2, L2, 0, false>(r1, r2, nullptr, INF_ARGS(11, f11, f12));
    inf_layer<L2, D3, 1, false>(r2, r1, r1, INF_ARGS(12, f12, f13));
    inf_layer<D3, L3, 0, true>(r1, r2, nullptr, INF_ARGS(13, f13, f14));
    inf_layer<L3, L3, 2, true>(r2, r0, r1, INF_ARGS(14, f14, f15));
    inf_layer<L3, L3, 0, false>(r0, r2, nullptr, INF_ARGS(15, f15, f16));
    inf_layer<L3, L3, 1, false>(r2, r0, r0, INF_ARGS(16, f16, f17));
    inf_layer<L3, L3, 0, false>(r0, r2, nullptr, INF_ARGS(17, f17, f18));
    inf_layer<L3, LS, 1, false, true>(r2, nullptr, r0, INF_ARGS(18, f18, f0));   // f0: the next image's stem
#undef INF_ARGS

    // ---- head (wave 0): fc 64 -> 10 in fp32, first maximum.  pooled[] is next written 19 barriers on.
    if (w == 0) {
      float lg = 0.f;
      if (lane < 10) {
        lg = fcw[640 + lane];
        for (int k = 0; k < 64; ++k) lg += pooled[k] * fcw[k * 10 + lane];
      }
      float m = lane < 10 ? lg : -INFINITY;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      int am = lane < 10 && lg == m ? lane : 64;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o));
      if (lane < 10) a.logits[(size_t)b * 10 + lane] = lg;
      if (lane == 0) {
        if (a.pred) a.pred[b] = am;
        if (a.correct) a.correct[b] = am == a.labels[row] ? 1 : 0;
      }
    }
  }
}

}  // namespace rn
}  // namespace dmlc

extern "C" hipError_t dmlc_rn_infer(const DmlcRnInferArgs* a, hipStream_t s) {
  using namespace dmlc;
  using namespace dmlc::rn;
  if (a->N < 1 || a->nrows < 1 || a->blocks < 0 || (a->correct && !a->labels)) return hipErrorInvalidValue;
  int blocks = a->blocks;
  if (blocks == 0) {                     // what the LDS footprint allows per CU, on every CU
    int dev = 0, cus = 0, lds = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev);
    if (e != hipSuccess) return e;
    const int per_cu = lds / (int)INF_LDS > 1 ? lds / (int)INF_LDS : 1;
    blocks = (cus > 0 ? cus : 1) * per_cu;
  }
  blocks = blocks < a->N ? blocks : a->N;
  DMLC_LDS_OPTIN(&k_rn_infer, INF_LDS);
  hipLaunchKernelGGL(k_rn_infer, dim3(blocks), dim3(RT), INF_LDS, s, *a);
  return hipGetLastError();
}
