// Fused ResNet-20 training kernels for gfx950 (BASELINE.json config 4; SURVEY.md §2.C "Extra kernels
// not in the reference": conv3x3 fwd/dgrad/wgrad with stride 1/2, train-mode batch-norm, residual add,
// global average pool).  Model: models/resnet.py (the eager oracle).
// This file: the conv kernels, their launchers and the shape dispatch.  rn_stats.h: the fixed-point
// statistics and BN coefficients; rn_conv_core.h: geometry and the phases the conv kernels share;
// resnet_head.hip: pool / fc / loss head; resnet_sgd.hip: the SGD kernel.
//
// Design (MI355X-first):
//   * every 3x3 conv is an implicit GEMM on MFMA 16x16x32 bf16 over an LDS image of ONE zero-padded
//     input (one image per 256-thread block for fwd/dgrad), no im2col buffer; the K order is
//     (tap, channel) so each 8-wide B fragment is one 16-byte LDS read (CIN padded to 8 for the stem);
//   * train-mode BatchNorm never gets its own kernel: a layer's forward kernel writes z and adds
//     per-block channel sums / sums of squares into fp64 accumulators; the NEXT conv applies
//     scale/shift + ReLU (+ the option-A residual) while staging its input (and materialises a for
//     the backward); the backward mirrors it: each dgrad's epilogue produces g_y of the layer below
//     plus its two BN reductions (sum g_y, sum g_y*xhat), and the consumer rebuilds
//     g_z = gamma*rstd*(g_y - R1/N - xhat*R2/N) in its prologue;
//   * the statistics are exact fixed-point sums: every block splits each fp32 channel partial into an
//     integer part and a 48-bit fraction and adds both with 64-bit integer atomics into one of NSLOT
//     copies (slot = blockIdx & 7, i.e. one per XCD under round-robin dispatch) so 256 blocks do not
//     serialise on 64 addresses; integer addition is associative, so the totals -- and everything
//     downstream -- are bitwise reproducible (graph replay == eager launches) at the cost of fp64
//     atomics (r6: the ticketed per-slot-group flush this replaces cost 54 us per step); consumers fold
//     the slots once per block (64 threads) into LDS coefficient tables;
//   * stride-2 dgrad is a stride-1 correlation over a zero-inserted LDS image (pad 2/0);
//   * weight gradients: split-K over image groups x m-chunks, several images staged per barrier, both
//     operands read with ds_read_b64_tr_b16 from NHWC LDS images (per-lane row addresses absorb stride
//     and taps);
//   * the SGD kernel reduces the slabs in fixed order (per-layer split factor so every thread issues
//     <= 8 loads), updates BN running statistics, refreshes both bf16 weight shadows and bumps the
//     device step counter (graph-capturable).
#include "rn_conv_core.h"

namespace dmlc {
namespace rn {

// ================================ forward ======================================================
template <int CIN, int COUT, int HIN, int S>
__global__ __launch_bounds__(RT) void k_rn_fwd(DmlcRnFwdArgs a) {
  using F = Fwd<CIN, COUT, HIN, S>;
  constexpr int CINP = F::CINP, HP = F::HP, HOUT = F::HOUT, KP = F::KP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* xs = reinterpret_cast<bf16*>(smem);
  float* red = reinterpret_cast<float*>(smem + F::XB);          // [4][2][64]
  float* cf = red + 4 * 2 * 64;                                  // [2][64] BN scale / shift of layer l-1
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = wave_id(), g = lane >> 4, li = lane & 15;
  // timing build only (tools/rn_ktiming.py): phases of the stage-1 16->16 forward, kernel id 0
  constexpr bool TS = CIN == 16 && COUT == 16 && S == 1;
  if (TS) DMLC_STAMP(0, 0);
  // weight fragments first (independent of everything): their latency overlaps the prologue's
  const int ct = w % F::CT, pt0 = w / F::CT;
  const bf16* W = reinterpret_cast<const bf16*>(a.w) + (16 * ct + li) * KP + 8 * g;
  bf16x8 wa[F::KS];
#pragma unroll
  for (int ks = 0; ks < F::KS; ++ks) wa[ks] = glb_b128(W + 32 * ks);

  // ---- prologue: padded input image (stem: dataset gather; else BN-apply of layer l-1) ----
  if constexpr (CIN == 3) {
    const uint8_t* img = a.data + (size_t)batch_index(a.src, a.B, b) * 3072;
    stage_stem<F::NCH, HP, F::PADB, HIN>(xs, a.cy, a.cx, tid, [&](int e, int& e1) { e1 = e; return img; });
  } else {
    constexpr int C8 = CIN / 8;
    const int c8 = tid % C8;                  // fixed channel chunk of this thread (RT % C8 == 0)
    const uint4* zp = reinterpret_cast<const uint4*>(a.z_prev) + (size_t)b * HIN * HIN * C8;
    const uint4* ss = reinterpret_cast<const uint4*>(a.sc_src);
    uint4 zv[F::IT], sv[F::IT];
#pragma unroll
    for (int i = 0; i < F::IT; ++i) {
      const int e = min(tid + i * RT, F::NCH - 1);
      // (pad_decode written out, here and below: through the shared function this prologue allocates
      // differently, and the 16->32 stride-2 kernel's occupancy moves with it)
      const int pp = e / C8, iy = pp / HP - F::PADB, ix = pp % HP - F::PADB;
      const bool ok = iy >= 0 && iy < HIN && ix >= 0 && ix < HIN;
      const int pin = ok ? iy * HIN + ix : 0;
      zv[i] = zp[pin * C8 + c8];
      sv[i] = make_uint4(0, 0, 0, 0);
      if (a.sc_mode == 1) sv[i] = ss[((size_t)b * HIN * HIN + pin) * C8 + c8];
      else if (a.sc_mode == 2) {               // option A: x[2y][2x][c] for c < CIN/2, zero above
        const bool lowc = c8 < C8 / 2;
        const size_t q = ((size_t)b * 4 * HIN * HIN + (ok ? (2 * iy) * (2 * HIN) + 2 * ix : 0)) * (C8 / 2) + (lowc ? c8 : 0);
        const uint4 v = ss[q];
        sv[i] = lowc ? v : make_uint4(0, 0, 0, 0);
      }
    }
    // BN_{l-1} coefficients, once per block: the statistics reads go out behind the image loads
    // (computed first, they added a dependent memory round trip to the prologue)
    if (tid < CIN) {
      float mean, rstd;
      bn_mean_rstd(a.stat_prev, tid, a.inv_n_prev, mean, rstd);
      const float sc = a.gamma_prev[tid] * rstd;
      cf[tid] = sc;
      cf[64 + tid] = a.beta_prev[tid] - mean * sc;
    }
    lds_barrier();
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = cf[c8 * 8 + j]; sh[j] = cf[64 + c8 * 8 + j]; }
    uint4* ao = reinterpret_cast<uint4*>(a.a_out) + (size_t)b * HIN * HIN * C8;
#pragma unroll
    for (int i = 0; i < F::IT; ++i) {
      const int e = tid + i * RT;
      if (e < F::NCH) {
        const int pp = e / C8, iy = pp / HP - F::PADB, ix = pp % HP - F::PADB;
        const bool ok = iy >= 0 && iy < HIN && ix >= 0 && ix < HIN;
        const uint32_t zw[4] = {zv[i].x, zv[i].y, zv[i].z, zv[i].w};
        const uint32_t sw[4] = {sv[i].x, sv[i].y, sv[i].z, sv[i].w};
        uint32_t ow[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float y0 = fmaxf(bf16_lo(zw[k]) * sc[2 * k] + sh[2 * k] + bf16_lo(sw[k]), 0.f);
          const float y1 = fmaxf(bf16_hi(zw[k]) * sc[2 * k + 1] + sh[2 * k + 1] + bf16_hi(sw[k]), 0.f);
          ow[k] = ok ? pack2(y0, y1) : 0u;
        }
        const uint4 o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        reinterpret_cast<uint4*>(xs)[e] = o;
        if (ok) st_rn16(ao, (uint32_t)((iy * HIN + ix) * C8 + c8) * 16, o);
      }
    }
  }
  if (TS) DMLC_STAMP(0, 1);                       // 1: input image staged (BN-apply done)
  __syncthreads();
  if (TS) DMLC_STAMP(0, 2);                       // 2: weights in registers, barrier passed

  // ---- implicit GEMM: C[co][px] = sum_k W[co][k] X[px][k] ----
  f32x4 acc[F::NPT];
#pragma unroll
  for (int i = 0; i < F::NPT; ++i) acc[i] = zero4();
#pragma unroll
  for (int i = 0; i < F::NPT; ++i) {
    const int px = 16 * (pt0 + F::WPC * i) + li;
    const int oy = px / HOUT, ox = px - (px / HOUT) * HOUT;
    const int base = (oy * S) * HP + ox * S;
#pragma unroll
    for (int ks = 0; ks < F::KS; ++ks) {
      const int k0 = 32 * ks + 8 * g;
      const int tap = min(k0 / CINP, 8), ci0 = k0 % CINP;
      const int kh = tap / 3, kw = tap - 3 * (tap / 3);
      const bf16x8 bx = lds_b128(xs + (base + kh * HP + kw) * CINP + ci0);
      acc[i] = mfma16(wa[ks], bx, acc[i]);
    }
  }
  if (TS) DMLC_STAMP(0, 3);                       // 3: MFMAs issued
  // ---- epilogue: z (bf16) + BN partial sums ----
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  bf16* zo = reinterpret_cast<bf16*>(a.z) + (size_t)b * HOUT * HOUT * COUT;
#pragma unroll
  for (int i = 0; i < F::NPT; ++i) {
    const int px = 16 * (pt0 + F::WPC * i) + li;
    st_rn8(zo, (uint32_t)(px * COUT + 16 * ct + 4 * g) * 2, pack4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[r] += acc[i][r]; s2[r] += acc[i][r] * acc[i][r]; }
  }
  if (TS) DMLC_STAMP(0, 4);                       // 4: z stored, partial sums ready
  if (b >= a.nvalid) {                            // batch padding: not part of the BN statistics
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[r] = 0.f; s2[r] = 0.f; }
  }
  reduce_flush<F::CT, COUT>(s1, s2, red, a.stat, w, g, li, tid);
  if (TS) DMLC_STAMP(0, 5);                       // 5: statistics flushed (end)
}

// ================================ dgrad ========================================================
template <int CIN, int COUT, int HIN, int S>
DEV void rn_dgrad_body(const DmlcRnDgradArgs& a) {   // workgroup blockIdx.x = image (grid starts with these)
  using D = Dg<CIN, COUT, HIN, S>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* gs = reinterpret_cast<bf16*>(smem);
  float* red = reinterpret_cast<float*>(smem + D::GB);           // [4][2][64]
  float* cf = red + 4 * 2 * 64;                                   // [5][64]: A, Bc, Cc (layer l); mean, rstd (l-1)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = wave_id(), g = lane >> 4, li = lane & 15;
  constexpr bool TS = CIN == 16 && COUT == 16 && S == 1;   // timing build: stage-1 dgrad, kernel id 1
  if (TS) DMLC_STAMP(1, 0);

  bnb_table<COUT, CIN>(cf, a, tid);
  // ---- prologue: g_z of layer l on the (zero-inserted for S = 2) padded grid ----
  stage_gz_padded<CIN, COUT, HIN, S>(gs, cf, a, b, tid);
  const int ct = w % D::CT, pt0 = w / D::CT, c0 = 16 * ct + 4 * g;
  bf16x8 wa[D::KS];
  dgrad_wfrags<D::KPD>(a.wd, ct, li, g, wa);
  __syncthreads();
  if (TS) DMLC_STAMP(1, 1);                       // 1: g_z staged, weights in registers

  // epilogue chunk 0 is issued here, under the MFMAs
  const ActGlobal<CIN> act{reinterpret_cast<const bf16*>(a.a_prev) + (size_t)b * HIN * HIN * CIN};
  EpiIn cur[D::EC];
  epi_load_chunk<CIN, COUT, HIN, S>(a, b, 0, pt0, li, c0, act, cur);
  f32x4 acc[D::NPT];
#pragma unroll
  for (int i = 0; i < D::NPT; ++i) acc[i] = zero4();
  dgrad_mfma<CIN, COUT, HIN, S>(gs, wa, acc, pt0, li, g);

  if (TS) DMLC_STAMP(1, 2);                       // 2: MFMAs issued
  // ---- epilogue: g_a_{l-1} (+ shortcut) -> g_y_{l-1} + its BN reductions ----
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  dgrad_epilogue<CIN, COUT, HIN, S>(a, b, acc, cur, cf, pt0, li, c0, act, s1, s2);
  if (TS) DMLC_STAMP(1, 3);                       // 3: g_y stored, partial sums ready
  reduce_flush<D::CT, CIN>(s1, s2, red, a.red_prev, w, g, li, tid);
  if (TS) DMLC_STAMP(1, 4);                       // 4: reductions flushed (end)
}

// ================================ wgrad ========================================================
template <int CIN, int COUT, int HIN, int S>
DEV void rn_wgrad_body(const DmlcRnWgradArgs& a, const int grp, const int mc) {
  using G = Wg<CIN, COUT, HIN, S>;
  constexpr int CINP = G::CINP, HP = G::HP, KP = G::KP, NT = G::NT, GLD = G::GLD, NB = G::NB;
  constexpr int C8 = COUT / 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* xs = reinterpret_cast<bf16*>(smem);                       // [NB][XE]
  bf16* gz = xs + NB * G::XE;                                     // [NB][GE]
  float* cf = reinterpret_cast<float*>(gz + NB * G::GE);          // [3][64]
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const int b0 = grp * a.B / a.G, b1 = (grp + 1) * a.B / a.G;
  constexpr bool TS = CIN == 16 && COUT == 16 && S == 1;   // timing build: stage-1 wgrad, kernel id 2
  if (TS) DMLC_STAMP(2, 0);

  bnb_table<COUT, 0>(cf, a, tid);
  const int c8 = tid % C8;                                        // RT % (C8) == 0 and GCH % C8 == 0

  f32x4 acc[G::MJ][NT];
#pragma unroll
  for (int j = 0; j < G::MJ; ++j)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[j][n] = zero4();

  // stem: the dataset rows of the block's images, once per image (thread i -> image b0 + i), published
  // by the first loop barrier.  Evaluated per staged element, the generated-order index (a keyed
  // Feistel, ~150 instructions) ran XIT times per thread per image batch.
  [[maybe_unused]] int* srow = nullptr;
  if constexpr (CIN == 3) {
    __shared__ int srow_s[RT];
    srow = srow_s;
    if (b1 - b0 <= RT && tid < b1 - b0) srow_s[tid] = batch_index(a.src, a.B, b0 + tid);
  }
  for (int bb = b0; bb < b1; bb += NB) {
    const int nb = min(NB, b1 - bb);
    __syncthreads();
    // ---- x images (padded) ----
    if constexpr (CIN == 3) {
      stage_stem<NB * G::XCH, HP, G::PADB, HIN>(xs, a.cy, a.cx, tid, [&](int e, int& e1) {
        const int im = min(e / G::XCH, nb - 1);
        e1 = e - (e / G::XCH) * G::XCH;
        const int row = b1 - b0 <= RT ? srow[bb - b0 + im] : batch_index(a.src, a.B, bb + im);
        return a.data + (size_t)row * 3072;
      });
    } else {
      constexpr int X8 = CIN / 8;
      uint4 xv[G::XIT];
#pragma unroll
      for (int i = 0; i < G::XIT; ++i) {
        const int e = min(tid + i * RT, NB * G::XCH - 1);
        const int im = min(e / G::XCH, nb - 1), e1 = e - (e / G::XCH) * G::XCH;
        const uint4* xp = reinterpret_cast<const uint4*>(a.x) + (size_t)(bb + im) * HIN * HIN * X8;
        const PadPx d = pad_decode<HP, G::PADB, HIN>(e1 / X8);
        const int iy = d.iy, ix = d.ix;
        const bool ok = d.ok;
        xv[i] = load_sel(xp + (ok ? (iy * HIN + ix) * X8 + e1 % X8 : 0), xp, ok);
      }
#pragma unroll
      for (int i = 0; i < G::XIT; ++i) {
        const int e = tid + i * RT;
        if (e < NB * G::XCH) reinterpret_cast<uint4*>(xs)[e] = xv[i];
      }
    }
    // ---- g_z images [NB][NPIX][GLD] ----
    {
      uint4 gv[G::GIT], zv[G::GIT];
#pragma unroll
      for (int i = 0; i < G::GIT; ++i) {
        const int e = min(tid + i * RT, NB * G::GCH - 1);
        const int im = min(e / G::GCH, nb - 1), e1 = e - (e / G::GCH) * G::GCH;
        const size_t off = (size_t)(bb + im) * G::GCH + e1;
        gv[i] = reinterpret_cast<const uint4*>(a.gy)[off];
        zv[i] = reinterpret_cast<const uint4*>(a.z)[off];
      }
      // (Bnb8 written out: through the shared struct two of these kernels' occupancy moves)
      float A[8], Bc[8], Cc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { A[j] = cf[c8 * 8 + j]; Bc[j] = cf[64 + c8 * 8 + j]; Cc[j] = cf[128 + c8 * 8 + j]; }
#pragma unroll
      for (int i = 0; i < G::GIT; ++i) {
        const int e = tid + i * RT;
        if (e < NB * G::GCH) {
          const int im = e / G::GCH, e1 = e - im * G::GCH;
          const uint32_t gw[4] = {gv[i].x, gv[i].y, gv[i].z, gv[i].w}, zw[4] = {zv[i].x, zv[i].y, zv[i].z, zv[i].w};
          const bool real = bb + im < a.nvalid;          // batch padding: g_z = 0
          uint32_t ow[4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            ow[k] = real ? pack2(bnb_apply(A[2 * k], Bc[2 * k], Cc[2 * k], bf16_lo(gw[k]), bf16_lo(zw[k])),
                                 bnb_apply(A[2 * k + 1], Bc[2 * k + 1], Cc[2 * k + 1], bf16_hi(gw[k]), bf16_hi(zw[k])))
                         : 0u;
          *reinterpret_cast<uint4*>(gz + im * G::GE + (e1 / C8) * GLD + (e1 % C8) * 8) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
      }
    }
    __syncthreads();
    if (TS && bb == b0) DMLC_STAMP(2, 1);         // 1: first staging step in LDS
    // ---- MFMA over the staged images' pixels ----
    // (wgrad_kloop written out: called as the shared function, the 8-step loops of the 16x16 layers are no
    // longer fully unrolled and two kernels' occupancy moves; the per-image backward uses wgrad_kloop)
    const auto t = wgrad_tiles<CINP, HP, G::MT, G::MCH, G::MJ>(mc, w, p);
    for (int im = 0; im < nb; ++im) {
      const bf16* xi = xs + im * G::XE;
      const bf16* gi = gz + im * G::GE;
      auto frags = [&](int s, bf16x8 (&bf)[NT], bf16x8 (&af)[G::MJ]) {
        const int rA = 32 * s + 8 * g + q, rB = rA + 4;
#pragma unroll
        for (int n = 0; n < NT; ++n) bf[n] = tr_frag(gi + rA * GLD + 16 * n + 4 * p, gi + rB * GLD + 16 * n + 4 * p);
        const int pA = WgXRow<G::HOUT, S, HP>{}(rA), pB = WgXRow<G::HOUT, S, HP>{}(rB);
#pragma unroll
        for (int j = 0; j < G::MJ; ++j)
          if (t.on[j]) af[j] = tr_frag(xi + (pA + t.moff[j]) * CINP + t.mci[j], xi + (pB + t.moff[j]) * CINP + t.mci[j]);
      };
      bf16x8 bf[NT], af[G::MJ];
      frags(0, bf, af);
      for (int s = 0; s < G::KSTEPS; ++s) {
        bf16x8 bn[NT], an[G::MJ];
        wait_lds();                                  // step s's fragments have landed
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < G::KSTEPS) frags(s + 1, bn, an);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < G::MJ; ++j)
          if (t.on[j]) {
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[j][n] = mfma16(af[j], bf[n], acc[j][n]);
          }
#pragma unroll
        for (int n = 0; n < NT; ++n) bf[n] = bn[n];
#pragma unroll
        for (int j = 0; j < G::MJ; ++j) af[j] = an[j];
      }
    }
  }
  if (TS) DMLC_STAMP(2, 2);                       // 2: all MFMAs issued
  wgrad_store<COUT>(a.part + (size_t)grp * KP * COUT, wgrad_tiles<CINP, HP, G::MT, G::MCH, G::MJ>(mc, w, p), acc, g, li);
  if (TS) DMLC_STAMP(2, 3);                       // 3: slab written (end)
}

template <int CIN, int COUT, int HIN, int S>
__global__ __launch_bounds__(RT) void k_rn_dgrad(DmlcRnDgradArgs a) { rn_dgrad_body<CIN, COUT, HIN, S>(a); }

template <int CIN, int COUT, int HIN, int S>
__global__ __launch_bounds__(RT) void k_rn_wgrad(DmlcRnWgradArgs a) {
  rn_wgrad_body<CIN, COUT, HIN, S>(a, blockIdx.x, blockIdx.y);
}

// Layer l's input gradient AND weight gradient in ONE launch (both only read what layer l+1's dgrad
// produced): workgroups [0, B) run the dgrad body (one image each, the same blockIdx as its own
// launch, so the BN-reduction slots are unchanged), the rest the wgrad body (group, m-chunk).  One
// launch per layer instead of two, with no stream fork/join in the step graph.
template <int CIN, int COUT, int HIN, int S>
__global__ __launch_bounds__(RT, 2) void k_rn_bwd(DmlcRnDgradArgs d, DmlcRnWgradArgs w) {
  if ((int)blockIdx.x < d.B) {
    rn_dgrad_body<CIN, COUT, HIN, S>(d);
  } else {
    const int t = (int)blockIdx.x - d.B;
    rn_wgrad_body<CIN, COUT, HIN, S>(w, t % w.G, t / w.G);
  }
}

// ============================ per-image backward (stride 1, one slab per image) ====================
// Layer l's input gradient AND its weight gradient from ONE workgroup per image: the g_z image the
// dgrad stages (padded, [HPD][HPD][COUT]) is also the weight gradient's B operand, and the layer
// input a_{l-1} is staged once into LDS (padded) for both the dgrad epilogue's ReLU mask and the
// weight gradient's A operand -- the separate wgrad blocks re-read g_y, z and a_{l-1} from memory
// (96 KB per 32x32x16 image).  Needs one split-K group per image (w.G == B, the 16-channel layers'
// choice at B <= 256): the slab of image b is part[b].  Same per-image sums in the same k-step
// order as the grouped wgrad body: the step is bitwise the merged launch's.
template <int CIN, int COUT, int HIN>
__global__ __launch_bounds__(RT, 2) void k_rn_bwd_img(DmlcRnDgradArgs a, DmlcRnWgradArgs wa_) {
  using D = Dg<CIN, COUT, HIN, 1>;
  using I = BwdImg<CIN, COUT, HIN>;
  constexpr int HPD = D::HPD, HP = I::HP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* gs = reinterpret_cast<bf16*>(smem);
  bf16* xs = reinterpret_cast<bf16*>(smem + D::GB);
  float* red = reinterpret_cast<float*>(smem + D::GB + I::XB);   // [4][2][64]
  float* cf = red + 4 * 2 * 64;                                  // [5][64]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = wave_id(), g = lane >> 4, li = lane & 15;
  const int q = li >> 2, p = li & 3;

  bnb_table<COUT, CIN>(cf, a, tid);
  stage_gz_padded<CIN, COUT, HIN, 1>(gs, cf, a, b, tid);
  // the layer input a_{l-1} (padded, halo 0): its loads fly during the dgrad MFMAs
  uint4 xv[I::XIT];
  {
    constexpr int X8 = CIN / 8;
    const uint4* xp = reinterpret_cast<const uint4*>(a.a_prev) + (size_t)b * HIN * HIN * X8;
#pragma unroll
    for (int i = 0; i < I::XIT; ++i) {
      const int e = min(tid + i * RT, I::XCH - 1);
      const PadPx d = pad_decode<HP, 1, HIN>(e / X8);
      const int iy = d.iy, ix = d.ix;
      const bool ok = d.ok;
      xv[i] = load_sel(xp + (ok ? (iy * HIN + ix) * X8 + e % X8 : 0), xp, ok);
    }
  }
  const int ct = w % D::CT, pt0 = w / D::CT, c0 = 16 * ct + 4 * g;
  bf16x8 wdf[D::KS];
  dgrad_wfrags<D::KPD>(a.wd, ct, li, g, wdf);
  __syncthreads();
  f32x4 acc[D::NPT];
#pragma unroll
  for (int i = 0; i < D::NPT; ++i) acc[i] = zero4();
  dgrad_mfma<CIN, COUT, HIN, 1>(gs, wdf, acc, pt0, li, g);
#pragma unroll
  for (int i = 0; i < I::XIT; ++i) {
    const int e = tid + i * RT;
    if (e < I::XCH) reinterpret_cast<uint4*>(xs)[e] = xv[i];
  }
  __syncthreads();                                // xs complete (the epilogue's mask reads it)

  const ActLds<HIN, HP, CIN> act{xs};
  EpiIn cur[D::EC];
  epi_load_chunk<CIN, COUT, HIN, 1>(a, b, 0, pt0, li, c0, act, cur);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  dgrad_epilogue<CIN, COUT, HIN, 1>(a, b, acc, cur, cf, pt0, li, c0, act, s1, s2);
  reduce_flush<D::CT, CIN>(s1, s2, red, a.red_prev, w, g, li, tid);

  // ---- weight gradient of this image: every m-tile, g_z rows read from the padded dgrad image ----
  const auto tiles = wgrad_tiles<CIN, HP, I::MT, I::MT, I::MJ>(0, w, p);
  f32x4 wacc[I::MJ][I::NT];
#pragma unroll
  for (int j = 0; j < I::MJ; ++j)
#pragma unroll
    for (int n = 0; n < I::NT; ++n) wacc[j][n] = zero4();
  wgrad_kloop<I::KSTEPS, CIN>(xs, [&](int r) { return gs + (((r / HIN) + 1) * HPD + (r % HIN) + 1) * COUT; },
                              WgXRow<HIN, 1, HP>{}, tiles, wacc, g, q, p);
  wgrad_store<COUT>(wa_.part + (size_t)b * I::KP * COUT, tiles, wacc, g, li);
}

}  // namespace rn
}  // namespace dmlc

using namespace dmlc;
using namespace dmlc::rn;

namespace {

template <int CI_, int CO_, int H_, int ST_>
struct Shape { static constexpr int CI = CI_, CO = CO_, H = H_, ST = ST_; };

// f(Shape<CIN, COUT, HIN, S>{}) of the ResNet-20 layer shape g names; STEM = false leaves the stem out
// (it has no input gradient, and Dg<3, ...> does not exist)
template <bool STEM, class F>
hipError_t for_shape(const DmlcRnLayerGeom* g, F&& f) {
#define X(CI, CO, H, ST)                                                                  \
  if constexpr (STEM || CI >= 16)                                                         \
    if (g->cin == CI && g->cout == CO && g->hin == H && g->stride == ST) return f(Shape<CI, CO, H, ST>{});
  X(3, 16, 32, 1) X(16, 16, 32, 1) X(16, 32, 32, 2) X(32, 32, 16, 1) X(32, 64, 16, 2) X(64, 64, 8, 1)
#undef X
  return hipErrorInvalidValue;
}

template <int C, int H>
hipError_t launch_bwd_img(const DmlcRnDgradArgs& d, const DmlcRnWgradArgs& w, hipStream_t s) {
  using I = BwdImg<C, C, H>;
  if (w.G != d.B) return hipErrorInvalidValue;   // one slab per image
  DMLC_LDS_OPTIN((&k_rn_bwd_img<C, C, H>), I::LDS);
  hipLaunchKernelGGL((k_rn_bwd_img<C, C, H>), dim3(d.B), dim3(RT), I::LDS, s, d, w);
  return hipGetLastError();
}

}  // namespace

extern "C" {

hipError_t dmlc_rn_fwd(const DmlcRnLayerGeom* g, const DmlcRnFwdArgs* a, hipStream_t s) {
  return for_shape<true>(g, [&](auto sh) {
    constexpr int CI = sh.CI, CO = sh.CO, H = sh.H, ST = sh.ST;
    using F = Fwd<CI, CO, H, ST>;
    DMLC_LDS_OPTIN((&k_rn_fwd<CI, CO, H, ST>), F::LDS);
    hipLaunchKernelGGL((k_rn_fwd<CI, CO, H, ST>), dim3(a->B), dim3(RT), F::LDS, s, *a);
    return hipGetLastError();
  });
}

hipError_t dmlc_rn_dgrad(const DmlcRnLayerGeom* g, const DmlcRnDgradArgs* a, hipStream_t s) {
  return for_shape<false>(g, [&](auto sh) {
    constexpr int CI = sh.CI, CO = sh.CO, H = sh.H, ST = sh.ST;
    using D = Dg<CI, CO, H, ST>;
    DMLC_LDS_OPTIN((&k_rn_dgrad<CI, CO, H, ST>), D::LDS);
    hipLaunchKernelGGL((k_rn_dgrad<CI, CO, H, ST>), dim3(a->B), dim3(RT), D::LDS, s, *a);
    return hipGetLastError();
  });
}

hipError_t dmlc_rn_wgrad(const DmlcRnLayerGeom* g, const DmlcRnWgradArgs* a, hipStream_t s) {
  return for_shape<true>(g, [&](auto sh) {
    constexpr int CI = sh.CI, CO = sh.CO, H = sh.H, ST = sh.ST;
    using G = Wg<CI, CO, H, ST>;
    DMLC_LDS_OPTIN((&k_rn_wgrad<CI, CO, H, ST>), G::LDS);
    hipLaunchKernelGGL((k_rn_wgrad<CI, CO, H, ST>), dim3(a->G, G::MC), dim3(RT), G::LDS, s, *a);
    return hipGetLastError();
  });
}

hipError_t dmlc_rn_bwd(const DmlcRnLayerGeom* g, const DmlcRnDgradArgs* d, const DmlcRnWgradArgs* w, hipStream_t s) {
  if (d->B != w->B) return hipErrorInvalidValue;
  if (g->per_image) {                              // one workgroup per image: dgrad + wgrad
    if (g->cin == 16 && g->cout == 16 && g->hin == 32 && g->stride == 1) return launch_bwd_img<16, 32>(*d, *w, s);
    if (g->cin == 32 && g->cout == 32 && g->hin == 16 && g->stride == 1) return launch_bwd_img<32, 16>(*d, *w, s);
    return hipErrorInvalidValue;
  }
  return for_shape<false>(g, [&](auto sh) {
    constexpr int CI = sh.CI, CO = sh.CO, H = sh.H, ST = sh.ST;
    using G = Wg<CI, CO, H, ST>;
    constexpr size_t lds = Dg<CI, CO, H, ST>::LDS > G::LDS ? Dg<CI, CO, H, ST>::LDS : G::LDS;
    DMLC_LDS_OPTIN((&k_rn_bwd<CI, CO, H, ST>), lds);
    hipLaunchKernelGGL((k_rn_bwd<CI, CO, H, ST>), dim3(d->B + w->G * G::MC), dim3(RT), lds, s, *d, *w);
    return hipGetLastError();
  });
}

}  // extern "C"
