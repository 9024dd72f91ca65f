// Geometry and shared phases of the fused ResNet-20 conv kernels (resnet.hip): every staging, MFMA and
// epilogue phase that more than one kernel runs is written here once, and the kernels compose them.
// The per-image backward must stay bitwise the merged launch's, so it is a composition of these only; a
// phase a kernel still writes out says why in place (profiles/rn_core_refactor_ab.txt).
#pragma once
#include "rn_stats.h"

namespace dmlc {
namespace rn {

// streaming (nt) stores for the activations / gradients / slabs the next launches read (common.h:
// fewer dirty L2 lines to write back at every one of the ~58 kernel boundaries): 0.695 -> 0.682 ms
constexpr bool kNtRn = kNtDefault;
#ifdef DMLC_RN_SLAB_PLAIN   // A/B build, slabs stored plain: 640.4-641.5 vs 611.7-611.9 us (r6s3_rn_slab_plain_ab.txt)
constexpr bool kNtSlab = false;
#else
constexpr bool kNtSlab = kNtRn;
#endif
// activation stores (z, a, g_y -> the next launch): write-through (common.h st_out16 / st_out8) unless
// -DDMLC_RN_NT (the r3 streaming form); the fp32 slabs stay streaming (their 4-B write-through
// stores are one fabric write each: 375 vs 401 k images/s, r5 same-box A/B)
#ifdef DMLC_RN_NT
DEV void st_rn16(void* base, uint32_t off, const uint4& v) {
  st_maybe_nt<kNtRn>(reinterpret_cast<uint4*>(reinterpret_cast<char*>(base) + off), v);
}
DEV void st_rn8(void* base, uint32_t off, const bf16x4& v) {
  st_maybe_nt<kNtRn>(reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(base) + off), v);
}
#else
DEV void st_rn16(void* base, uint32_t off, const uint4& v) { st_out16(base, off, v); }
DEV void st_rn8(void* base, uint32_t off, const bf16x4& v) { st_out8(base, off, __builtin_bit_cast(uint2, v)); }
#endif

__host__ __device__ constexpr int round32(int x) { return (x + 31) / 32 * 32; }

DEV uint32_t pack2(float a, float b) {
  const bf16x4 v = pack4(a, b, 0.f, 0.f);
  return __builtin_bit_cast(uint2, v).x;
}

template <int CIN, int COUT, int HIN, int S>
struct Fwd {
  static constexpr int CINP = CIN < 8 ? 8 : CIN;
  static constexpr int HOUT = HIN / S;
  static constexpr int PADB = S == 1 ? 1 : 0;
  static constexpr int HP = HIN + (S == 1 ? 2 : 1);
  static constexpr int KP = round32(9 * CINP), KS = KP / 32;
  static constexpr int CT = COUT / 16, WPC = 4 / CT, NPXT = HOUT * HOUT / 16, NPT = NPXT / WPC;
  static constexpr int NCH = HP * HP * CINP / 8;               // 16-B chunks of the padded image
  static constexpr int IT = (NCH + RT - 1) / RT;
  static constexpr size_t XB = (size_t)HP * HP * CINP * 2;
  static constexpr size_t LDS = XB + 4 * 2 * 64 * 4 + 2 * 64 * 4;
};

template <int CIN, int COUT, int HIN, int S>
struct Dg {
  static constexpr int HOUT = HIN / S;
  static constexpr int HPD = HIN + 2;
  static constexpr int KPD = round32(9 * COUT), KS = KPD / 32;
  static constexpr int CT = CIN / 16, WPC = 4 / CT, NPXT = HIN * HIN / 16, NPT = NPXT / WPC;
  static constexpr int NCH = HPD * HPD * COUT / 8;
  static constexpr int IT = (NCH + RT - 1) / RT;
  static constexpr int EC = NPT < 4 ? NPT : 4;                 // pixel tiles per epilogue chunk
  static constexpr size_t GB = (size_t)HPD * HPD * COUT * 2;
  static constexpr size_t LDS = GB + 4 * 2 * 64 * 4 + 5 * 64 * 4;
};

// Block (grp, mc): images [grp*B/G, (grp+1)*B/G), slab rows of m-tiles [mc*MCH, (mc+1)*MCH); NB images are
// staged per barrier (LDS budget ~120 KB) so their global loads are all in flight together.
template <int CIN, int COUT, int HIN, int S>
struct Wg {
  static constexpr int CINP = CIN < 8 ? 8 : CIN;
  static constexpr int HOUT = HIN / S;
  static constexpr int PADB = S == 1 ? 1 : 0;
  static constexpr int HP = HIN + (S == 1 ? 2 : 1);
  static constexpr int KP = round32(9 * CINP);
  static constexpr int MT = KP / 16;
  static constexpr int MC = MT <= 12 ? 1 : (MT <= 24 ? 2 : 3);           // m-chunks (grid.y)
  static constexpr int MCH = (MT + MC - 1) / MC;
  static constexpr int MJ = (MCH + 3) / 4;                               // m-tiles per wave
  static constexpr int NT = COUT / 16;
  static constexpr int NPIX = HOUT * HOUT, KSTEPS = NPIX / 32;
  static constexpr int GLD = COUT + 8;                                   // g_z LDS row stride (bf16)
  static constexpr int XE = HP * HP * CINP, GE = NPIX * GLD;            // bf16 elements per image
  static constexpr int XCH = XE / 8, GCH = NPIX * COUT / 8;             // 16-B chunks per image
  static constexpr int PER_IMG = (XE + GE) * 2;
  static constexpr int NB = (120 * 1024 / PER_IMG) < 1 ? 1 : ((120 * 1024 / PER_IMG) > 4 ? 4 : 120 * 1024 / PER_IMG);
  static constexpr int XIT = (NB * XCH + RT - 1) / RT, GIT = (NB * GCH + RT - 1) / RT;
  static constexpr size_t LDS = (size_t)NB * PER_IMG + 3 * 64 * 4;
};

// per-image backward (stride 1): the dgrad's geometry plus one weight-gradient m-chunk of all MT tiles
template <int CIN, int COUT, int HIN>
struct BwdImg {
  using D = Dg<CIN, COUT, HIN, 1>;
  static constexpr int HP = HIN + 2, CINP = CIN;
  static constexpr int XCH = HP * HP * CIN / 8, XIT = (XCH + RT - 1) / RT;
  static constexpr size_t XB = (size_t)HP * HP * CIN * 2;
  static constexpr int KP = round32(9 * CIN), MT = KP / 16, MJ = (MT + 3) / 4, NT = COUT / 16;
  static constexpr int NPIX = HIN * HIN, KSTEPS = NPIX / 32;
  static constexpr size_t LDS = D::GB + XB + 4 * 2 * 64 * 4 + 5 * 64 * 4;
  static_assert(CIN == COUT && CIN % 16 == 0 && NPIX % 32 == 0, "per-image backward: square stride-1 layers");
};

// pixel pp of a zero-padded [HP][HP] grid with PAD leading rows / columns -> (iy, ix) of the [H][H]
// image under it; false on the halo
struct PadPx { int iy, ix; bool ok; };
template <int HP, int PAD, int H>
DEV PadPx pad_decode(int pp) {
  const int iy = pp / HP - PAD, ix = pp % HP - PAD;
  return {iy, ix, iy >= 0 && iy < H && ix >= 0 && ix < H};
}

// uint8 NHWC pixel (3 channels) -> 8 bf16 lanes (ci 3..7 zero)
DEV uint4 px_u8_to_bf16x8(uint32_t v) {
  return make_uint4(pack2((float)(v & 0xff), (float)((v >> 8) & 0xff)), pack2((float)((v >> 16) & 0xff), 0.f), 0u, 0u);
}
DEV uint32_t load_px_u8(const uint8_t* img, int cy, int cx, int iy, int ix, bool ok) {
  const uint8_t* s = img + (ok ? ((cy + iy) * 32 + cx + ix) * 3 : 0);
  const uint32_t v = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
  return ok ? v : 0u;
}

// stem input: N pixels (one 16-B chunk each) of padded dataset crops into xs, every load before any
// LDS store.  img_of(e, e1) returns the dataset image of chunk e and sets e1, its pixel on the grid.
template <int N, int HP, int PAD, int HIN, class ImgOf>
DEV void stage_stem(bf16* xs, int cy, int cx, int tid, ImgOf img_of) {
  constexpr int IT = (N + RT - 1) / RT;
  uint32_t px3[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    int e1;
    const uint8_t* img = img_of(min(tid + i * RT, N - 1), e1);
    const PadPx d = pad_decode<HP, PAD, HIN>(e1);
    px3[i] = load_px_u8(img, cy, cx, d.iy, d.ix, d.ok);
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = tid + i * RT;
    if (e < N) reinterpret_cast<uint4*>(xs)[e] = px_u8_to_bf16x8(px3[i]);
  }
}

// coefficient tables in LDS, once per block: cf[0..191] = A, Bc, Cc of layer l (threads 0..COUT-1)
// and, for the dgrad epilogue (CIN > 0), cf[192..] = mean, rstd of layer l-1 (threads 128..128+CIN-1)
template <int COUT, int CIN, class Args>
DEV void bnb_table(float* cf, const Args& a, int tid) {
  if (tid < COUT) {
    float A, Bc, Cc;
    bnb_coeffs(a.stat, a.red, a.gamma, tid, a.inv_n, A, Bc, Cc);
    cf[tid] = A; cf[64 + tid] = Bc; cf[128 + tid] = Cc;
  } else if constexpr (CIN > 0) {
    if (tid >= 128 && tid < 128 + CIN) {
      float mean, rstd;
      bn_mean_rstd(a.stat_prev, tid - 128, a.inv_n_prev, mean, rstd);
      cf[192 + tid - 128] = mean; cf[256 + tid - 128] = rstd;
    }
  }
}

// the table's coefficients of channel chunk c8, and g_z of those 8 channels from the 16-B chunks of
// g_y and z (zero unless `on`)
struct Bnb8 {
  float A[8], Bc[8], Cc[8];
  MDEV Bnb8(const float* cf, int c8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { A[j] = cf[c8 * 8 + j]; Bc[j] = cf[64 + c8 * 8 + j]; Cc[j] = cf[128 + c8 * 8 + j]; }
  }
  MDEV uint4 operator()(const uint4& gv, const uint4& zv, bool on) const {
    const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w}, zw[4] = {zv.x, zv.y, zv.z, zv.w};
    uint32_t ow[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v0 = bnb_apply(A[2 * k], Bc[2 * k], Cc[2 * k], bf16_lo(gw[k]), bf16_lo(zw[k]));
      const float v1 = bnb_apply(A[2 * k + 1], Bc[2 * k + 1], Cc[2 * k + 1], bf16_hi(gw[k]), bf16_hi(zw[k]));
      ow[k] = on ? pack2(v0, v1) : 0u;
    }
    return make_uint4(ow[0], ow[1], ow[2], ow[3]);
  }
};

// g_z of layer l of image b on the (zero-inserted for S = 2) padded grid gs [HPD][HPD][COUT]; the
// barrier inside publishes the coefficient table (bnb_table) behind the image loads
template <int CIN, int COUT, int HIN, int S>
DEV void stage_gz_padded(bf16* gs, const float* cf, const DmlcRnDgradArgs& a, int b, int tid) {
  using D = Dg<CIN, COUT, HIN, S>;
  constexpr int HOUT = D::HOUT, HPD = D::HPD, C8 = COUT / 8;
  const int c8 = tid % C8;
  const uint4* gyp = reinterpret_cast<const uint4*>(a.gy) + (size_t)b * HOUT * HOUT * C8;
  const uint4* zp = reinterpret_cast<const uint4*>(a.z) + (size_t)b * HOUT * HOUT * C8;
  uint4 gv[D::IT], zv[D::IT];
  bool okv[D::IT];
#pragma unroll
  for (int i = 0; i < D::IT; ++i) {
    const int e = min(tid + i * RT, D::NCH - 1);
    const int pp = e / C8;
    int oy, ox;
    bool ok;
    if (S == 1) { const PadPx d = pad_decode<HPD, 1, HOUT>(pp); oy = d.iy; ox = d.ix; ok = d.ok; }
    else {
      const int py = pp / HPD, px = pp % HPD;
      oy = (py - 2) >> 1; ox = (px - 2) >> 1;
      ok = py >= 2 && px >= 2 && !((py - 2) & 1) && !((px - 2) & 1) && oy < HOUT && ox < HOUT;
    }
    const int q = (ok ? oy * HOUT + ox : 0) * C8 + c8;
    gv[i] = gyp[q];
    zv[i] = zp[q];
    okv[i] = ok && (tid + i * RT) < D::NCH && b < a.nvalid;   // padding image: g_z = 0
  }
  lds_barrier();
  const Bnb8 gz8(cf, c8);
#pragma unroll
  for (int i = 0; i < D::IT; ++i) {
    const int e = tid + i * RT;
    if (e < D::NCH) reinterpret_cast<uint4*>(gs)[e] = gz8(gv[i], zv[i], okv[i]);
  }
}

// ================================ dgrad ========================================================
// the wave's rows (16 * ct + li) of the rotated weight shadow wd [CIN][KPD], all k-steps
template <int KPD, int KS>
DEV void dgrad_wfrags(const void* wd, int ct, int li, int g, bf16x8 (&wa)[KS]) {
  const bf16* Wd = reinterpret_cast<const bf16*>(wd) + (16 * ct + li) * KPD + 8 * g;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) wa[ks] = glb_b128(Wd + 32 * ks);
}

// acc (zeroed by the kernel) += C[ci][px_in] = sum_{tap', co} Wd[ci][tap'*COUT + co] G[(iy+kh')*HPD + ix + kw'][co]
template <int CIN, int COUT, int HIN, int S>
DEV void dgrad_mfma(const bf16* gs, const bf16x8 (&wa)[Dg<CIN, COUT, HIN, S>::KS],
                    f32x4 (&acc)[Dg<CIN, COUT, HIN, S>::NPT], int pt0, int li, int g) {
  using D = Dg<CIN, COUT, HIN, S>;
  constexpr int HPD = D::HPD;
#pragma unroll
  for (int i = 0; i < D::NPT; ++i) {
    const int px = 16 * (pt0 + D::WPC * i) + li;
    const int iy = px / HIN, ix = px - (px / HIN) * HIN;
    const int base = iy * HPD + ix;
#pragma unroll
    for (int ks = 0; ks < D::KS; ++ks) {
      const int k0 = 32 * ks + 8 * g;
      const int tap = min(k0 / COUT, 8), co0 = k0 % COUT;
      const int kh = tap / 3, kw = tap - 3 * (tap / 3);
      const bf16x8 bx = lds_b128(gs + (base + kh * HPD + kw) * COUT + co0);
      acc[i] = mfma16(wa[ks], bx, acc[i]);
    }
  }
}

// Epilogue operands of layer l-1 (activation for the ReLU mask, z for x-hat, the shortcut's g_y),
// 4 pixel tiles per chunk, software-pipelined: the kernel issues chunk 0 (epi_load_chunk), and the
// epilogue chunk c+1 before chunk c's stores.  (Loaded inside the store loop, every tile paid a full
// memory latency -- the stores may alias the loads -- 11 of the kernel's 22 us at 16 tiles per wave.)
// Where the activation comes from is the caller's: ActGlobal travels with the chunk, ActLds is read
// at the tile's turn.
struct EpiIn { uint2 a, z, s; };
template <int CIN>
struct ActGlobal {     // a_{l-1} of image b in global memory [HIN][HIN][CIN]
  static constexpr bool kWithChunk = true;
  const bf16* ap;
  MDEV uint2 operator()(int px, int c0) const { return *reinterpret_cast<const uint2*>(ap + px * CIN + c0); }
};
template <int HIN, int HP, int CIN>
struct ActLds {        // a_{l-1} staged as a padded LDS image [HP][HP][CIN] (complete before the epilogue)
  static constexpr bool kWithChunk = false;
  const bf16* xs;
  MDEV uint2 operator()(int px, int c0) const {
    const int iy = px / HIN, ix = px - (px / HIN) * HIN;
    return *reinterpret_cast<const uint2*>(xs + ((iy + 1) * HP + ix + 1) * CIN + c0);
  }
};

// chunk c's operands of the wave's pixel tiles c .. c + EC - 1 (channels c0 .. c0 + 3)
template <int CIN, int COUT, int HIN, int S, class Act>
DEV void epi_load_chunk(const DmlcRnDgradArgs& a, int b, int c, int pt0, int li, int c0, const Act& act,
                        EpiIn (&e)[Dg<CIN, COUT, HIN, S>::EC]) {
  using D = Dg<CIN, COUT, HIN, S>;
  const bf16* zpp = reinterpret_cast<const bf16*>(a.z_prev) + (size_t)b * HIN * HIN * CIN;
#pragma unroll
  for (int j = 0; j < D::EC; ++j) {
    const int px = 16 * (pt0 + D::WPC * (c + j)) + li;
    const int iy = px / HIN, ix = px - (px / HIN) * HIN;
    e[j].a = make_uint2(0u, 0u);
    if constexpr (Act::kWithChunk) e[j].a = act(px, c0);
    e[j].z = *reinterpret_cast<const uint2*>(zpp + px * CIN + c0);
    e[j].s = make_uint2(0u, 0u);
    if (a.sc_mode == 1) {
      e[j].s = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16*>(a.gy_sc) + ((size_t)b * HIN * HIN + px) * CIN + c0);
    } else if (a.sc_mode == 2) {
      const bool even = !(iy & 1) && !(ix & 1);
      const int HB = HIN / 2;
      const size_t q = ((size_t)b * HB * HB + (even ? (iy / 2) * HB + ix / 2 : 0)) * (2 * CIN) + c0;
      const uint2 v = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16*>(a.gy_sc) + q);
      e[j].s = even ? v : make_uint2(0u, 0u);
    }
  }
}

// g_a_{l-1} (+ shortcut) -> g_y_{l-1} (stored) + its BN reduction partials s1 = sum g_y, s2 = sum g_y*xhat
template <int CIN, int COUT, int HIN, int S, class Act>
DEV void dgrad_epilogue(const DmlcRnDgradArgs& a, int b, const f32x4 (&acc)[Dg<CIN, COUT, HIN, S>::NPT],
                        EpiIn (&cur)[Dg<CIN, COUT, HIN, S>::EC], const float* cf, int pt0, int li, int c0,
                        const Act& act, float (&s1)[4], float (&s2)[4]) {
  using D = Dg<CIN, COUT, HIN, S>;
  constexpr int EC = D::EC;
  float mean[4], rstd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mean[r] = cf[192 + c0 + r]; rstd[r] = cf[256 + c0 + r]; }
  bf16* gyo = reinterpret_cast<bf16*>(a.gy_prev) + (size_t)b * HIN * HIN * CIN;
#pragma unroll
  for (int c = 0; c < D::NPT; c += EC) {
    EpiIn nxt[EC];
    if (c + EC < D::NPT) epi_load_chunk<CIN, COUT, HIN, S>(a, b, c + EC, pt0, li, c0, act, nxt);
#pragma unroll
    for (int j = 0; j < EC; ++j) {
      const int i = c + j;
      const int px = 16 * (pt0 + D::WPC * i) + li;
      uint2 av = cur[j].a;
      if constexpr (!Act::kWithChunk) av = act(px, c0);
      const uint2 zv = cur[j].z, sv = cur[j].s;
      const float sc4[4] = {bf16_lo(sv.x), bf16_hi(sv.x), bf16_lo(sv.y), bf16_hi(sv.y)};
      const float av4[4] = {bf16_lo(av.x), bf16_hi(av.x), bf16_lo(av.y), bf16_hi(av.y)};
      const float zv4[4] = {bf16_lo(zv.x), bf16_hi(zv.x), bf16_lo(zv.y), bf16_hi(zv.y)};
      float gy[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gy[r] = av4[r] > 0.f ? acc[i][r] + sc4[r] : 0.f;
        s1[r] += gy[r];
        s2[r] = __builtin_fmaf(gy[r] * (zv4[r] - mean[r]), rstd[r], s2[r]);   // pinned (bitwise across kernels)
      }
      st_rn8(gyo, (uint32_t)(px * CIN + c0) * 2, pack4(gy[0], gy[1], gy[2], gy[3]));
    }
    if (c + EC < D::NPT) {
#pragma unroll
      for (int j = 0; j < EC; ++j) cur[j] = nxt[j];
    }
  }
}

// ================================ wgrad ========================================================
// The wave's m-tiles m = m0 + 4j of the slab (k = 16m .. 16m+15 = tap (16m) / CINP, channels
// (16m) % CINP .. +15; taps past 8: K padding; the stem's 8-channel taps come two per tile): loop-
// invariant LDS offsets of the tap (pixels) and the lane's channels.  on[j] is wave-uniform.
template <int MJ>
struct WgTiles { int m0, moff[MJ], mci[MJ]; bool on[MJ]; };
template <int CINP, int HP, int MT, int MCH, int MJ>
DEV WgTiles<MJ> wgrad_tiles(int mc, int w, int p) {
  WgTiles<MJ> t;
  t.m0 = mc * MCH + w;
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int m = t.m0 + 4 * j;
    t.on[j] = w + 4 * j < MCH && m < MT;
    int tap, ci0;
    if (CINP >= 16) { tap = (16 * m) / CINP; ci0 = (16 * m) % CINP + 4 * p; }
    else { tap = 2 * m + (p >> 1); ci0 = 4 * (p & 1); }
    tap = min(tap, 8);
    const int kh = tap / 3, kw = tap - 3 * (tap / 3);
    t.moff[j] = kh * HP + kw;
    t.mci[j] = ci0;
  }
  return t;
}

// One staged image's k-loop: C[k = (tap, ci)][co] += sum_px X[px + tap][ci] g_z[px][co], 32 pixels per
// k-step.  grow(r): LDS row (COUT bf16) of g_z of output pixel r; xrow(r): padded-grid pixel of x under
// output pixel r's tap 0.
// Software-pipelined: the next k-step's fragments (ds_read_b64_tr_b16) are read under this
// k-step's MFMAs -- with the reads in line, every k-step waited one LDS latency (the phase took
// 7 us for one 32x32x16 image, tools/rn_ktiming.py).  The wave's m-tiles are loop-invariant.
template <int KSTEPS, int CINP, int NT, int MJ, class GRow, class XRow>
DEV void wgrad_kloop(const bf16* xi, GRow grow, XRow xrow, const WgTiles<MJ>& t, f32x4 (&acc)[MJ][NT], int g,
                     int q, int p) {
  auto frags = [&](int s, bf16x8 (&bf)[NT], bf16x8 (&af)[MJ]) {
    const int rA = 32 * s + 8 * g + q, rB = rA + 4;
#pragma unroll
    for (int n = 0; n < NT; ++n) bf[n] = tr_frag(grow(rA) + 16 * n + 4 * p, grow(rB) + 16 * n + 4 * p);
    const int pA = xrow(rA), pB = xrow(rB);
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      if (t.on[j]) af[j] = tr_frag(xi + (pA + t.moff[j]) * CINP + t.mci[j], xi + (pB + t.moff[j]) * CINP + t.mci[j]);
  };
  bf16x8 bf[NT], af[MJ];
  frags(0, bf, af);
  for (int s = 0; s < KSTEPS; ++s) {
    bf16x8 bn[NT], an[MJ];
    wait_lds();                                  // step s's fragments have landed
    __builtin_amdgcn_sched_barrier(0);
    if (s + 1 < KSTEPS) frags(s + 1, bn, an);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      if (t.on[j]) {
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[j][n] = mfma16(af[j], bf[n], acc[j][n]);
      }
#pragma unroll
    for (int n = 0; n < NT; ++n) bf[n] = bn[n];
#pragma unroll
    for (int j = 0; j < MJ; ++j) af[j] = an[j];
  }
}
// xrow of a padded [HP][HP] x image: pixel under tap 0 of output pixel r (stride S, HOUT output columns)
template <int HOUT, int S, int HP>
struct WgXRow {
  MDEV int operator()(int r) const {
    const int oy = r / HOUT, ox = r - oy * HOUT;
    return (oy * S) * HP + ox * S;
  }
};

// slab rows k = 16m + 4g + i, cols co = 16n + li
template <int COUT, int NT, int MJ>
DEV void wgrad_store(float* out, const WgTiles<MJ>& t, const f32x4 (&acc)[MJ][NT], int g, int li) {
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int m = t.m0 + 4 * j;
    if (t.on[j]) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) st_maybe_nt<kNtSlab>(out + (16 * m + 4 * g + i) * COUT + 16 * n + li, acc[j][n][i]);
    }
  }
}

}  // namespace rn
}  // namespace dmlc
