// Eval-mode forward of the whole CIFAR-10 CNN (models/cifar_cnn.py cnn_forward) in true fp32 for gfx950:
// one launch carries N uint8 images to fp32 logits.  Every product runs on v_mfma_f32_16x16x4_f32 (fp32
// operands, fp32 accumulation: no bf16 / tf32 rounding anywhere) and the activations stay fp32 from the
// pixel cast to the logits.  The weights are read straight from the model's flat parameter buffer in
// their TF layouts (HWIO viewed as [kh*kw*ci][co], fc as [in][out]): this engine has no shadow copies.
//
// Shape of k_cnn_infer (cnn_infer.hip): a persistent 512-thread workgroup (at most one per CU: the LDS
// map allows no more) takes a tile of 16 images from pixels to logits on its own and loops over tiles
// (tile = blockIdx.x, += gridDim.x).  No flags, no counters, no spins, no grid barrier: no workgroup
// reads what another wrote, the only synchronisation is the workgroup barrier.
//
// MFMA lane map (16x16x4 f32, lane = 16 q + r): first operand element [row r][k q], second [k q][col r],
// result rows 4q .. 4q + 3 of column r.  Every GEMM here is formulated transposed -- D[channel][pixel or
// image] = sum_k W[k][channel] * X[pixel][k] -- so the weight is the first operand (lane r = channel: 16
// consecutive floats of a [k][n] row, one coalesced 64-B segment per q) and a lane ends with 4 consecutive
// channels of one pixel / image: bias + ReLU leave as one 16-B LDS store.  The k order inside a group of
// four k-steps is free as long as both operands agree: lane q takes k = k0 + 4q + j in step j, so the
// activation operand of four k-steps is ONE 16-B LDS read (channels 4q .. 4q + 3 of the group's 16).
//
// Per image (conv phase):
//   crop     the 3072 raw bytes (requested one image ahead) -> zero-padded 28x28x3 fp32 crop.
//   conv1    M = 576 pixels, N = 64, K = 75 padded to 76 (19 k-steps; weight row 75 is zero in LDS).  The
//            weights [76][64] stay in LDS for the whole launch.  The 24x24x64 fp32 output (147 KB) does
//            not fit, so conv1 runs in 3 bands of 9 conv rows (8b .. 8b + 8; the last band has 8), each
//            followed by the 4 rows of the TF-SAME 3x3/2 pool it feeds (window rows 2r .. 2r + 2 clipped
//            at 23; the row two bands share is recomputed).  Wave w owns pixel tiles w and w + 8 of the
//            band's 14 (12), all four channel tiles.
//   pool1    -> the zero-padded 16x16x64 fp32 conv2 input p1 (halo re-zeroed per image: the fc map
//            aliases it).
//   conv2    M = 144 (9 tiles of 4x4 pixels), N = 64, K = 1600 = 100 chunks of 16 (tap, 16 channels).
//            Wave (h, nt) = (w & 1, w >> 1) owns channel tile nt over ALL 9 pixel tiles for K half h
//            (chunks 50h .. 50h + 49): 36 accumulator registers, 1800 MFMAs per wave -- the same count on
//            every wave -- and every weight is fetched exactly once per image and CU (409.6 KB; they
//            stream from L2 as first-operand fragments straight into registers, two chunks requested
//            ahead of use).  Half 1 parks its partial sums in the output image, half 0 adds them, the
//            bias and the ReLU.
//   pool2    -> row i of the workgroup's own slab of the scratch tensor [grid][16][2304] fp32 (NHWC
//            flatten order), as write-through stores; the same workgroup reads them back with sc1 loads
//            behind vmcnt(0) + barrier (a plain load could hit the previous tile's line in L1).
// Per tile (fc phase):
//   fc1      M = 16 images, N = 384, K = 2304.  The tile's A operand comes back from the slab in 4 K chunks
//            of 576 through two LDS buffers (the next chunk's loads are in flight under the MFMAs, one
//            barrier per chunk); wave w owns n-tiles 3w .. 3w + 2 over all of K (no split), the 3.54 MB
//            weight streams once per tile, 32 k (24 loads per lane) requested ahead of use.
//   fc2/fc3  384 -> 192 (n-tiles w, w + 8) and 192 -> 10 (wave 0, N padded to 16 with zero columns), weight
//            fragments straight from memory, h1 / h2 in LDS.  Bias and ReLU as cnn_forward; per row the
//            first maximum and, with labels, the hit flag.
//
// LDS, bytes (161,472 of the CU's 163,840; the fc map aliases everything but the conv1 weights):
//   conv   [0, 24,320)        conv1 weights [76][80]
//          [24,320, 33,728)   crop [28][28][3]
//          [33,728, 95,936)   conv1 band [216][72], then conv2 output [144][72]
//          [95,936, 161,472)  p1 [16][16][64] (first: 3072 raw bytes at its pixel (2,2))
//   fc     [24,320, 99,072)   A 2 x [16][584]     [99,072, 124,160) h1 [16][392]
//          [124,160, 136,960) h2 [16][200]
// Bank behaviour of the fragment reads (tools/lds_banks.py: 64 banks, a ds_read_b128 is served in 4 lane
// groups of 16, each holding every r once with q = 0 for r in 0-3 / 12-15 and q = 1 for r in 4-11, or
// q = 2 / 3 likewise):
//   conv1 weights  ds_read_b32 of 4 k-rows x 16 consecutive n, row pitch 80 = 16 (mod 64): 64 distinct
//                  banks (f32_gemm.hip's rule).  The crop reads are 16 pixels 3 floats apart, the q groups
//                  one float apart: 2-way on a few lanes; conv1 is 15 % of the MFMAs.
//   p1             no padding: the sixteen 16-B channel chunks of a pixel are XORed with the key
//                  (x & 3) | (y & 3) << 2.  The 16 pixels of a 4x4 block, at any tap offset, carry 16
//                  distinct keys, and the chunk index of lane q is 4g + q: within a lane group the slots
//                  (g ^ y & 3) << 2 | (q ^ x & 3) are distinct -- 4 cycles, conflict-free, every tile and tap.
//   A, h1, h2,     k-major rows 8 (mod 64) floats apart: lane (q, r) starts at bank 8r + 4q, distinct 4-bank
//   band stores    windows within every lane group -- 4 cycles.
#include "common.h"
#include "api_f32.h"
#include "f32_conv_core.h"   // mfma_f32, lds4, p1_off, p1_tile, out_tile

namespace dmlc {

constexpr int FI_NT = 512, FI_TM = 16;                       // threads, images per tile
constexpr int FI_K1 = 76, FI_W1LD = 80;                      // conv1 K (padded), weight row pitch
constexpr int FI_XW = 28, FI_XN = FI_XW * FI_XW * 3;         // padded crop
constexpr int FI_BLD = 72, FI_BPIX = 9 * 24;                 // band / conv2 output pixel pitch, band pixels
constexpr int FI_KF = 2304, FI_N1 = 384, FI_N2 = 192;
constexpr int FI_WG = 2;   // fc1 weight read-ahead in groups of 16 k (3: 6 VGPRs spill, 4: 38)
constexpr int FI_KCH = 576, FI_ALD = FI_KCH + 8, FI_H1LD = FI_N1 + 8, FI_H2LD = FI_N2 + 8;
constexpr int FI_W1 = 0, FI_X = FI_W1 + FI_K1 * FI_W1LD * 4, FI_BAND = FI_X + FI_XN * 4;
constexpr int FI_P1 = FI_BAND + FI_BPIX * FI_BLD * 4, FI_CONV_LDS = FI_P1 + 256 * 64 * 4;
constexpr int FI_RAW = FI_P1 + (2 * 16 + 2) * 64 * 4;        // 3072 B = the 12 interior pixels of p1 row 2
constexpr int FI_A = FI_X, FI_H1 = FI_A + 2 * FI_TM * FI_ALD * 4, FI_H2 = FI_H1 + FI_TM * FI_H1LD * 4;
constexpr int FI_FC_LDS = FI_H2 + FI_TM * FI_H2LD * 4;
constexpr int FI_LDS = FI_CONV_LDS > FI_FC_LDS ? FI_CONV_LDS : FI_FC_LDS;
static_assert(FI_LDS <= 160 * 1024 && FI_X % 16 == 0 && FI_BAND % 16 == 0 && FI_P1 % 16 == 0 && FI_H1 % 16 == 0 &&
                  FI_H2 % 16 == 0 && 144 * FI_BLD <= FI_BPIX * FI_BLD, "f32_infer LDS map");

DEV f32x4 max4(const f32x4& a, const f32x4& b) {
  f32x4 m = {fmaxf(a[0], b[0]), fmaxf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3])};
  return m;
}
// relu(acc + bias) of a transposed accumulator tile: the lane's 4 consecutive channels
DEV f32x4 bias_relu(const f32x4& acc, const float* bias) {
  const float4 b = *reinterpret_cast<const float4*>(bias);
  f32x4 v = {fmaxf(acc[0] + b.x, 0.f), fmaxf(acc[1] + b.y, 0.f), fmaxf(acc[2] + b.z, 0.f), fmaxf(acc[3] + b.w, 0.f)};
  return v;
}

// conv1 of band b (conv rows 8b .. 8b + 8, clipped at 23) -> band [local pixel][64], bias + ReLU applied.
DEV void conv1_band(const float* W1s, const float* xs, float* band, const float* b1, int b, int w, int q, int r) {
  const int npix = b < 2 ? FI_BPIX : 8 * 24;
  for (int mt = w; 16 * mt < npix; mt += FI_NT / 64) {       // wave-uniform
    const int lp = 16 * mt + r, p = min(8 * 24 * b + lp, 575), y = p / 24, x = p - 24 * y;
    const float* xp = xs + (y * FI_XW + x) * 3;
    f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
#pragma unroll
    for (int s = 0; s < FI_K1 / 4; ++s) {
      // k = (kh*5 + kw)*3 + ci -> crop offset (kh*28 + kw)*3 + ci = k + 69 kh; k = 75 (zero weight) re-reads 74
      const int k = min(4 * s + q, 74), kh = k / 15;
      const float xv = xp[k + 69 * kh];
      const float* wr = W1s + (4 * s + q) * FI_W1LD + r;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma_f32(wr[16 * nt], xv, acc[nt]);
    }
    if (lp < npix) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        *reinterpret_cast<f32x4*>(band + lp * FI_BLD + 16 * nt + 4 * q) = bias_relu(acc[nt], b1 + 16 * nt + 4 * q);
    }
  }
}

// TF-SAME 3x3/2 max-pool of band b -> p1 rows 4b .. 4b + 3 (padded rows + 2): 4 x 12 pixels x 16 chunks
DEV void pool1_band(const float* band, float* p1, int b, int tid) {
  for (int e = tid; e < 4 * 12 * 16; e += FI_NT) {
    const int c = e & 15, pp = e >> 4, prl = pp / 12, pc = pp - 12 * prl;
    const int ny = min(3, 24 - 8 * b - 2 * prl), nx = min(3, 24 - 2 * pc);   // rows / columns inside the image
    const float* src = band + ((2 * prl) * 24 + 2 * pc) * FI_BLD + 4 * c;
    f32x4 m = lds4(src);
    for (int dy = 0; dy < ny; ++dy)
      for (int dx = 0; dx < nx; ++dx) m = max4(m, lds4(src + (dy * 24 + dx) * FI_BLD));
    *reinterpret_cast<f32x4*>(p1 + p1_off(4 * b + prl + 2, pc + 2, c)) = m;
  }
}

// One K half of conv2 for channel tile nt over all 9 pixel tiles: chunks c0 .. c0 + 49 of 16 k each,
// chunk cc = (tap cc >> 2, channels 16 (cc & 3) .. + 15).  Weights: two chunks (8 loads) ahead of use.
DEV void conv2_half(const float* W2, const float* p1, int c0, int nt, int q, int r, f32x4 (&acc)[9]) {
  const int ry = r >> 2, rx = r & 3;
  const float* wp = W2 + (4 * q) * 64 + 16 * nt + r;          // + (16 cc + j) * 64
  float bw[8], bn[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bw[j] = wp[(16 * c0 + 4 * (j & 4) + (j & 3)) * 64];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = zero4();
  for (int i = 0; i < 50; i += 2) {
    const int cn = c0 + min(i + 2, 48);                       // past the end: the last pair again
#pragma unroll
    for (int j = 0; j < 8; ++j) bn[j] = wp[(16 * cn + 4 * (j & 4) + (j & 3)) * 64];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int cc = c0 + i + u, tap = cc >> 2, g = cc & 3, kh = tap / 5, kw = tap - 5 * kh;
      const float* xp = p1 + p1_off(ry + kh, rx + kw, 4 * g + q);
      f32x4 xa[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) xa[t] = lds4(xp + p1_tile(t));
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = mfma_f32(bw[4 * u + j], xa[t][j], acc[t]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) bw[j] = bn[j];
  }
}

// TF-SAME 3x3/2 max-pool of the conv2 output [144][72] -> the slab row (6 x 6 x 64, NHWC), write-through
DEV void pool2_emit(const float* out2, rsrc_t slab, int row, int tid) {
  for (int e = tid; e < 36 * 16; e += FI_NT) {
    const int c = e & 15, pp = e >> 4, pr = pp / 6, pc = pp - 6 * pr;
    const int ny = min(3, 12 - 2 * pr), nx = min(3, 12 - 2 * pc);
    const float* src = out2 + ((2 * pr) * 12 + 2 * pc) * FI_BLD + 4 * c;
    f32x4 m = lds4(src);
    for (int dy = 0; dy < ny; ++dy)
      for (int dx = 0; dx < nx; ++dx) m = max4(m, lds4(src + (dy * 12 + dx) * FI_BLD));
    st_sc1(slab, (uint32_t)(row * FI_KF + pp * 64 + 4 * c) * 4, m);
  }
}

// The tile's A operand, K chunk kc: [16][576] floats of the slab = 2304 16-B pieces, 4.5 per thread
struct AChunk {
  f32x4 v[5];
  MDEV void fetch(rsrc_t slab, int kc, int nv, int t) {
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int e = min(t + u * FI_NT, FI_TM * 144 - 1), row = e / 144, c4 = e - 144 * row;
      const bool keep = row < nv;                              // rows past the tile's images: zeros
      const float4 x = ld_sc1(slab, (uint32_t)(keep ? row * FI_KF + kc * FI_KCH + 4 * c4 : 0) * 4);
      f32x4 y = {keep ? x.x : 0.f, keep ? x.y : 0.f, keep ? x.z : 0.f, keep ? x.w : 0.f};
      v[u] = y;
    }
  }
  MDEV void put(float* buf, int t) const {
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int e = t + u * FI_NT, row = e / 144, c4 = e - 144 * row;
      if (e < FI_TM * 144) *reinterpret_cast<f32x4*>(buf + row * FI_ALD + 4 * c4) = v[u];
    }
  }
};

__global__ __launch_bounds__(FI_NT, 1) void k_cnn_infer_f32(DmlcF32InferArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* W1s = reinterpret_cast<float*>(smem + FI_W1);
  float* xs = reinterpret_cast<float*>(smem + FI_X);
  float* band = reinterpret_cast<float*>(smem + FI_BAND);
  float* out2 = band;                                          // the band is dead after the last pool1
  float* p1 = reinterpret_cast<float*>(smem + FI_P1);
  uint8_t* raw = reinterpret_cast<uint8_t*>(smem + FI_RAW);
  float* As = reinterpret_cast<float*>(smem + FI_A);
  float* h1 = reinterpret_cast<float*>(smem + FI_H1);
  float* h2 = reinterpret_cast<float*>(smem + FI_H2);
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), q = lane >> 4, r = lane & 15;
  const int ntiles = (a.N + FI_TM - 1) / FI_TM;

  // once per workgroup: the conv1 weights [75][64] -> LDS [76][80], row 75 zero
  for (int e = tid; e < FI_K1 * 64; e += FI_NT) {
    const int k = e >> 6, n = e & 63;
    const float v = a.w1[min(e, 75 * 64 - 1)];
    W1s[k * FI_W1LD + n] = k < 75 ? v : 0.f;
  }
  const rsrc_t slab = buf_rsrc(a.scratch + (size_t)blockIdx.x * FI_TM * FI_KF);
  // image n of the launch (clamped: the request past the workgroup's last image re-reads a valid one)
  auto row_of = [&](int n) {
    n = min(n, a.N - 1);
    return min(max(a.idx ? a.idx[n] : n, 0), a.nrows - 1);
  };
  auto fetch_raw = [&](int n, int t) {       // 3072 B = 192 16-B pieces (threads past them re-read the last)
    return reinterpret_cast<const uint4*>(a.data + (size_t)row_of(n) * 3072)[min(t, 191)];
  };
  uint4 rawv = fetch_raw(blockIdx.x * FI_TM, tid);

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int nv = min(FI_TM, a.N - tile * FI_TM);
    // ======================= conv phase: image i of the tile -> slab row i =======================
    for (int i = 0; i < nv; ++i) {
      // (p1 was last read by the previous image's conv2, the fc map by the previous tile: both end in a
      // barrier.)  Raw bytes into p1's interior, zeros into its halo (rows / columns 0, 1, 14, 15).
      if (tid < 192) reinterpret_cast<uint4*>(raw)[tid] = rawv;
      for (int e = tid; e < 256 * 16; e += FI_NT) {
        const int pix = e >> 4, py = pix >> 4, px = pix & 15;
        if (py < 2 || py >= 14 || px < 2 || px >= 14) *reinterpret_cast<f32x4*>(p1 + pix * 64 + 4 * (e & 15)) = zero4();
      }
      lds_barrier();
      // the next image of this workgroup (the next tile's first after the tile's last)
      rawv = fetch_raw(i + 1 < nv ? tile * FI_TM + i + 1 : (tile + (int)gridDim.x) * FI_TM, tid);
      for (int e = tid; e < FI_XN; e += FI_NT) {               // zero-padded fp32 crop [28][28][3]
        const int yy = e / (FI_XW * 3), rem = e - yy * (FI_XW * 3), xx = rem / 3, ci = rem - 3 * xx;
        const bool in = yy >= 2 && yy < 26 && xx >= 2 && xx < 26;
        const uint8_t v = raw[in ? ((a.cy + yy - 2) * 32 + a.cx + xx - 2) * 3 + ci : 0];
        xs[e] = in ? (float)v : 0.f;
      }
      lds_barrier();
      for (int b = 0; b < 3; ++b) {
        conv1_band(W1s, xs, band, a.b1, b, w, q, r);
        lds_barrier();
        pool1_band(band, p1, b, tid);
        lds_barrier();
      }
      {
        const int h = w & 1, nt = w >> 1;
        f32x4 acc[9];
        conv2_half(a.w2, p1, 50 * h, nt, q, r, acc);
        float* o = out2 + ((r >> 2) * 12 + (r & 3)) * FI_BLD + 16 * nt + 4 * q;
        if (h == 1) {
#pragma unroll
          for (int t = 0; t < 9; ++t) *reinterpret_cast<f32x4*>(o + out_tile(t) * FI_BLD) = acc[t];
        }
        lds_barrier();
        if (h == 0) {
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            f32x4* d = reinterpret_cast<f32x4*>(o + out_tile(t) * FI_BLD);
            *d = bias_relu(acc[t] + *d, a.b2 + 16 * nt + 4 * q);
          }
        }
        lds_barrier();
      }
      pool2_emit(out2, slab, i, tid);
    }
    wait_vm_all();                         // every wave's slab stores acknowledged by L2 ...
    __syncthreads();                       // ... before any wave loads them; the conv regions are free

    // ================================ fc phase: the tile's 16 rows ================================
    {
      // ---- fc1: D[n][image] = sum_k W[k][n] * A[image][k], wave w: n-tiles 3w .. 3w + 2 ----
      AChunk ac;
      ac.fetch(slab, 0, nv, tid);
      const float* wp = a.fw1 + (size_t)(4 * q) * FI_N1 + 48 * w + r;   // + (k0 + j) * 384 + 16 t
      float wc[FI_WG][3][4], wn[FI_WG][3][4];                  // [k group of 16][n-tile][j]
      auto wload = [&](float (&d)[FI_WG][3][4], int k0) {
#pragma unroll
        for (int u = 0; u < FI_WG; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 3; ++t) d[u][t][j] = wp[(size_t)(k0 + 16 * u + j) * FI_N1 + 16 * t];
      };
      wload(wc, 0);
      f32x4 acc1[3] = {zero4(), zero4(), zero4()};
      ac.put(As, tid);
      lds_barrier();
      for (int kc = 0; kc < FI_KF / FI_KCH; ++kc) {
        if (kc + 1 < FI_KF / FI_KCH) ac.fetch(slab, kc + 1, nv, tid);
        const float* ar = As + (kc & 1) * FI_TM * FI_ALD + r * FI_ALD + 4 * q;
        for (int s = 0; s < FI_KCH / (16 * FI_WG); ++s) {
          const int k0 = kc * FI_KCH + 16 * FI_WG * s;
          wload(wn, min(k0 + 16 * FI_WG, FI_KF - 16 * FI_WG));   // past the end: the last groups again
#pragma unroll
          for (int u = 0; u < FI_WG; ++u) {
            const f32x4 xa = lds4(ar + 16 * FI_WG * s + 16 * u);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int t = 0; t < 3; ++t) acc1[t] = mfma_f32(wc[u][t][j], xa[j], acc1[t]);
          }
#pragma unroll
          for (int u = 0; u < FI_WG; ++u)
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
              for (int j = 0; j < 4; ++j) wc[u][t][j] = wn[u][t][j];
        }
        // (the other buffer was last read before the previous chunk's closing barrier)
        if (kc + 1 < FI_KF / FI_KCH) ac.put(As + ((kc + 1) & 1) * FI_TM * FI_ALD, tid);
        lds_barrier();
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int n0 = 48 * w + 16 * t + 4 * q;
        *reinterpret_cast<f32x4*>(h1 + r * FI_H1LD + n0) = bias_relu(acc1[t], a.fb1 + n0);
      }
    }
    lds_barrier();                         // h1 complete
    // ---- fc2: n-tiles w, w + 8 (wave-uniform), 24 k groups of 16 ----
    for (int jn = w; jn < FI_N2 / 16; jn += FI_NT / 64) {
      const float* wp = a.fw2 + (4 * q) * FI_N2 + 16 * jn + r;
      f32x4 acc = zero4();
#pragma unroll 6
      for (int s = 0; s < FI_N1 / 16; ++s) {
        const f32x4 xa = lds4(h1 + r * FI_H1LD + 16 * s + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma_f32(wp[(16 * s + j) * FI_N2], xa[j], acc);
      }
      const int n0 = 16 * jn + 4 * q;
      *reinterpret_cast<f32x4*>(h2 + r * FI_H2LD + n0) = bias_relu(acc, a.fb2 + n0);
    }
    lds_barrier();                         // h2 complete
    // ---- fc3 (wave 0): lane (q, r) holds logits 4q .. 4q + 3 of image r; weight columns >= 10 are zero ----
    if (w == 0) {
      const float* wp = a.fw3 + (4 * q) * 10 + min(r, 9);
      f32x4 acc = zero4();
#pragma unroll
      for (int s = 0; s < FI_N2 / 16; ++s) {
        const f32x4 xa = lds4(h2 + r * FI_H2LD + 16 * s + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float wv = wp[(16 * s + j) * 10];
          acc = mfma_f32(r < 10 ? wv : 0.f, xa[j], acc);
        }
      }
      const int n = tile * FI_TM + r;        // the lane's image
      const bool valid = r < nv;
      float best = -INFINITY;
      int bi = 64;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 4 * q + i;
        float v = acc[i] + a.fb3[min(k, 9)];
        if (a.relu_logits) v = fmaxf(v, 0.f);
        if (k < 10) {
          if (valid) a.logits[(size_t)n * 10 + k] = v;
          if (v > best) { best = v; bi = k; }              // strict: the first maximum
        }
      }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {                  // over the image's four lanes; ties -> smaller index
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (valid && q == 0) {
        if (a.pred) a.pred[n] = bi;
        if (a.correct) a.correct[n] = bi == a.labels[row_of(n)] ? 1 : 0;
      }
    }
    lds_barrier();                         // h2 read: the next tile's p1 halo and crop overwrite the fc map
  }
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

hipError_t dmlc_f32_infer_grid(int N, int blocks, int* grid) {
  if (N < 1 || blocks < 0) return hipErrorInvalidValue;
  if (blocks == 0) {                       // one workgroup per CU
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&blocks, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (blocks < 1) blocks = 1;
  }
  const int tiles = (N + FI_TM - 1) / FI_TM;
  *grid = tiles < blocks ? tiles : blocks;
  return hipSuccess;
}

hipError_t dmlc_f32_infer(const DmlcF32InferArgs* a, hipStream_t s) {
  if (a->N < 1 || a->nrows < 1 || a->blocks < 0 || (a->correct && !a->labels)) return hipErrorInvalidValue;
  if (a->cy < 0 || a->cy > 8 || a->cx < 0 || a->cx > 8) return hipErrorInvalidValue;
  int grid = 0;
  const hipError_t e = dmlc_f32_infer_grid(a->N, a->blocks, &grid);
  if (e != hipSuccess) return e;
  if (a->scratch_slabs < grid) return hipErrorInvalidValue;   // one slab per workgroup
  DMLC_LDS_OPTIN(&k_cnn_infer_f32, FI_LDS);
  hipLaunchKernelGGL(k_cnn_infer_f32, dim3(grid), dim3(FI_NT), FI_LDS, s, *a);
  return hipGetLastError();
}

}  // extern "C"
