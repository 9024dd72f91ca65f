// conv1's backward of the fp32 training step (--dtype fp32, ops/f32.py CONV1_IMPL_F32 = "direct"): the weight
// and bias gradient of the stride-1 TF-SAME 5x5 convolution of the image x, fp32 NHWC [B][24][24][3], with 64
// output channels, in true fp32 on v_mfma_f32_16x16x4_f32 for gfx950.  conv1 has no data gradient (its input
// is the image), so this is the stage's whole backward: M = 76, N = 64, K = 576 B.
//
//   out[76][64]: row (kh*5 + kw)*3 + ci = dW1[kh][kw][ci][:] = sum over (b, y, x) of xpad[b][y+kh][x+kw][ci] dy[b][y][x][:]
//                row 75 = db1 = sum dy        (the layout of the implicit GEMM's weight gradient with the ones column)
//
//   k_f32_conv1_wgrad<false>  dy [B][24][24][64] is read from memory (the fused=False path)
//   k_f32_conv1_wgrad<true>   dy is REBUILT in LDS from the pooled gradient dp [B][12][12][64] and the one-byte
//                             argmax of k_f32_relu_pool_fwd (kh*3 + kw, 255 = masked by the ReLU): the ReLU +
//                             pool backward and the weight gradient in one launch; dy never exists in memory.
//   k_f32_conv1_reduce        sums the workgroups' partials in a fixed order (a second launch).
// The two forms share everything but the code that fills a band of dy (C1BandDense / C1BandPool).
//
// Fragments.  k = four consecutive pixels of a row (q = lane >> 4 picks the pixel), r = lane & 15.  M = 76 is
// padded to five row tiles: the first operand of tile t is im2col row m = 16 t + r of the lane's pixel, one
// word of the zero-padded image at the loop-invariant offset (kh*28 + kw)*3 + ci (+ 4 pad words per row, below)
// plus 3 words per pixel; row 75 is the constant 1 (its output row is db), rows 76 .. 79 are 0 and are not
// stored.  The second operand is dy[pixel][16 nt + r].  Accumulator v of lane (q, r): out[16 t + 4 q + v][16 nt + r].
//
// Work split.  Grid = G image groups (G = the CU count by default, at most B: every group owns an image), one
// 512-thread workgroup each, looping over the images g, g + G, ... and, per image, over four BANDS of six dy
// rows (three pooled rows).  Wave (h, nt) = (w >> 2, w & 3) owns output-channel tile nt for all five row tiles
// -- 5 independent accumulators, 20 registers, one dy word feeds 5 MFMAs -- and the two waves of a SIMD
// (w, w + 4) take alternate pixel groups: k-step ks = 6 row + group of the band's 36 goes to wave h = ks & 1,
// 18 x 5 = 90 MFMAs per wave and band, the operands of step i + 1 read under the MFMAs of step i.  The sums
// run over a group's bands and images in order; at the end the h = 1 waves park their tiles in LDS and the
// h = 0 waves store (h0 + h1), 1 KB per store.  No workgroup reads what another wrote in a launch: no flags,
// no atomics, no spins; one workgroup barrier per band.
//
// LDS, 4-byte words ([0, 4,928) x, [4,928, 23,488) dy; 93,952 B, dynamic):
//   x    two buffers (image n / the group's next image) of the zero-padded image [28][88]: 28 x 3 = 84 words
//        of a row + 4.  With the pitch 88 a wave's 64 one-word first-operand reads -- words m + 73 kh + 3 q,
//        m = 16 t .. 16 t + 15 -- touch every bank at most once in tiles 0 .. 3 (equal words are one
//        broadcast); the plain pitch 84 is 2-way conflicted wherever a tile spans two kernel rows
//        (tools/lds_banks.py: 1.06 passes per read on average against 1.86; what is left is tile 4, whose
//        replaced lanes read word 0 against the others' words in 31 % of its reads).  Both buffers are
//        zeroed once; an image overwrites exactly the interior.
//   dy   two band buffers of four channel-tile planes [144 pixels][16] + 16 words of pad: lane (q, r) of a
//        wave reads word 16 (pixel + q) + r of plane nt, 64 consecutive words, conflict-free at every
//        step; the plane pad spreads the 16-byte band stores of a pixel's 16 channel quads over all banks.
//        After the last band the first buffer is the h = 1 waves' exchange buffer (20,480 B).
// The next band (and, at an image's last band, the group's next image) is requested into registers BEFORE the
// MFMA loop and stored into the other buffer after it; a group's last band re-requests itself (cached, not
// stored), so the loop has no branch around the loads.
//
// Pool form.  Window (i, j) of the pooled gradient owns dy pixels (2i + a, 2j + b), which receive gradient
// only from the windows UL, U, L and W at fixed argmax values -- the ownership rule and the summation order
// ((UL + U) + L) + W of k_f32_relu_pool_bwd (f32_pool.hip), so the band is bit-identical to that kernel's
// output.  A band is 3 x 12 windows x 16 channel quads = 576 items: thread t takes item t, and wave 0 item
// 512 + t too.  An item's four dp quads and argmax words come straight from global memory (L2 / L1 hits for
// three of the four) into 20 registers.  The argmax byte selects by comparison, never as an address.
//
// Reduction.  ws[g] = [nt][t][lane] 16-byte accumulator vectors, 20,480 B per group (5 MB at G = 256).
// k_f32_conv1_reduce: thread (k, c) sums unit 16 blockIdx.x + c over sixteenth k of the groups in group order,
// thread (0, c) adds the sixteen sums in order through LDS and stores the four values at their rows: a fixed
// order for a fixed (B, G), bit-reproducible.
//
// gfx950 resource use (hipcc -O3 -Rpass-analysis=kernel-resource-usage, built WITH the no-packed-fp32 flag,
// _build.py HIP_FILE_FLAGS, so the pool form's sums are the scalar v_add_f32 of k_f32_relu_pool_bwd):
//   k_f32_conv1_wgrad<false>  110 VGPRs, 0 AGPRs, 40 SGPRs, 93,952 B LDS (dynamic), no scratch, no spills
//   k_f32_conv1_wgrad<true>   142 VGPRs, 0 AGPRs, 46 SGPRs, 93,952 B LDS (dynamic), no scratch, no spills
//   k_f32_conv1_reduce         63 VGPRs, 0 AGPRs, 22 SGPRs,  3,840 B LDS, no scratch, no spills
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "api_f32.h"
#include "f32_conv_core.h"

namespace dmlc {

constexpr int C1_NT = 512;                                    // threads
constexpr int C1_XIMG = 24 * 24 * 3, C1_XPIECES = C1_XIMG / 4;  // floats / 16-byte pieces of an image: 1728 / 432
constexpr int C1_XP = 88, C1_XBUF = 28 * C1_XP;               // padded-row pitch and one x buffer, words
constexpr int C1_BPIX = 6 * 24, C1_BPIECES = C1_BPIX * 16;    // pixels / 16-byte pieces of a dy band: 144 / 2304
constexpr int C1_BIT = (C1_BPIECES + C1_NT - 1) / C1_NT;      // pieces per thread, rounded up: 5
constexpr int C1_PLANE = C1_BPIX * 16 + 16, C1_BAND = 4 * C1_PLANE;   // one channel-tile plane, one band buffer
constexpr int C1_X = 0, C1_DY = 2 * C1_XBUF, C1_LDS = (C1_DY + 2 * C1_BAND) * 4;
constexpr int C1_STEPS = 18;                                  // k-steps of a wave per band
constexpr int C1_PART4 = 4 * 5 * 64;                          // a group's partial in 16-byte units: [nt][t][lane]
constexpr int C1_RNT = 256;                                   // threads of the reduction: 16 parts x 16 units
static_assert(C1_LDS <= 160 * 1024 && (C1_DY * 4) % 16 == 0 && (C1_PLANE * 4) % 16 == 0, "f32 conv1 LDS map");
static_assert(C1_PART4 * 4 <= C1_BAND && C1_PART4 % 16 == 0, "the exchange buffer fits a band buffer");
static_assert((C1_BPIECES - (C1_BIT - 1) * C1_NT) % 64 == 0, "the last staging round ends on a wave boundary");
static_assert(27 * C1_XP + 27 * 3 + 2 < C1_XBUF, "the last tap of the last pixel is inside the x buffer");

// One x image on its way to LDS: thread t < 432 holds 16 bytes = words 4 (t % 18) .. + 3 of image row t / 18.
struct C1Image {
  f32x4 v;
  MDEV void fetch(const float* img, int t) { v = reinterpret_cast<const f32x4*>(img)[min(t, C1_XPIECES - 1)]; }
  MDEV void put(float* xb, int t) const {
    if (t < C1_XPIECES) {
      float* o = xb + (t / 18 + 2) * C1_XP + 6 + 4 * (t % 18);   // padded (row + 2, column 2): 6 words in
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = v[j];
    }
  }
};

// 16-byte address of channel quad c of band pixel pix in a band buffer
DEV f32x4* band_at(float* band, int pix, int c) {
  return reinterpret_cast<f32x4*>(band + (c >> 2) * C1_PLANE + pix * 16 + 4 * (c & 3));
}

// A band of dy (image n, dy rows 6 b4 .. 6 b4 + 5) from memory: 2304 contiguous 16-byte pieces, piece
// e = 16 * pixel + quad, thread t holds pieces t + 512 u.
struct C1BandDense {
  f32x4 v[C1_BIT];
  MDEV void fetch(const float* dy, const uint8_t*, int n, int b4, int t, int) {
    const f32x4* s = reinterpret_cast<const f32x4*>(dy) + ((size_t)n * 4 + b4) * C1_BPIECES;
#pragma unroll
    for (int u = 0; u < C1_BIT; ++u) v[u] = s[min(t + u * C1_NT, C1_BPIECES - 1)];   // past the band: the last piece
  }
  MDEV void put(float* band, int t, int) const {
#pragma unroll
    for (int u = 0; u < C1_BIT; ++u) {
      const int e = t + u * C1_NT;
      if (e < C1_BPIECES) *band_at(band, e >> 4, e & 15) = v[u];
    }
  }
};

// The same band rebuilt from the pooled gradient: item wi = (pooled row il of the band, pooled column j, channel
// quad c) = window (3 b4 + il, j); f / a = dp quad / argmax word of the windows W, L, U, UL (a window that does
// not exist is read at the nearest one that does and its argmax word replaced by NONE: no byte of it matches).
struct C1BandPool {
  static constexpr uint32_t NONE = 0xffffffffu;
  f32x4 f[2][4];
  uint32_t a[2][4];
  MDEV void fetch(const float* dp, const uint8_t* arg, int n, int b4, int t, int w) {
    const f32x4* d4 = reinterpret_cast<const f32x4*>(dp) + (size_t)n * (144 * 16);
    const uint32_t* a4 = reinterpret_cast<const uint32_t*>(arg) + (size_t)n * (144 * 16);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k == 0 || w == 0) {                                  // wave-uniform: items 512 .. 575 are wave 0's
        const int wi = t + k * C1_NT, c = wi & 15, j = (wi >> 4) % 12, i = 3 * b4 + wi / 192;
        const int iu = max(i - 1, 0), jl = max(j - 1, 0);
        const int o[4] = {(i * 12 + j) * 16 + c, (i * 12 + jl) * 16 + c, (iu * 12 + j) * 16 + c, (iu * 12 + jl) * 16 + c};
#pragma unroll
        for (int s = 0; s < 4; ++s) { f[k][s] = d4[o[s]]; a[k][s] = a4[o[s]]; }
        if (j == 0) a[k][1] = a[k][3] = NONE;
        if (i == 0) a[k][2] = a[k][3] = NONE;
      }
    }
  }
  // dp of one window where its argmax byte (channel j of the quad) is d, else 0 (f32_pool.hip pick)
  static MDEV float pick(uint32_t a, int j, uint32_t d, float v) { return ((a >> (8 * j)) & 0xffu) == d ? v : 0.f; }
  MDEV void put(float* band, int t, int w) const {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k == 0 || w == 0) {
        const int wi = t + k * C1_NT, c = wi & 15, j = (wi >> 4) % 12, il = wi / 192;
        const f32x4 &fw = f[k][0], &fl = f[k][1], &fu = f[k][2], &ful = f[k][3];
        const uint32_t aw = a[k][0], al = a[k][1], au = a[k][2], aul = a[k][3];
        f32x4 o[4];                                            // dy pixel (2i + a, 2j + b): o[2a + b]
#pragma unroll
        for (int e = 0; e < 4; ++e) {                          // the expressions of k_f32_relu_pool_bwd, bit for bit
          o[0][e] = ((pick(aul, e, 8, ful[e]) + pick(au, e, 6, fu[e])) + pick(al, e, 2, fl[e])) + pick(aw, e, 0, fw[e]);
          o[1][e] = pick(au, e, 7, fu[e]) + pick(aw, e, 1, fw[e]);
          o[2][e] = pick(al, e, 5, fl[e]) + pick(aw, e, 3, fw[e]);
          o[3][e] = pick(aw, e, 4, fw[e]);
        }
        const int pix = 2 * il * 24 + 2 * j;
        *band_at(band, pix, c) = o[0];
        *band_at(band, pix + 1, c) = o[1];
        *band_at(band, pix + 24, c) = o[2];
        *band_at(band, pix + 25, c) = o[3];
      }
    }
  }
};

// One band's MFMAs of wave half H: k-steps ks = 2 i + H (band row ks / 6, pixels 4 (ks % 6) .. + 3).  xa[t]:
// the lane's first-operand word of tile t at the band's first pixel, bl: its dy word there; every step is an
// immediate offset.  Tile 4 holds rows 64 .. 79: lanes r >= 11 take the constant c4 (1 for the bias row 75,
// else 0) instead of an image word.
template <int H>
DEV void c1_band(const float* const (&xa)[5], const float* bl, bool real4, float c4, f32x4 (&acc)[5]) {
  float a[2][5], b[2];                                         // step i + 1 is read under step i's MFMAs
#pragma unroll
  for (int i = -1; i < C1_STEPS; ++i) {
    if (i + 1 < C1_STEPS) {
      const int ks = 2 * (i + 1) + H, yy = ks / 6, gx = ks % 6;
#pragma unroll
      for (int t = 0; t < 5; ++t) a[(i + 1) & 1][t] = xa[t][yy * C1_XP + 12 * gx];
      b[(i + 1) & 1] = bl[(yy * 24 + 4 * gx) * 16];
    }
    __builtin_amdgcn_sched_barrier(0);                         // the reads go out before the MFMAs, not among them
    if (i >= 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma_f32(a[i & 1][t], b[i & 1], acc[t]);
      acc[4] = mfma_f32(real4 ? a[i & 1][4] : c4, b[i & 1], acc[4]);
    }
    __builtin_amdgcn_sched_barrier(0);                         // one step of read-ahead
  }
}

template <bool POOL>
__global__ __launch_bounds__(C1_NT, 1) void k_f32_conv1_wgrad(const float* __restrict__ x, const float* __restrict__ src,
                                                              const uint8_t* __restrict__ arg, float* __restrict__ ws,
                                                              int B, int G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xb = reinterpret_cast<float*>(smem) + C1_X;
  float* db = reinterpret_cast<float*>(smem) + C1_DY;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), q = lane >> 4, r = lane & 15;
  const int h = w >> 2, nt = w & 3, g = blockIdx.x;            // waves w, w + 4 share a SIMD

  // the lane's im2col word of each row tile at pixel (0, q): (kh * 28 + kw) * 3 + ci under the row pitch
  int oa[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int m = min(16 * t + r, 74), tap = m / 3, kh = tap / 5;
    oa[t] = 16 * t + r < 75 ? kh * C1_XP + (m - 15 * kh) + 3 * q : 0;
  }
  const bool real4 = r < 11;
  const float c4 = r == 11 ? 1.f : 0.f;

  typename std::conditional<POOL, C1BandPool, C1BandDense>::type bd;
  C1Image im;
  im.fetch(x + (size_t)g * C1_XIMG, tid);
  bd.fetch(src, arg, g, 0, tid, w);
  for (int e = tid; e < 2 * C1_XBUF / 4; e += C1_NT) reinterpret_cast<f32x4*>(xb)[e] = zero4();   // both halos, once
  lds_barrier();
  im.put(xb, tid);
  bd.put(db, tid, w);
  lds_barrier();

  f32x4 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) acc[t] = zero4();
  const int units = 4 * ((B - g + G - 1) / G);                 // (image, band) of the group, in order
  for (int u = 0; u < units; ++u) {
    const bool more = u + 1 < units;
    const int un = more ? u + 1 : u, nn = g + (un >> 2) * G, bn = un & 3;   // the last band re-requests itself
    im.fetch(x + (size_t)nn * C1_XIMG, tid);
    bd.fetch(src, arg, nn, bn, tid, w);
    __builtin_amdgcn_sched_barrier(0);                         // the requests stay in front of the MFMA loop
    const float* xl = xb + ((u >> 2) & 1) * C1_XBUF + (u & 3) * 6 * C1_XP;
    const float* const xa[5] = {xl + oa[0], xl + oa[1], xl + oa[2], xl + oa[3], xl + oa[4]};
    const float* bl = db + (u & 1) * C1_BAND + nt * C1_PLANE + lane;
    if (h == 0) c1_band<0>(xa, bl, real4, c4, acc);
    else c1_band<1>(xa, bl, real4, c4, acc);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {                                                // the buffers every wave left at the last barrier
      if (bn == 0) im.put(xb + ((un >> 2) & 1) * C1_XBUF, tid);
      bd.put(db + (un & 1) * C1_BAND, tid, w);
    }
    lds_barrier();
  }

  f32x4* xc = reinterpret_cast<f32x4*>(db) + nt * 5 * 64 + lane;   // every wave is past its last band
  if (h == 1) {
#pragma unroll
    for (int t = 0; t < 5; ++t) xc[t * 64] = acc[t];
  }
  lds_barrier();
  if (h == 0) {
    f32x4* o = reinterpret_cast<f32x4*>(ws) + (size_t)g * C1_PART4 + nt * 5 * 64 + lane;
#pragma unroll
    for (int t = 0; t < 5; ++t) o[t * 64] = acc[t] + xc[t * 64];
  }
}

// out[76][64] = the sum of the G partials: see the header.  Unit p = [nt][t][lane] holds rows
// 16 t + 4 q + v, v = 0 .. 3, of column 16 nt + r.
__global__ __launch_bounds__(C1_RNT) void k_f32_conv1_reduce(const float* __restrict__ ws, float* __restrict__ out, int G) {
  __shared__ f32x4 sm[15][16];
  const int tid = threadIdx.x, c = tid & 15, k = tid >> 4, p = blockIdx.x * 16 + c;   // p < C1_PART4: the grid is exact
  const int per = (G + 15) >> 4, g0 = k * per, g1 = min(G, g0 + per);
  const f32x4* s4 = reinterpret_cast<const f32x4*>(ws) + p;
  f32x4 s = zero4();
#pragma unroll 8
  for (int g = g0; g < g1; ++g) s = s + s4[(size_t)g * C1_PART4];
  if (k) sm[k - 1][c] = s;
  __syncthreads();
  if (k) return;
#pragma unroll
  for (int i = 0; i < 15; ++i) s = s + sm[i][c];
  const int lane = p & 63, tn = p >> 6, nt = tn / 5, t = tn - 5 * nt;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int m = 16 * t + 4 * (lane >> 4) + v;
    if (m < 76) out[m * 64 + 16 * nt + (lane & 15)] = s[v];
  }
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

hipError_t dmlc_f32_conv1_wgrad_plan(int B, int groups, int* G, size_t* ws_floats) {
  if (B < 1 || B > (1 << 20) || groups < 0) return hipErrorInvalidValue;
  if (groups == 0) {                       // one workgroup per CU
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&groups, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (groups < 1) groups = 1;
  }
  *G = std::min(B, groups);                // every group has an image: no partial stays unwritten
  *ws_floats = (size_t)*G * C1_PART4 * 4;
  return hipSuccess;
}

hipError_t dmlc_f32_conv1_wgrad(const float* x, const float* dy, const float* dp, const uint8_t* arg, float* out,
                                float* ws, int B, int groups, hipStream_t s) {
  int G = 0;
  size_t n = 0;
  const hipError_t e = dmlc_f32_conv1_wgrad_plan(B, groups, &G, &n);
  if (e != hipSuccess) return e;
  if (!x || !out || !ws || (dy ? dp || arg : !dp || !arg)) return hipErrorInvalidValue;
  if (dy) {
    DMLC_LDS_OPTIN(&k_f32_conv1_wgrad<false>, C1_LDS);
    hipLaunchKernelGGL(k_f32_conv1_wgrad<false>, dim3(G), dim3(C1_NT), C1_LDS, s, x, dy, arg, ws, B, G);
  } else {
    DMLC_LDS_OPTIN(&k_f32_conv1_wgrad<true>, C1_LDS);
    hipLaunchKernelGGL(k_f32_conv1_wgrad<true>, dim3(G), dim3(C1_NT), C1_LDS, s, x, dp, arg, ws, B, G);
  }
  hipLaunchKernelGGL(k_f32_conv1_reduce, dim3(C1_PART4 / 16), dim3(C1_RNT), 0, s, ws, out, G);
  return hipGetLastError();
}

}  // extern "C"
