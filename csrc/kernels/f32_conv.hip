// Direct conv2 of the fp32 training step (--dtype fp32, ops/f32.py conv_same(impl="direct" / "direct_all")):
// the stride-1 TF-SAME 5x5 convolution of an fp32 NHWC [B][12][12][64] tensor with 64 output channels, forward,
// data gradient and (further down) weight gradient, in true fp32 on v_mfma_f32_16x16x4_f32 for gfx950.
// Forward and data gradient: M = 144 pixels per image, N = 64, K = 1600.
//
//   k_f32_conv2<false>  y  = conv(x, W) (+ bias)             W = the HWIO weight viewed [1600][64]
//   k_f32_conv2<true>   dx = conv(dy, W'), W'[kh][kw][co][ci] = W[4-kh][4-kw][ci][co], the SAME tensor read in
//                       place (conv2_wfrag<true>): no flipped or transposed copy exists.
// No ReLU either way: relu_pool (f32_pool.hip) consumes the raw conv output.
//
// Work split.  A 512-thread workgroup owns whole images and loops over them (image = blockIdx.x, +=
// gridDim.x; grid = min(B, blocks or the CU count); the LDS map allows one workgroup per CU).  No workgroup
// reads what another wrote: no flags, no counters, no spins; the only synchronisation is the workgroup
// barrier, twice per image.  Wave (h, nt) = (w & 1, w >> 1) takes channel tile nt over all nine 4x4 pixel
// tiles for K half h (chunks 50h .. 50h + 49 of 16 k, the split of k_cnn_infer_f32's conv2_half in eval
// mode): 36 accumulator registers, 1800 MFMAs on every wave, every weight fetched once per image and CU
// straight from L2 into first-operand registers, two chunks ahead of use.  Half 1 parks its sums in the LDS
// exchange buffer; after the barrier half 0 computes (half 0 + half 1) + bias -- a fixed order, so a result
// depends on neither B, the grid nor the image's place in the batch -- and stores 4 consecutive channels of
// one pixel per lane, 16 bytes.
//
// Input through LDS.  The image goes into the zero-padded [16][16][64] fp32 buffer p1 under the p1_off chunk
// swizzle (the sixteen 16-B channel chunks of a pixel XORed with (x & 3) | (y & 3) << 2: the nine 16-byte
// fragment reads of a chunk are conflict-free at every tile and tap, see f32_infer.hip).  The 2304 16-byte
// pieces of an image are 4.5 per thread: global loads and LDS stores are 16 bytes wide.  The halo (rows /
// columns 0, 1, 14, 15) is zeroed once per workgroup: every image overwrites exactly the interior.  The next
// image's 36 KB is requested into 5 x 4 registers BEFORE the current image's MFMA loop and stored to p1 after
// the barrier that ends it (two 64 KB image buffers do not fit beside the exchange buffer in 160 KB); a
// workgroup's last image re-requests itself instead (cached, not stored), so the loop has no branch around
// the loads.  The read-ahead does not spill (resource use below).
//
// LDS, bytes: [0, 65,536) p1, [65,536, 107,008) exchange buffer [144][72] (the pixel pitch of
// k_cnn_infer_f32's conv2 output; 18 16-byte accesses per lane and image against 1800 MFMAs).
//
// gfx950 resource use (hipcc -O3 -Rpass-analysis=kernel-resource-usage; built WITH the no-packed-fp32 flag,
// _build.py HIP_FILE_FLAGS: the epilogue's 4-wide sums stay scalar v_add_f32, so a value cannot depend on how
// the compiler paired them):
//   k_f32_conv2<false>  156 VGPRs, 0 AGPRs, 55 SGPRs, 107,008 B LDS (dynamic), no scratch, no spills
//   k_f32_conv2<true>   156 VGPRs, 0 AGPRs, 64 SGPRs, 107,008 B LDS (dynamic), no scratch, no spills
//
// k_f32_conv2_wgrad + k_f32_wgrad_reduce (conv_same(impl="direct_all")): the third role, conv2's weight and
// bias gradient out[1601][64], rows (kh*5 + kw)*64 + ci = dW[kh][kw][ci][:] = sum over (b, y, x) of
// xpad[b][y+kh][x+kw][ci] dy[b][y][x][:], row 1600 = db = sum dy: M = 1600, N = 64, K = 144 B on the same MFMA.
//
// Fragments.  k = four pixels of a row (q = lane >> 4 picks the pixel), r = lane & 15.  The first operand of
// tile j is word j of channel chunk r of the shifted x pixel (input channel 4 r + j), the second operand of
// role j' word j' of chunk r of the dy pixel (output channel 4 r + j'): accumulator v of lane (q, r) is
// dW[ci = 16 q + 4 v + j][co = 4 r + j'].  The channel-to-tile-row permutation costs nothing; the reduction's
// store address undoes it.
//
// Work split.  Grid = 4 roles x G image groups (G = CUs / 4 by default, at most B: one 512-thread workgroup
// per CU; 4 images each at B = 256, 2 at B = 128).  A workgroup owns output channels {4 r + role} for all 25
// taps and 64 input channels -- 100 tiles, 400 accumulator registers over its 8 waves -- and loops over the
// images g, g + G, ...  Wave (h, j) = (w >> 2, w & 3) takes input-channel tile j and taps 13 h .. 13 h + 12 - h:
// 52 / 48 accumulator registers, and the two waves of a SIMD (w, w + 4) issue 13 + 12 MFMAs per pixel group,
// 900 per image and SIMD, with 13 / 12 independent accumulators back to back.  The 36 dy values of a lane
// and image come straight from global memory into registers (4-byte loads, the next image's before the MFMA
// loop) and are shared by all taps; db is their plain sum per lane (every wave has them; wave 0 adds the
// four pixel lanes in order and stores).  No workgroup reads what another wrote: no flags, no atomics.
//
// Input through LDS.  The x image goes zero-padded into FOUR channel planes [16][16][16] fp32 (plane j = word
// j of every 16-byte chunk): lane (q, r) of wave (h, j) reads word 16 * (pixel + q) + r of plane j, so a
// wave's 64 lanes read 64 consecutive words -- conflict-free at every tap and group, where the 4-byte read of
// word j under the p1_off swizzle is 4-way conflicted (tools/lds_banks.py) -- and every tap is an immediate
// offset.  ConvImage fetches 16 bytes per piece as above and put_planes scatters the four words (64
// consecutive words per wave and plane).  Two image buffers: the next image, requested before the MFMA loop,
// is stored into the other buffer after it, one barrier per image; both halos are zeroed once.
// LDS, bytes: [0, 65,536) buffer 0 = planes 0 .. 3 of 16,384 each, [65,536, 131,072) buffer 1.
//
// Reduction.  Each wave stores its tiles once as they lie in the registers, 1 KB per store, into the group's
// partial ws[g] = [role][tap][j][lane] 16-byte units + 64 bias sums (409,856 B per group, 26 MB at G = 64).
// k_f32_wgrad_reduce (a second launch: it reads exactly the G partials this call wrote) sums a unit over the
// groups in four quarters of consecutive groups, each in group order, adds the quarter sums in order through
// LDS and stores the four values at their dW rows: a fixed order for a fixed (B, G), bit-reproducible.
//
// gfx950 resource use (same flags):
//   k_f32_conv2_wgrad   250 VGPRs, 0 AGPRs, 38 SGPRs, 131,072 B LDS (dynamic), no scratch, no spills
//   k_f32_wgrad_reduce   64 VGPRs, 0 AGPRs, 24 SGPRs,   3,072 B LDS, no scratch, no spills
#include <algorithm>

#include "common.h"
#include "api_f32.h"
#include "f32_conv_core.h"

namespace dmlc {

constexpr int FC_NT = 512;                                   // threads
constexpr int FC_IMG = 144 * 64, FC_PIECES = FC_IMG / 4;      // floats / 16-byte pieces of an image
constexpr int FC_IT = (FC_PIECES + FC_NT - 1) / FC_NT;        // pieces per thread, rounded up: 5
constexpr int FC_XLD = 72;                                   // exchange buffer pixel pitch
constexpr int FC_P1 = 0, FC_XB = FC_P1 + 256 * 64 * 4, FC_LDS = FC_XB + 144 * FC_XLD * 4;
static_assert(FC_LDS <= 160 * 1024 && FC_XB % 16 == 0 && (FC_PIECES - (FC_IT - 1) * FC_NT) % 64 == 0,
              "f32_conv LDS map; the last staging round ends on a wave boundary");
// k_f32_conv2_wgrad: one channel plane of the padded image (floats), its two image buffers, and a group's
// partial in 16-byte units: [role][tap][j][lane] accumulator vectors, then the 64 bias sums [role][r]
constexpr int WG_PLANE = 256 * 16, WG_BUF = 4 * WG_PLANE, WG_LDS = 2 * WG_BUF * 4;
constexpr int WG_ROLES = 4, WG_RT = 100 * 64, WG_PART4 = WG_ROLES * WG_RT + 16, WG_RNT = 256;
static_assert(WG_LDS <= 160 * 1024, "f32 wgrad LDS map");

// One image on its way from memory to p1: piece e = 16 * pixel + chunk, thread t holds pieces t + 512 u.
struct ConvImage {
  f32x4 v[FC_IT];
  MDEV void fetch(const float* img, int t) {
#pragma unroll
    for (int u = 0; u < FC_IT; ++u)                            // a piece past the image re-reads the last one
      v[u] = reinterpret_cast<const f32x4*>(img)[min(t + u * FC_NT, FC_PIECES - 1)];
  }
  MDEV void put(float* p1, int t) const {
#pragma unroll
    for (int u = 0; u < FC_IT; ++u) {
      const int e = t + u * FC_NT, pix = e >> 4, py = pix / 12, px = pix - 12 * py;
      if (e < FC_PIECES) *reinterpret_cast<f32x4*>(p1 + p1_off(py + 2, px + 2, e & 15)) = v[u];
    }
  }
  // the same pieces into the four channel planes of k_f32_conv2_wgrad: word j of chunk c goes to word c of
  // the pixel in plane j (a wave's 64 lanes are 4 pixels of one row: 64 consecutive words per store)
  MDEV void put_planes(float* pl, int t) const {
#pragma unroll
    for (int u = 0; u < FC_IT; ++u) {
      const int e = t + u * FC_NT, pix = e >> 4, py = pix / 12, px = pix - 12 * py;
      float* o = pl + ((py + 2) * 16 + px + 2) * 16 + (e & 15);
      if (e < FC_PIECES) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j * WG_PLANE] = v[u][j];
      }
    }
  }
};

// The first-operand fragments of chunks cc, cc + 1 (cc even; chunk = (tap cc >> 2, k 16 (cc & 3) .. + 15)) for
// output channel 16 nt + r: d[4u + j] = weight at k = 16 g + 4 q + j of chunk cc + u.
//   forward  W viewed [1600][64]: k is the row, the lane's channel the contiguous index -- 8 4-byte loads,
//            16 lanes a 64-B segment.
//   DGRAD    tap (kh, kw) uses W[4-kh][4-kw][ci][co] with ci = the OUTPUT channel and co = k, so k is the
//            contiguous index and a chunk's four k values are ONE 16-byte load from row ci = 16 nt + r of
//            tap 24 - tap.
template <bool DGRAD>
DEV void conv2_wfrag(const float* W, int cc, int nt, int q, int r, float (&d)[8]) {
  if constexpr (DGRAD) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = cc + u, tap = c >> 2, g = c & 3;
      const f32x4 v = *reinterpret_cast<const f32x4*>(W + ((24 - tap) * 64 + 16 * nt + r) * 64 + 16 * g + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[4 * u + j] = v[j];
    }
  } else {
    const float* wp = W + (4 * q) * 64 + 16 * nt + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = wp[(16 * cc + 4 * (j & 4) + (j & 3)) * 64];
  }
}

// The 72 MFMAs of chunks cc, cc + 1 over the 9 pixel tiles: per chunk 9 16-byte activation reads (channels
// 16 g + 4 q .. + 3 of the lane's pixel at the tap, every tile), then k-steps j = 0 .. 3.
DEV void conv2_pair(const float* p1, int cc, int q, int r, const float (&b)[8], f32x4 (&acc)[9]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = cc + u, tap = c >> 2, g = c & 3, kh = tap / 5, kw = tap - 5 * kh;
    const float* xp = p1 + p1_off((r >> 2) + kh, (r & 3) + kw, 4 * g + q);
    f32x4 xa[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) xa[t] = lds4(xp + p1_tile(t));
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = mfma_f32(b[4 * u + j], xa[t][j], acc[t]);
  }
}

// One K half (chunks c0 .. c0 + 49, 25 pairs) for channel tile nt: the summation order of k_cnn_infer_f32's
// conv2_half.  The weights alternate between two register sets, each requested one pair (72 MFMAs) before
// its first use; the scheduling barriers keep the compiler from sinking a request down to its use (it did,
// with a copy between the sets: a full L2 round trip per pair in front of the MFMAs).
template <bool DGRAD>
DEV void conv2_khalf(const float* W, const float* p1, int c0, int nt, int q, int r, f32x4 (&acc)[9]) {
  float ba[8], bb[8];
  conv2_wfrag<DGRAD>(W, c0, nt, q, r, ba);
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = zero4();
  for (int i = 0; i < 48; i += 4) {
    conv2_wfrag<DGRAD>(W, c0 + i + 2, nt, q, r, bb);
    __builtin_amdgcn_sched_barrier(0);
    conv2_pair(p1, c0 + i, q, r, ba, acc);
    __builtin_amdgcn_sched_barrier(0);
    conv2_wfrag<DGRAD>(W, c0 + i + 4, nt, q, r, ba);
    __builtin_amdgcn_sched_barrier(0);
    conv2_pair(p1, c0 + i + 2, q, r, bb, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  conv2_pair(p1, c0 + 48, q, r, ba, acc);
}

template <bool DGRAD>
__global__ __launch_bounds__(FC_NT, 1) void k_f32_conv2(const float* __restrict__ x, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, float* __restrict__ y, int B) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* p1 = reinterpret_cast<float*>(smem + FC_P1);
  float* xb = reinterpret_cast<float*>(smem + FC_XB);
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), q = lane >> 4, r = lane & 15;
  const int h = w & 1, nt = w >> 1;

  ConvImage im;
  im.fetch(x + (size_t)blockIdx.x * FC_IMG, tid);
  for (int e = tid; e < 256 * 16; e += FC_NT) {                // the halo, once: zeros
    const int pix = e >> 4, py = pix >> 4, px = pix & 15;
    if (py < 2 || py >= 14 || px < 2 || px >= 14) *reinterpret_cast<f32x4*>(p1 + pix * 64 + 4 * (e & 15)) = zero4();
  }
  im.put(p1, tid);
  lds_barrier();

  const int pl = (r >> 2) * 12 + (r & 3), ch = 16 * nt + 4 * q;   // the lane's pixel in a tile, its 4 channels
  float* o = xb + pl * FC_XLD + ch;
  for (int n = blockIdx.x; n < B; n += gridDim.x) {
    const int nn = n + gridDim.x;                              // the workgroup's next image (wave-uniform)
    const bool more = nn < B;
    im.fetch(x + (size_t)(more ? nn : n) * FC_IMG, tid);
    f32x4 acc[9];
    conv2_khalf<DGRAD>(wt, p1, 50 * h, nt, q, r, acc);
    if (h == 1) {
#pragma unroll
      for (int t = 0; t < 9; ++t) *reinterpret_cast<f32x4*>(o + out_tile(t) * FC_XLD) = acc[t];
    }
    lds_barrier();                         // every wave is past its p1 reads; half 1's sums are parked
    if (more) im.put(p1, tid);
    if (h == 0) {
      const bool hb = !DGRAD && bias != nullptr;
      const f32x4 bv = hb ? *reinterpret_cast<const f32x4*>(bias + ch) : zero4();
      float* yo = y + (size_t)n * FC_IMG + pl * 64 + ch;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        f32x4 v = acc[t] + lds4(o + out_tile(t) * FC_XLD);
        if (hb) v = v + bv;
        *reinterpret_cast<f32x4*>(yo + out_tile(t) * 64) = v;
      }
    }
    lds_barrier();                         // the next image is in p1; the exchange buffer is read
  }
}

// ---- k_f32_conv2_wgrad: see the header -------------------------------------------------------------------

// The lane's 36 dy values of one image, one per four-pixel group p = (row p / 3, columns 4 (p % 3) .. + 3);
// dyl = the image + the lane's (q * 64 + 4 r + role).
DEV void wgrad_dy(const float* dyl, float (&d)[36]) {
#pragma unroll
  for (int p = 0; p < 36; ++p) d[p] = dyl[((p / 3) * 12 + 4 * (p % 3)) * 64];
}

// One image's MFMAs of tap set H (taps 13 H .. 13 H + NT - 1, NT = 13 - H): per pixel group the NT shifted
// one-word reads of the lane's plane (pl = plane j + lane: every offset is an immediate) against d[p];
// NT independent accumulators back to back.  bs: the lane's running sum of dy (bias gradient).
template <int H>
DEV void wgrad_image(const float* pl, const float (&d)[36], f32x4 (&acc)[13], float& bs) {
  constexpr int T0 = 13 * H, NT = 13 - H;
  float a[2][NT];                                              // group p + 1 is read under group p's MFMAs
#pragma unroll
  for (int p = -1; p < 36; ++p) {
    const int y = (p + 1) / 3, gx = 4 * ((p + 1) % 3);
    if (p + 1 < 36) {
#pragma unroll
      for (int i = 0; i < NT; ++i) a[(p + 1) & 1][i] = pl[((y + (T0 + i) / 5) * 16 + gx + (T0 + i) % 5) * 16];
    }
    if (p >= 0) {
      bs += d[p];
#pragma unroll
      for (int i = 0; i < NT; ++i) acc[i] = mfma_f32(a[p & 1][i], d[p], acc[i]);
    }
    __builtin_amdgcn_sched_barrier(0);                         // no further read-ahead: it spilled
  }
}

__global__ __launch_bounds__(FC_NT, 1) void k_f32_conv2_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ ws, int B, int G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pl = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), q = lane >> 4, r = lane & 15;
  const int h = w >> 2, j = w & 3;                             // waves w, w + 4 share a SIMD: 13 + 12 taps each
  // (group, role) of the workgroup.  Workgroups go round-robin over the 8 XCDs: with G a multiple of 8 the
  // four roles of a group are 8 apart, so they read their images through one L2.
  const int b = blockIdx.x, xcd = (G & 7) == 0;
  const int g = xcd ? (b & 7) | ((b >> 5) << 3) : b >> 2, role = xcd ? (b >> 3) & 3 : b & 3;

  ConvImage im;
  im.fetch(x + (size_t)g * FC_IMG, tid);
  const float* dyl = dy + (q * 64 + 4 * r + role);
  float d[36], dn[36];
  wgrad_dy(dyl + (size_t)g * FC_IMG, d);
  for (int e = tid; e < 2 * WG_BUF / 4; e += FC_NT) {          // the halo of both buffers, once: zeros
    const int pix = (e >> 2) & 255, py = pix >> 4, px = pix & 15;
    if (py < 2 || py >= 14 || px < 2 || px >= 14) *reinterpret_cast<f32x4*>(pl + 4 * e) = zero4();
  }
  im.put_planes(pl, tid);
  lds_barrier();

  f32x4 acc[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) acc[i] = zero4();
  float bs = 0.f;
  int buf = 0;
  for (int n = g; n < B; n += G) {
    const int nn = n + G;                                      // the group's next image (wave-uniform)
    const bool more = nn < B;
    const size_t nx = (size_t)(more ? nn : n) * FC_IMG;        // the last image re-requests itself (cached)
    im.fetch(x + nx, tid);
    wgrad_dy(dyl + nx, dn);
    __builtin_amdgcn_sched_barrier(0);                         // the requests stay in front of the MFMA loop
    const float* src = pl + buf * WG_BUF + j * WG_PLANE + lane;
    if (h == 0) wgrad_image<0>(src, d, acc, bs);
    else wgrad_image<1>(src, d, acc, bs);
    __builtin_amdgcn_sched_barrier(0);
    if (more) im.put_planes(pl + (buf ^ 1) * WG_BUF, tid);     // the buffer every wave left at the last barrier
#pragma unroll
    for (int p = 0; p < 36; ++p) d[p] = dn[p];
    lds_barrier();
    buf ^= 1;
  }

  // the wave's tiles as they lie in the registers: 1 KB per store (k_f32_wgrad_reduce undoes the permutation)
  f32x4* o = reinterpret_cast<f32x4*>(ws) + (size_t)g * WG_PART4 + role * WG_RT + j * 64 + lane;
#pragma unroll
  for (int i = 0; i < 13; ++i)
    if (i < 13 - h) o[(13 * h + i) * 256] = acc[i];
  if (w == 0) {                                                // db: the four pixel lanes of a channel, in order
    const float s = ((__shfl(bs, r) + __shfl(bs, r + 16)) + __shfl(bs, r + 32)) + __shfl(bs, r + 48);
    if (q == 0) ws[((size_t)g * WG_PART4 + WG_ROLES * WG_RT) * 4 + role * 16 + r] = s;
  }
}

// out[1601][64] = the sum of the G partials.  Thread (k, c) of a workgroup sums the 16-byte unit
// p = 64 blockIdx.x + c over quarter k of the groups (groups k * ceil(G / 4) ..., in order); thread (0, c)
// then adds the four quarter sums in order and stores the four values where they belong: unit
// [role][tap][j][lane] holds dW rows tap * 64 + 16 q + 4 v + j, v = 0 .. 3, at column 4 r + role.
__global__ __launch_bounds__(WG_RNT) void k_f32_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ out,
                                                            int G) {
  __shared__ f32x4 sm[3][64];
  const int tid = threadIdx.x, c = tid & 63, k = tid >> 6, p = blockIdx.x * 64 + c;
  const int per = (G + 3) >> 2, g0 = k * per, g1 = min(G, g0 + per);
  f32x4 s = zero4();
  if (p < WG_PART4) {
    const f32x4* src = reinterpret_cast<const f32x4*>(ws) + p;
#pragma unroll 8
    for (int g = g0; g < g1; ++g) s = s + src[(size_t)g * WG_PART4];
  }
  if (k) sm[k - 1][c] = s;
  __syncthreads();
  if (k || p >= WG_PART4) return;
  s = ((s + sm[0][c]) + sm[1][c]) + sm[2][c];
  if (p < WG_ROLES * WG_RT) {
    const int lane = p & 63, j = (p >> 6) & 3, rt = p >> 8, role = rt / 25, t = rt - 25 * role;
    float* o = out + (t * 64 + 16 * (lane >> 4) + j) * 64 + 4 * (lane & 15) + role;
#pragma unroll
    for (int v = 0; v < 4; ++v) o[v * 4 * 64] = s[v];
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = 4 * (p - WG_ROLES * WG_RT) + v;              // bias sum [role i >> 4][r i & 15]
      out[1600 * 64 + 4 * (i & 15) + (i >> 4)] = s[v];
    }
  }
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

hipError_t dmlc_f32_conv2(const float* x, const float* w, const float* bias, float* y, int B, int dgrad, int blocks,
                          hipStream_t s) {
  if (B < 1 || B > (1 << 20) || blocks < 0 || (dgrad && bias)) return hipErrorInvalidValue;
  if (blocks == 0) {                       // one workgroup per CU
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&blocks, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (blocks < 1) blocks = 1;
  }
  const int grid = std::min(B, blocks);
  if (dgrad) {
    DMLC_LDS_OPTIN(&k_f32_conv2<true>, FC_LDS);
    hipLaunchKernelGGL(k_f32_conv2<true>, dim3(grid), dim3(FC_NT), FC_LDS, s, x, w, bias, y, B);
  } else {
    DMLC_LDS_OPTIN(&k_f32_conv2<false>, FC_LDS);
    hipLaunchKernelGGL(k_f32_conv2<false>, dim3(grid), dim3(FC_NT), FC_LDS, s, x, w, bias, y, B);
  }
  return hipGetLastError();
}

hipError_t dmlc_f32_conv2_wgrad_plan(int B, int groups, int* G, size_t* ws_floats) {
  if (B < 1 || B > (1 << 20) || groups < 0) return hipErrorInvalidValue;
  if (groups == 0) {                       // one workgroup per CU: CUs / roles groups
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    groups = std::max(1, cus / WG_ROLES);
  }
  *G = std::min(B, groups);                // every group has an image: no partial stays unwritten
  *ws_floats = (size_t)*G * WG_PART4 * 4;
  return hipSuccess;
}

hipError_t dmlc_f32_conv2_wgrad(const float* x, const float* dy, float* out, float* ws, int B, int groups,
                                hipStream_t s) {
  int G = 0;
  size_t n = 0;
  const hipError_t e = dmlc_f32_conv2_wgrad_plan(B, groups, &G, &n);
  if (e != hipSuccess) return e;
  if (!x || !dy || !out || !ws) return hipErrorInvalidValue;
  DMLC_LDS_OPTIN(&k_f32_conv2_wgrad, WG_LDS);
  hipLaunchKernelGGL(k_f32_conv2_wgrad, dim3(WG_ROLES * G), dim3(FC_NT), WG_LDS, s, x, dy, ws, B, G);
  hipLaunchKernelGGL(k_f32_wgrad_reduce, dim3((WG_PART4 + 63) / 64), dim3(WG_RNT), 0, s, ws, out, G);
  return hipGetLastError();
}

}  // extern "C"
