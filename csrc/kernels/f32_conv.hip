// Direct conv2 of the fp32 training step (--dtype fp32, ops/f32.py conv_same(impl="direct")): the stride-1
// TF-SAME 5x5 convolution of an fp32 NHWC [B][12][12][64] tensor with 64 output channels, forward and data
// gradient, in true fp32 on v_mfma_f32_16x16x4_f32 for gfx950.  M = 144 pixels per image, N = 64, K = 1600.
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

}  // extern "C"
