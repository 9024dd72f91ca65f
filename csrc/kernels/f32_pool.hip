// The non-GEMM half of the fp32 training step (--dtype fp32, ops/f32.py): ReLU + TF-SAME 3x3/2
// max-pool forward and backward of the two conv stages, and the softmax cross-entropy head.  With
// them the step's forward, backward and loss are HIP from the first conv to dlogits; max, ReLU and
// the argmax are exact, so the forward is bit-identical to relu + max_pool2d.
//
// Pool geometry (both kernels): y is the conv output NHWC [B][H][H][64] (bias added), H = 24 or 12,
// pooled [B][H/2][H/2][64]; window (i, j) covers y rows 2i..2i+2, columns 2j..2j+2, the row / column
// H (TF-SAME pads bottom / right only) is ignored.  A lane owns 4 consecutive channels (one 16-byte
// access), 16 lanes a pixel.  A workgroup of 192 threads takes one UNIT at a time, grid-stride:
//   H = 24: a band of 3 pooled rows of one image (4 units per image) -- thread = (pooled column,
//           channel quad), 12 x 16;
//   H = 12: a whole image (6 pooled rows) -- thread = (half, pooled column, channel quad), 2 x 6 x 16.
// Either way a thread walks DOWN 3 pooled rows of one pooled column.
//
//  * k_f32_relu_pool_fwd: the unit's y rows (7 x 24 or 12 x 12 pixels, 43 / 36 KB) are staged into
//    LDS once, every 16-byte load of a thread issued before its first LDS store (14 / 12 loads in
//    flight per thread); a window's 9 taps are LDS reads, and the y row shared by two consecutive
//    pooled rows stays in registers (3 taps x 4 channels) from one to the next.  Scan order (kh, kw),
//    strict '>' against a running maximum that starts at 0: the result is max(0, window) = pool of
//    relu(y), the argmax is the FIRST maximum, and a window with no positive value keeps the initial
//    255.  A tap in the padding is read clamped to row / column H-1, i.e. it repeats an earlier tap
//    and can never win the strict compare.  NaN taps win (as in PyTorch's pool), so a diverged
//    run stays visible.
//    Argmax byte: kh*3 + kw, 255 = masked by the ReLU -- the convention of conv_common.h (pool_window).
//  * k_f32_relu_pool_bwd: gather form of pool backward + ReLU backward in one pass, "2x2 ownership"
//    as conv_common.h's pool_bwd_2x2: window (i, j) owns y pixels (2i + a, 2j + b), a, b in {0, 1},
//    which receive gradient only from the windows UL (i-1, j-1), U (i-1, j), L (i, j-1) and W (i, j)
//    at fixed argmax values; the sum runs in that order (i ascending, then j).  The unit's dp rows and
//    argmax bytes (plus the pooled row above the band) are staged into LDS once (<= 15 KB); walking
//    down, a thread's W / L of one pooled row are the U / UL of the next and stay in registers.
//    Every dy element is stored exactly once, zeros included: no memset, no atomics, bitwise
//    reproducible.  Neither y nor relu(y) is read: the byte 255 is the ReLU mask.
//  * k_f32_xent_head: mean softmax cross-entropy of logits [B][10] (on relu(logits) with relu_logits),
//    the count of rows whose first maximum is the label, and dlogits = (softmax - onehot) / B (zero
//    where the logit ReLU masked).  One workgroup, one row per thread and round, the row's 10 logits
//    in registers; a thread's partial loss / hit count accumulate in row order, lanes combine in a
//    fixed butterfly and wave partials are summed by wave index: deterministic, no atomics, one
//    launch, any B >= 1.  Labels (int32 or int64) select a register by comparison, never an address.
#include <algorithm>

#include "common.h"
#include "api_f32.h"

namespace dmlc {

constexpr int PT = 192;      // threads of the pool kernels
constexpr int PBAND = 3;     // pooled rows a thread walks
constexpr int PGRID = 2048;  // default cap of the pool kernels' grid (units beyond it: grid-stride)

template <int H>
struct PoolGeom {
  static constexpr int HO = H / 2;
  static constexpr int SUB = PT / (16 * HO);                          // thread groups stacked vertically: 1 / 2
  static constexpr int UROWS = PBAND * SUB;                           // pooled rows of a unit: 3 / 6
  static constexpr int UNITS = HO / UROWS;                            // units per image: 4 / 1
  static constexpr int YROWS = 2 * UROWS + 1 < H ? 2 * UROWS + 1 : H; // y rows of a unit: 7 / 12
  static constexpr int YCH = YROWS * H * 16;                          // ... in 16-byte chunks
  static constexpr int YIT = YCH / PT;                                // ... per thread: 14 / 12
  static constexpr int DROWS = UNITS > 1 ? UROWS + 1 : UROWS;         // pooled rows the backward stages: 4 / 6
  static constexpr int DCH = DROWS * HO * 16;                         // ... dp in 16-byte chunks: 768 / 576
  static constexpr int DIT = DCH / PT;                                // ... per thread: 4 / 3
  static_assert(PT % (16 * HO) == 0 && HO % UROWS == 0, "threads tile the unit");
  static_assert(YCH % PT == 0 && (2 * UROWS * H * 16) % PT == 0, "y staging rounds are workgroup-uniform");
  static_assert(DCH % PT == 0 && (UROWS * HO * 16) % PT == 0 && DCH / 4 <= PT, "dp / argmax staging rounds");
};

template <int H>
__global__ __launch_bounds__(PT) void k_f32_relu_pool_fwd(const float* __restrict__ y, float* __restrict__ p,
                                                          uint8_t* __restrict__ arg, int units) {
  using G = PoolGeom<H>;
  constexpr int HO = G::HO;
  __shared__ f32x4 ys[G::YCH];
  const int tid = threadIdx.x, c = tid & 15, px = (tid >> 4) % HO, lr = (tid / (16 * HO)) * PBAND;
  const int x0 = 2 * px, x1 = 2 * px + 1, x2 = min(2 * px + 2, H - 1);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int b = u / G::UNITS, r0 = (u - b * G::UNITS) * G::UROWS;   // image, first pooled row
    const int rows = min(G::YROWS, H - 2 * r0);                       // y rows 2 r0 .. 2 r0 + rows - 1
    const int n = rows * H * 16;                                      // a multiple of PT: rounds are uniform
    const f32x4* src = reinterpret_cast<const f32x4*>(y) + ((size_t)b * H + 2 * r0) * (H * 16);
    f32x4 v[G::YIT];
#pragma unroll
    for (int i = 0; i < G::YIT; ++i) v[i] = src[i * PT < n ? tid + i * PT : tid];   // a round past n re-reads round 0
    __syncthreads();                                                  // the previous unit's taps are read
#pragma unroll
    for (int i = 0; i < G::YIT; ++i)
      if (i * PT < n) ys[tid + i * PT] = v[i];
    __syncthreads();

    f32x4 t[9];                                                       // taps kh*3 + kw, 4 channels each
    const auto load_row = [&](int kh, int row) {
      const f32x4* r = ys + row * (H * 16) + c;
      t[3 * kh] = r[x0 * 16]; t[3 * kh + 1] = r[x1 * 16]; t[3 * kh + 2] = r[x2 * 16];
    };
    load_row(0, 2 * lr);
#pragma unroll
    for (int r = 0; r < PBAND; ++r) {
      const int y0 = 2 * (lr + r);
      load_row(1, y0 + 1);
      load_row(2, min(y0 + 2, rows - 1));
      f32x4 m = zero4();
      uint32_t a[4] = {255u, 255u, 255u, 255u};
#pragma unroll
      for (int d = 0; d < 9; ++d) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float e = t[d][j];
          if (e > m[j] || e != e) { m[j] = e; a[j] = d; }
        }
      }
      const size_t o = (((size_t)b * HO + r0 + lr + r) * HO + px) * 16 + c;
      reinterpret_cast<f32x4*>(p)[o] = m;
      reinterpret_cast<uint32_t*>(arg)[o] = a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24);
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = t[6 + k];                    // the shared row: next window's kh = 0
    }
  }
}

// dp of one window where its argmax byte (channel j of the quad) is d, else 0
DEV float pick(uint32_t a, int j, uint32_t d, float v) { return ((a >> (8 * j)) & 0xffu) == d ? v : 0.f; }

template <int H>
__global__ __launch_bounds__(PT) void k_f32_relu_pool_bwd(const float* __restrict__ dp, const uint8_t* __restrict__ arg,
                                                          float* __restrict__ dy, int units) {
  using G = PoolGeom<H>;
  constexpr int HO = G::HO;
  __shared__ f32x4 ds[G::DCH];
  __shared__ u32x4 as4[G::DCH / 4];                                   // 4 argmax bytes per (pixel, channel quad)
  const uint32_t* as = reinterpret_cast<const uint32_t*>(as4);
  const int tid = threadIdx.x, c = tid & 15, px = (tid >> 4) % HO, lr = (tid / (16 * HO)) * PBAND;
  const int ol = px > 0 ? 16 : 0;                                     // chunk distance of the left window (0: none)
  constexpr uint32_t NONE = 0xffffffffu;                              // argmax bytes of a window that does not exist
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int b = u / G::UNITS, r0 = (u - b * G::UNITS) * G::UROWS;
    const int halo = r0 > 0 ? 1 : 0;                                  // the pooled row above the band is staged too
    const int n = (G::UROWS + halo) * HO * 16;                        // a multiple of PT: rounds are uniform
    const size_t base = ((size_t)b * HO + r0 - halo) * (HO * 16);
    const f32x4* src = reinterpret_cast<const f32x4*>(dp) + base;
    const u32x4* asrc = reinterpret_cast<const u32x4*>(reinterpret_cast<const uint32_t*>(arg) + base);
    f32x4 v[G::DIT];
#pragma unroll
    for (int i = 0; i < G::DIT; ++i) v[i] = src[i * PT < n ? tid + i * PT : tid];
    const u32x4 av = asrc[tid * 4 < n ? tid : 0];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < G::DIT; ++i)
      if (i * PT < n) ds[tid + i * PT] = v[i];
    if (tid * 4 < n) as4[tid] = av;
    __syncthreads();

    const int R = lr + halo;                                          // LDS row of the thread's first pooled row
    const int ou = R > 0 ? HO * 16 : 0;                               // chunk distance of the row above (0: none)
    int i0 = (R * HO + px) * 16 + c;
    f32x4 fu = ds[i0 - ou], ful = ds[i0 - ou - ol];
    uint32_t au = ou ? as[i0 - ou] : NONE, aul = ou && ol ? as[i0 - ou - ol] : NONE;
#pragma unroll
    for (int r = 0; r < PBAND; ++r, i0 += HO * 16) {
      const f32x4 fw = ds[i0], fl = ds[i0 - ol];
      const uint32_t aw = as[i0], al = ol ? as[i0 - ol] : NONE;
      f32x4 o[4];                                                     // y pixel (2i + a, 2j + b): o[2a + b]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[0][j] = ((pick(aul, j, 8, ful[j]) + pick(au, j, 6, fu[j])) + pick(al, j, 2, fl[j])) + pick(aw, j, 0, fw[j]);
        o[1][j] = pick(au, j, 7, fu[j]) + pick(aw, j, 1, fw[j]);
        o[2][j] = pick(al, j, 5, fl[j]) + pick(aw, j, 3, fw[j]);
        o[3][j] = pick(aw, j, 4, fw[j]);
      }
      f32x4* out = reinterpret_cast<f32x4*>(dy) + (((size_t)b * H + 2 * (r0 + lr + r)) * H + 2 * px) * 16 + c;
      out[0] = o[0];
      out[16] = o[1];
      out[H * 16] = o[2];
      out[H * 16 + 16] = o[3];
      fu = fw; ful = fl; au = aw; aul = al;
    }
  }
}

constexpr int XT = 256;      // threads of the loss head (one workgroup)

template <class L>
__global__ __launch_bounds__(XT) void k_f32_xent_head(const float* __restrict__ logits, const L* __restrict__ labels,
                                                      float* __restrict__ dlogits, float* __restrict__ loss,
                                                      int* __restrict__ hits, int B, int relu) {
  __shared__ float sl[XT / 64];
  __shared__ int sh[XT / 64];
  const int tid = threadIdx.x;
  const float fB = (float)B;
  float lsum = 0.f;
  int hsum = 0;
  for (int row = tid; row < B; row += XT) {
    float x[10], z[10], e[10];
    const float2* src = reinterpret_cast<const float2*>(logits + (size_t)row * 10);   // rows are 40 bytes
#pragma unroll
    for (int j = 0; j < 5; ++j) { const float2 q = src[j]; x[2 * j] = q.x; x[2 * j + 1] = q.y; }
    const L lab = labels[row];
#pragma unroll
    for (int j = 0; j < 10; ++j) z[j] = relu ? fmaxf(x[j], 0.f) : x[j];
    float m = z[0], zl = 0.f, s = 0.f;
    int am = 0;
#pragma unroll
    for (int j = 1; j < 10; ++j)
      if (z[j] > m) { m = z[j]; am = j; }                             // first maximum
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      e[j] = expf(z[j] - m);
      s += e[j];
      if (lab == (L)j) zl = z[j];
    }
    lsum += (logf(s) + m) - zl;
    hsum += lab == (L)am ? 1 : 0;
    float2* dst = reinterpret_cast<float2*>(dlogits + (size_t)row * 10);
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const float g = (e[j] / s - (lab == (L)j ? 1.f : 0.f)) / fB;
      e[j] = relu && x[j] <= 0.f ? 0.f : g;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) dst[j] = make_float2(e[2 * j], e[2 * j + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lsum += __shfl_xor(lsum, o); hsum += __shfl_xor(hsum, o); }
  if ((tid & 63) == 0) { sl[tid >> 6] = lsum; sh[tid >> 6] = hsum; }
  __syncthreads();
  if (tid == 0) {
    float l = sl[0];
    int h = sh[0];
#pragma unroll
    for (int w = 1; w < XT / 64; ++w) { l += sl[w]; h += sh[w]; }
    *loss = l / fB;
    *hits = h;
  }
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

static int pool_grid(int units, int blocks) { return std::min(units, blocks > 0 ? blocks : PGRID); }

hipError_t dmlc_f32_relu_pool_fwd(const float* y, float* p, uint8_t* arg, int B, int H, int blocks, hipStream_t s) {
  if (B < 1 || B > (1 << 20) || blocks < 0 || (H != 24 && H != 12)) return hipErrorInvalidValue;
  if (H == 24) {
    const int units = B * PoolGeom<24>::UNITS;
    hipLaunchKernelGGL(k_f32_relu_pool_fwd<24>, dim3(pool_grid(units, blocks)), dim3(PT), 0, s, y, p, arg, units);
  } else {
    const int units = B * PoolGeom<12>::UNITS;
    hipLaunchKernelGGL(k_f32_relu_pool_fwd<12>, dim3(pool_grid(units, blocks)), dim3(PT), 0, s, y, p, arg, units);
  }
  return hipGetLastError();
}

hipError_t dmlc_f32_relu_pool_bwd(const float* dp, const uint8_t* arg, float* dy, int B, int H, int blocks,
                                  hipStream_t s) {
  if (B < 1 || B > (1 << 20) || blocks < 0 || (H != 24 && H != 12)) return hipErrorInvalidValue;
  if (H == 24) {
    const int units = B * PoolGeom<24>::UNITS;
    hipLaunchKernelGGL(k_f32_relu_pool_bwd<24>, dim3(pool_grid(units, blocks)), dim3(PT), 0, s, dp, arg, dy, units);
  } else {
    const int units = B * PoolGeom<12>::UNITS;
    hipLaunchKernelGGL(k_f32_relu_pool_bwd<12>, dim3(pool_grid(units, blocks)), dim3(PT), 0, s, dp, arg, dy, units);
  }
  return hipGetLastError();
}

hipError_t dmlc_f32_xent_head(const float* logits, const void* labels, int labels64, float* dlogits, float* loss,
                              int* hits, int B, int relu_logits, hipStream_t s) {
  if (B < 1 || B > (1 << 27)) return hipErrorInvalidValue;
  if (labels64)
    hipLaunchKernelGGL(k_f32_xent_head<int64_t>, dim3(1), dim3(XT), 0, s, logits, static_cast<const int64_t*>(labels),
                       dlogits, loss, hits, B, relu_logits);
  else
    hipLaunchKernelGGL(k_f32_xent_head<int>, dim3(1), dim3(XT), 0, s, logits, static_cast<const int*>(labels), dlogits,
                       loss, hits, B, relu_logits);
  return hipGetLastError();
}

}  // extern "C"
