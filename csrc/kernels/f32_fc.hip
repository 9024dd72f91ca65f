// The fully connected stack of the fp32 training step (--dtype fp32, ops/f32.py fc_impl = "fused"): everything
// behind fc1's forward, 2304 -> 384 -> 192 -> 10, in three launches on v_mfma_f32_16x16x4_f32 (true fp32
// operands and accumulation).  No kernel here waits on another workgroup -- no flags, counters or atomics --
// and every output element is written once by one workgroup in a fixed order: results are bit-reproducible.
//
//  * k_f32_fc_tail_fwd: h2 = relu(h1 W2 + b2), logits = h2 W3 + b3.  Batch rows are independent, so a
//    workgroup (6 waves) owns 16 rows: the h1 tile lives in LDS (pitch 388 floats: a 16-B fragment read of
//    16 rows covers all 64 banks), W2 streams from L2 as second-operand fragments -- one 16-B load per lane
//    brings 4 consecutive columns of one k row, which are the same MFMA column of 4 column tiles, so a lane
//    ends up owning 4 consecutive output columns and stores them as one vector.  Waves 0-2 take K 0..191 of
//    64 columns each, waves 3-5 K 192..383 of the same columns; the halves meet in LDS (low + high, then the
//    bias).  The h2 tile stays in LDS for fc3: W3's 40-byte rows are read with scalar loads, its 10 columns
//    one MFMA column tile padded with zeros in registers (never read past a row).
//  * k_f32_fc_tail_bwd: dh2 = (dlogits W3^T) . [h2 > 0], dh1 = (dh2 W2^T) . [h1 > 0] with the same row tile
//    and the same device core; W3 and W2 are read in place as stored (k-contiguous now: one 16-B load brings
//    4 consecutive k of one column, and the LDS operand is read with the same k permutation).
//  * k_f32_fc_grads: ONE launch over a tile table of four problems -- dW1 = x^T dh1 [2304,384], dW2 = h1^T dh2
//    [384,192], dW3 = h2^T dlogits [192,10] (K = B) and dx = dh1 W1^T [B,2304] (K = 384, optional) -- 64x64
//    tiles, 4 waves of 32x32.  The weight gradients stage both k-major operands with 16-B loads straight into
//    k-major LDS rows (f32_gemm.hip's 80-float pitch); the tiles of the first row block also sum the columns
//    of dh as it passes through LDS and write them as row `in` of the [in + 1, out] output: the bias gradient.
//    dx needs no LDS: both operands are k-contiguous, a 16-B load per lane feeds 4 MFMAs with one k
//    permutation on both sides.  The longer tiles (dx while B <= 384) come first in the table, and a block
//    finds its problem by comparing its index with all four ranges at once.
#include "common.h"
#include "api_f32.h"

namespace dmlc {

constexpr int FC_T = 384, FC_R = 16;                 // tail kernels: threads (6 waves), rows per workgroup
constexpr int FC_D1 = 384, FC_D2 = 192, FC_D3 = 10;  // h1, h2, logits widths
constexpr int FC_P1 = FC_D1 + 4, FC_P2 = FC_D2 + 4;  // LDS pitches (== 4 mod 64 floats)
constexpr int FC_U = 3;                              // fc_core: 16-k chunks per loop trip
constexpr int FC_PL = 12;                            // dlogits tile pitch: K = 10 padded to 3 MFMA k-steps

DEV f32x4 fc_mfma(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
DEV float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The wave-level core of both tail kernels: acc[0..3] += A[16][kbeg..kend) . op(B) for four 16-column tiles.
// A: an LDS tile, row pitch `pitch` floats; kbeg a multiple of 16, kend - kbeg of 16 FC_U.  Lane (r = lane & 15, q = lane >> 4)
// reads A[r][k0 + 4q .. + 3] per 16-k chunk and pairs element s with B row k0 + 4q + s (the k permutation is
// the same on both sides, the sum the same set of products).
//  !TB: B stored [K][ldb], columns contiguous: the lane's 16-B load of row k holds columns n0 + 4r .. + 3, one
//       per tile: acc[t] element i is C[4q + i][n0 + 4r + t].
//   TB: B stored [N][ldb], k contiguous (the product with B^T): the load of row n0 + 16t + r holds its 4 k:
//       acc[t] element i is C[4q + i][n0 + 16t + r].
template <bool TB>
DEV void fc_core(const float* As, int pitch, const float* __restrict__ Bg, int ldb, int kbeg, int kend, int n0,
                 int lane, f32x4 (&acc)[4]) {
  const int r = lane & 15, q = lane >> 4;
  const float* ap = As + r * pitch + 4 * q;
  const float* bp = TB ? Bg + (int64_t)(n0 + r) * ldb + 4 * q : Bg + (int64_t)(4 * q) * ldb + n0 + 4 * r;
  for (int k0 = kbeg; k0 < kend; k0 += 16 * FC_U) {             // FC_U chunks of loads in flight per lane
    float4 b[FC_U][4], a[FC_U];
#pragma unroll
    for (int c = 0; c < FC_U; ++c) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        b[c][u] = ld4(TB ? bp + (int64_t)(16 * u) * ldb + k0 + 16 * c : bp + (int64_t)(k0 + 16 * c + u) * ldb);
      a[c] = ld4(ap + k0 + 16 * c);
    }
#pragma unroll
    for (int c = 0; c < FC_U; ++c) {
      const float av[4] = {a[c].x, a[c].y, a[c].z, a[c].w};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if constexpr (TB) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float bv[4] = {b[c][t].x, b[c][t].y, b[c][t].z, b[c][t].w};
            acc[t] = fc_mfma(av[s], bv[s], acc[t]);
          }
        } else {
          acc[0] = fc_mfma(av[s], b[c][s].x, acc[0]);
          acc[1] = fc_mfma(av[s], b[c][s].y, acc[1]);
          acc[2] = fc_mfma(av[s], b[c][s].z, acc[2]);
          acc[3] = fc_mfma(av[s], b[c][s].w, acc[3]);
        }
      }
    }
  }
}

__global__ __launch_bounds__(FC_T) void k_f32_fc_tail_fwd(const float* __restrict__ h1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, const float* __restrict__ w3,
                                                          const float* __restrict__ b3, float* __restrict__ h2,
                                                          float* __restrict__ logits, int B) {
  __shared__ __attribute__((aligned(16))) float h1s[FC_R * FC_P1], h2s[FC_R * FC_P2], part[FC_R * FC_P2];
  const int t = threadIdx.x, lane = t & 63, w = wave_id(), r = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * FC_R;
  for (int e = t; e < FC_R * FC_D1 / 4; e += FC_T) {            // the h1 tile; rows past the batch are zeros
    const int row = e / (FC_D1 / 4), c = e - row * (FC_D1 / 4);
    const bool ok = row0 + row < B;
    const float4 v = load_sel(reinterpret_cast<const float4*>(h1 + (int64_t)(ok ? row0 + row : 0) * FC_D1) + c,
                              reinterpret_cast<const float4*>(h1), ok);
    *reinterpret_cast<float4*>(h1s + row * FC_P1 + 4 * c) = v;
  }
  __syncthreads();
  // fc2: wave w -> columns 64 (w % 3) .. + 63, K half w / 3
  const int half = w >= 3 ? 1 : 0, n0 = 64 * (w - 3 * half);
  f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
  fc_core<false>(h1s, FC_P1, w2, FC_D2, half * (FC_D1 / 2), (half + 1) * (FC_D1 / 2), n0, lane, acc);
  if (half) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<float4*>(part + (4 * q + i) * FC_P2 + n0 + 4 * r) = make_float4(acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
  }
  __syncthreads();
  if (!half) {
    const float4 bv = ld4(b2 + n0 + 4 * r);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * q + i;
      const float4 hi = ld4(part + row * FC_P2 + n0 + 4 * r);
      float4 v;
      v.x = fmaxf((acc[0][i] + hi.x) + bv.x, 0.f);
      v.y = fmaxf((acc[1][i] + hi.y) + bv.y, 0.f);
      v.z = fmaxf((acc[2][i] + hi.z) + bv.z, 0.f);
      v.w = fmaxf((acc[3][i] + hi.w) + bv.w, 0.f);
      *reinterpret_cast<float4*>(h2s + row * FC_P2 + n0 + 4 * r) = v;
      if (row0 + row < B) *reinterpret_cast<float4*>(h2 + (int64_t)(row0 + row) * FC_D2 + n0 + 4 * r) = v;
    }
  }
  __syncthreads();
  if (w != 0) return;
  // fc3 on wave 0: column r of the one column tile is W3's column r, zero from 10 on
  f32x4 c = zero4();
  const bool col = r < FC_D3;
#pragma unroll 4
  for (int k0 = 0; k0 < FC_D2; k0 += 16) {
    const int k = k0 + 4 * q;
    float bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) bv[s] = load_sel(w3 + (col ? (k + s) * FC_D3 + r : 0), w3, col);
    const float4 a = ld4(h2s + r * FC_P2 + k);
    c = fc_mfma(a.x, bv[0], c);
    c = fc_mfma(a.y, bv[1], c);
    c = fc_mfma(a.z, bv[2], c);
    c = fc_mfma(a.w, bv[3], c);
  }
  const float b3v = load_sel(b3 + (col ? r : 0), b3, col);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 4 * q + i;
    if (col && row < B) logits[(int64_t)row * FC_D3 + r] = c[i] + b3v;
  }
}

__global__ __launch_bounds__(FC_T) void k_f32_fc_tail_bwd(const float* __restrict__ dl, const float* __restrict__ h1,
                                                          const float* __restrict__ h2, const float* __restrict__ w2,
                                                          const float* __restrict__ w3, float* __restrict__ dh2,
                                                          float* __restrict__ dh1, int B) {
  __shared__ __attribute__((aligned(16))) float dls[FC_R * FC_PL], dh2s[FC_R * FC_P2];
  const int t = threadIdx.x, lane = t & 63, w = wave_id(), r = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * FC_R;
  if (t < FC_R * FC_PL) {                                        // the dlogits tile, zeros past row B and column 10
    const int row = t / FC_PL, k = t - row * FC_PL;
    const bool ok = row0 + row < B && k < FC_D3;
    dls[t] = load_sel(dl + (ok ? (int64_t)(row0 + row) * FC_D3 + k : 0), dl, ok);
  }
  __syncthreads();
  // dh2: 12 column tiles of 16, two per wave; B^T = W3 as stored, 10 k per row read with scalar loads
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int n = 32 * w + 16 * u + r;
    f32x4 c = zero4();
#pragma unroll
    for (int kk = 0; kk < FC_PL / 4; ++kk) {
      const int k = 4 * kk + q;
      const bool ok = k < FC_D3;
      c = fc_mfma(dls[r * FC_PL + k], load_sel(w3 + (ok ? n * FC_D3 + k : 0), w3, ok), c);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * q + i;
      const bool ok = row0 + row < B;
      const float h = load_sel(h2 + (ok ? (int64_t)(row0 + row) * FC_D2 + n : 0), h2, ok);
      const float g = h > 0.f ? c[i] : 0.f;
      dh2s[row * FC_P2 + n] = g;
      if (ok) dh2[(int64_t)(row0 + row) * FC_D2 + n] = g;
    }
  }
  __syncthreads();
  // dh1: wave w -> columns 64 w .. + 63, K = 192; B^T = W2 as stored
  const int n0 = 64 * w;
  f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
  fc_core<true>(dh2s, FC_P2, w2, FC_D2, 0, FC_D2, n0, lane, acc);
#pragma unroll
  for (int tt = 0; tt < 4; ++tt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 4 * q + i, n = n0 + 16 * tt + r;
      if (row < B) dh1[(int64_t)row * FC_D1 + n] = h1[(int64_t)row * FC_D1 + n] > 0.f ? acc[tt][i] : 0.f;
    }
}

// ---- k_f32_fc_grads -------------------------------------------------------------------------------------------
constexpr int FG_T = 256, FG_BK = 32, FG_LD = 80, FC_D0 = 2304;

struct F32FcGradArgs {
  const float *x, *h1, *h2, *dh1, *dh2, *dl, *w1;
  float *g1, *g2, *g3, *dx;
  int B;
  int beg[4], cnt[4];      // tile ranges of dW1, dW2, dW3, dx in the grid (cnt 0: absent)
};

// One 64x64 tile of out[M (+ 1)][N] = A^T Bm, A stored [K][M], Bm stored [K][N] (both k-major); M a multiple
// of 64, N a multiple of 64 or (NARROW) any width whose rows are read with scalar loads.  With m0 == 0 the
// block also writes row M = the column sums of Bm for its 64 columns, in a fixed order.
template <bool NARROW>
DEV void fg_wgrad_tile(float* As, float* Bs, const float* __restrict__ A, const float* __restrict__ Bm,
                       float* __restrict__ out, int M, int N, int K, int m0, int n0) {
  const int t = threadIdx.x, lane = t & 63, w = wave_id(), r = lane & 15, q = lane >> 4;
  const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
  const int c4 = 4 * (t & 15), kr = t >> 4;          // staging: float4 column, k row (+ 16 p)
  const int scol = t & 63, sg = t >> 6;              // column sums: column, k phase
  const bool bias = m0 == 0;
  float4 pa[2], pb[2];
  const auto load = [&](int k0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = k0 + kr + 16 * p;
      const bool ok = k < K;
      pa[p] = load_sel(reinterpret_cast<const float4*>(A + (int64_t)(ok ? k : 0) * M + m0 + c4),
                       reinterpret_cast<const float4*>(A), ok);
      if constexpr (NARROW) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool oke = ok && n0 + c4 + e < N;
          v[e] = load_sel(Bm + (oke ? (int64_t)k * N + n0 + c4 + e : 0), Bm, oke);
        }
        pb[p] = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        pb[p] = load_sel(reinterpret_cast<const float4*>(Bm + (int64_t)(ok ? k : 0) * N + n0 + c4),
                         reinterpret_cast<const float4*>(Bm), ok);
      }
    }
  };
  f32x4 acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
  float bsum = 0.f;
  load(0);
  for (int k0 = 0; k0 < K; k0 += FG_BK) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      *reinterpret_cast<float4*>(As + (kr + 16 * p) * FG_LD + c4) = pa[p];
      *reinterpret_cast<float4*>(Bs + (kr + 16 * p) * FG_LD + c4) = pb[p];
    }
    __syncthreads();
    if (k0 + FG_BK < K) load(k0 + FG_BK);            // the next step under the MFMAs
#pragma unroll
    for (int kk = 0; kk < FG_BK / 4; ++kk) {
      const float* ar = As + (4 * kk + q) * FG_LD + wm + r;
      const float* br = Bs + (4 * kk + q) * FG_LD + wn + r;
      const float a0 = ar[0], a1 = ar[16], b0 = br[0], b1 = br[16];
      acc[0][0] = fc_mfma(a0, b0, acc[0][0]);
      acc[0][1] = fc_mfma(a0, b1, acc[0][1]);
      acc[1][0] = fc_mfma(a1, b0, acc[1][0]);
      acc[1][1] = fc_mfma(a1, b1, acc[1][1]);
    }
    if (bias) {
#pragma unroll
      for (int i = 0; i < FG_BK / 4; ++i) bsum += Bs[(4 * i + sg) * FG_LD + scol];
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn + 16 * j + r;
    if (NARROW && col >= N) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(int64_t)(m0 + wm + 16 * i + 4 * q + e) * N + col] = acc[i][j][e];
  }
  if (bias) {                                         // block-uniform
    As[sg * 64 + scol] = bsum;
    __syncthreads();
    if (t < 64 && n0 + t < N) out[(int64_t)M * N + n0 + t] = (As[t] + As[64 + t]) + (As[128 + t] + As[192 + t]);
  }
}

// One 64x64 tile of dx[B][2304] = dh1 [B][384] . W1^T, W1 stored [2304][384]: both operands k-contiguous, no LDS.
DEV void fg_dx_tile(const float* __restrict__ dh1, const float* __restrict__ w1, float* __restrict__ dx, int B, int m0,
                    int n0) {
  const int lane = threadIdx.x & 63, w = wave_id(), r = lane & 15, q = lane >> 4;
  const int wm = m0 + (w & 1) * 32, wn = n0 + (w >> 1) * 32;
  const float *ap[2], *bp[2];
  bool aok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    aok[i] = wm + 16 * i + r < B;
    ap[i] = dh1 + (int64_t)(aok[i] ? wm + 16 * i + r : 0) * FC_D1 + 4 * q;
    bp[i] = w1 + (int64_t)(wn + 16 * i + r) * FC_D1 + 4 * q;
  }
  f32x4 acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
#pragma unroll 4
  for (int k0 = 0; k0 < FC_D1; k0 += 16) {
    float a[2][4], b[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 va = ld4(ap[i] + k0), vb = ld4(bp[i] + k0);
      a[i][0] = aok[i] ? va.x : 0.f; a[i][1] = aok[i] ? va.y : 0.f; a[i][2] = aok[i] ? va.z : 0.f; a[i][3] = aok[i] ? va.w : 0.f;
      b[i][0] = vb.x; b[i][1] = vb.y; b[i][2] = vb.z; b[i][3] = vb.w;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = fc_mfma(a[i][s], b[j][s], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = wm + 16 * i + 4 * q + e;
      if (row >= B) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) dx[(int64_t)row * FC_D0 + wn + 16 * j + r] = acc[i][j][e];
    }
}

__global__ __launch_bounds__(FG_T) void k_f32_fc_grads(F32FcGradArgs p) {
  __shared__ __attribute__((aligned(16))) float As[FG_BK * FG_LD], Bs[FG_BK * FG_LD];
  const unsigned bid = blockIdx.x;
  // the block's problem: all four ranges compared at once (cnt 0 never matches)
  const unsigned o0 = bid - (unsigned)p.beg[0], o1 = bid - (unsigned)p.beg[1], o2 = bid - (unsigned)p.beg[2],
                 o3 = bid - (unsigned)p.beg[3];
  const bool i0 = o0 < (unsigned)p.cnt[0], i1 = o1 < (unsigned)p.cnt[1], i2 = o2 < (unsigned)p.cnt[2];
  if (i0) {                  // dW1 [2304 + 1][384] = x^T dh1: 36 x 6 tiles
    const int mt = o0 / 6, nt = o0 - mt * 6;
    fg_wgrad_tile<false>(As, Bs, p.x, p.dh1, p.g1, FC_D0, FC_D1, p.B, mt * 64, nt * 64);
  } else if (i1) {           // dW2 [384 + 1][192] = h1^T dh2: 6 x 3 tiles
    const int mt = o1 / 3, nt = o1 - mt * 3;
    fg_wgrad_tile<false>(As, Bs, p.h1, p.dh2, p.g2, FC_D1, FC_D2, p.B, mt * 64, nt * 64);
  } else if (i2) {           // dW3 [192 + 1][10] = h2^T dlogits: 3 x 1 tiles
    fg_wgrad_tile<true>(As, Bs, p.h2, p.dl, p.g3, FC_D2, FC_D3, p.B, (int)o2 * 64, 0);
  } else if (o3 < (unsigned)p.cnt[3]) {   // dx [B][2304]: ceil(B / 64) x 36 tiles
    const int mt = o3 / 36, nt = o3 - mt * 36;
    fg_dx_tile(p.dh1, p.w1, p.dx, p.B, mt * 64, nt * 64);
  }
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

hipError_t dmlc_f32_fc_tail_fwd(const float* h1, const float* w2, const float* b2, const float* w3, const float* b3,
                                float* h2, float* logits, int B, hipStream_t s) {
  if (B < 1 || B > DMLC_F32_FC_MAX_B) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_f32_fc_tail_fwd, dim3((B + FC_R - 1) / FC_R), dim3(FC_T), 0, s, h1, w2, b2, w3, b3, h2, logits, B);
  return hipGetLastError();
}

hipError_t dmlc_f32_fc_tail_bwd(const float* dlogits, const float* h1, const float* h2, const float* w2, const float* w3,
                                float* dh2, float* dh1, int B, hipStream_t s) {
  if (B < 1 || B > DMLC_F32_FC_MAX_B) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_f32_fc_tail_bwd, dim3((B + FC_R - 1) / FC_R), dim3(FC_T), 0, s, dlogits, h1, h2, w2, w3, dh2, dh1, B);
  return hipGetLastError();
}

hipError_t dmlc_f32_fc_grads(const float* x, const float* h1, const float* h2, const float* dh1, const float* dh2,
                             const float* dlogits, const float* w1, float* g1, float* g2, float* g3, float* dx, int B,
                             hipStream_t s) {
  if (B < 1 || B > DMLC_F32_FC_MAX_B) return hipErrorInvalidValue;
  F32FcGradArgs p{x, h1, h2, dh1, dh2, dlogits, w1, g1, g2, g3, dx, B, {0, 0, 0, 0}, {36 * 6, 6 * 3, 3, 0}};
  p.cnt[3] = dx ? (B + 63) / 64 * 36 : 0;
  // the longest tiles first: a dx tile runs K = 384, a weight-gradient tile K = B
  const bool dx_first = B <= FC_D1;
  int at = dx_first ? p.cnt[3] : 0;
  for (int k = 0; k < 3; ++k) {
    p.beg[k] = at;
    at += p.cnt[k];
  }
  p.beg[3] = dx_first ? 0 : at;
  hipLaunchKernelGGL(k_f32_fc_grads, dim3(p.cnt[0] + p.cnt[1] + p.cnt[2] + p.cnt[3]), dim3(FG_T), 0, s, p);
  return hipGetLastError();
}

}  // extern "C"
