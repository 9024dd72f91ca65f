// Eval-mode forward of the whole CIFAR-10 CNN (models/cifar_cnn.py) for gfx950: one launch carries N
// images from uint8 pixels to logits.  The training forward is three launches per batch because its
// fc part is batched over the whole step's images; here a persistent 512-thread workgroup (one per CU:
// the LDS footprint allows no more) takes a TILE of 16 images from pixels to logits on its own and loops
// over tiles (tile = blockIdx.x, += gridDim.x).  Workgroups never communicate: no flags, no counters,
// no grid barrier -- the only synchronisation is the workgroup barrier.
//
// Per tile:
//   conv phase   image by image, the body of k_conv12_fwd (cnn_conv.hip) on its LDS map (conv2_core.h):
//                conv1 -> pool1 (straight into conv2's padded LDS input) -> conv2 -> pool2.  Neither
//                p1 nor an argmax byte is stored; the pooled [2304] bf16 row of image i goes to row i of
//                the workgroup's slab of the scratch tensor [grid][16][2304] (72 KB: it does not fit
//                beside the 151 KB conv map; it stays in L2).  The slab is rewritten every tile, so the
//                rows leave as write-through stores and come back as sc1 loads behind a __syncthreads()
//                -- a plain load could hit the previous tile's line in L1.  The conv1 weight fragments
//                and both bias sets are fetched once per workgroup; the NEXT image's pixels and conv2
//                kernel row 0 are requested into registers before the current image's pool2.
//   fc phase     the conv regions are free.  A = the 16 x 2304 tile, copied once from the slab (rows
//                past the tile's valid count zero).  fc1 (16 x 2304 x 384) streams the current-parity
//                fc1n shadow [2304][384] in 72 k-chunks of 32 rows (24 KB, contiguous in memory) through a
//                register-staged pipeline: three chunks of loads in flight per thread (72 KB per CU),
//                two LDS buffers, one LDS-only barrier per chunk.  A chunk sits in LDS as 6 sub-tiles
//                [32 k][64 n] in the grouped GEMM's m-major swizzle (fc_common.h mz) and is read with
//                ds_read_b64_tr_b16; wave w owns the 3 n-tiles 3w .. 3w+2, K runs sequentially in one
//                accumulator each (no split-K).  The GEMMs are formulated transposed (C[n][image]), so a
//                lane holds 4 consecutive outputs of one image: bias + ReLU + bf16 leave as one 8-B LDS
//                store into h1 [16][384].  fc2 (12 n-tiles over the 8 waves) takes its weight fragments
//                straight from fc2t [192][384] (k-major, 16-B global loads) into h2 [16][192]; fc3 is
//                one wave, 6 k-steps on fc3t [16][192], and ends in the logits (fp32), the first
//                maximum and the hit flag of every valid row.
//
// LDS (154,624 B = the conv map; the fc map aliases it):
//   conv   [0, 80 KB) conv1 output / conv2 weight slices; [80, 112 KB) conv2 input; [112, 130 KB) conv2
//          output; [130, 151 KB) conv1 input                                     (C12_* of conv2_core.h)
//   fc     A  [16][2320] bf16   74,240 B at 0        B  2 x [6][32][64] bf16  49,152 B at 74,240
//          h1 [16][400]  bf16   12,800 B at 123,392   h2 [16][208] bf16        6,656 B at 136,192
// Bank model (tools/lds_banks.py, its lane groups and cycle count): the k-major rows of A, h1 and h2 are
// padded by 16 elements, i.e. a row is 8 banks further on (the grouped GEMM's KC_LD rule), and every
// ds_read_b128 of a fragment takes 4 cycles -- conflict-free (an 8-element pad: 8 cycles, none: 32); the
// B sub-tiles are the grouped GEMM's m-major image: 2 cycles per ds_read_b64_tr_b16, conflict-free.  The
// stores: A rows 4 cycles (conflict-free), a B chunk's 16-B pieces 6.7 on average (2-way on a third).
//
// fp8 variant (k_cnn_infer<true>, for engines whose conv2 shadow is e4m3: a.w2f8 [64][1600] + a.scale_w):
// the same launch with everything between pool1 and pool2 replaced; the conv1 front, the slab and the
// whole fc phase are the code above, shared through the template parameter.
//   scale      pool1 writes the bf16 p1 image as before and hands back each thread's largest pooled
//              value; wave shuffles + 8 LDS words give the image's own amax.  sx = 2^k is the largest
//              power of two with amax * sx <= 448 (k from amax's exponent and mantissa fields, clamped to
//              +-126; amax = 0: sx = 1), so bf16 * sx is exact and a host reference reproduces the
//              quantised bytes.  No scale depends on another image, on the tile or on N.  The weight scale
//              is scale_w[*step & 1], read on the device like the fc1n parity; nothing but the outputs
//              and the scratch is written.
//   quantise   p1 (padded, halo included: zeros stay zeros) -> e4m3 through the hardware converter (RNE,
//              saturating) into the padded [16x16][64] e4m3 image (16 KB, fp8_common.h x8_addr).
//   conv2      v_mfma_scale_f32_16x16x128_f8f6f4, block scales 2^0, K = (tap, ci) in 13 chunks of 128 = two
//              taps x 64 ci: 25 taps + one zero tap, 1/26 = 4 % of the MFMAs wasted (three chunks per
//              kernel row would be 15 chunks, 17 %).  Both operands see the same k order (lane group g:
//              tap 2c + (g >> 1), channels 32 (g & 1) .. + 31).  fp32 accumulators * 1 / (sx * sw) + bias,
//              ReLU, bf16, pool2 into the slab row as above.
//   weights    streamed e4m3 slices.  The whole e4m3 matrix is 13 chunk blocks [64 rows][128 B] = 104 KB,
//              and once p1 is quantised [0, 112 KB) is free, so every block has a home of its own and no
//              buffer is reused inside an image: slice 0 (chunks 0-3) and chunk 12 are requested into
//              registers under the previous image's pool2 (as kernel row 0 above) and stored after
//              pool1; slice 1 (chunks 4-7) is copied by LDS-DMA under slice 0's MFMAs, slice 2 (chunks
//              8-11) under slice 1's, each awaited (vmcnt(0) + barrier) at its predecessor's end: two
//              barriers inside the core.  Chunk 12's zero tap is stored as zeros (only 64 B of its 128
//              exist per row in memory).  Per image 104 KB of weights cross L2 -> CU instead of 200 KB.
// LDS, fp8 conv phase (same 154,624 B):
//   [0, 32 KB) slice 0   [32, 40 KB) chunk 12   [40, 72 KB) slice 1   [72, 104 KB) slice 2 (over the bf16
//   p1 image at [80, 112 KB), free once quantised)   [112, 130 KB) conv2 output
//   [130, 146 KB) e4m3 input, then 8 wave maxima (the conv1 input region, free after conv1's MFMAs)
// Bank model (tools/lds_banks.py cycles(), 4 = conflict-free): a weight row's eight 16-B units are XORed
// with (row >> 1 & 1) | (row >> 3 & 1) << 2: every A half-fragment read 4 cycles (no key 16, the key
// (row >> 1) & 7 8); the e4m3 input under x8_addr with 4x4-pixel tiles: every B read 4 cycles over all 9
// tiles x 25 taps; the quantiser's p1 reads 4 cycles, its 8-B stores 2 (ds_write_b64 lane groups).
// Per chunk a wave reads 2 A + 2-3 B fragments of 2 KB for 4-5 MFMAs of 32 cycles: 72 KB per chunk and CU
// = 288 LDS cycles against 288 MFMA cycles per SIMD (bf16: 36 KB per 144 MFMA cycles, 50 chunks).
#include "conv2_core.h"
#include "fc_common.h"
#include "fp8_common.h"

namespace dmlc {

constexpr int CI_TM = 16;                                 // images per tile
constexpr int CI_K1 = 2304, CI_N1 = 384, CI_N2 = 192;
constexpr int CI_KC = 32, CI_NCH = CI_K1 / CI_KC;         // fc1 k-chunk (one MFMA k-step), 72 chunks
constexpr int CI_LDA = CI_K1 + 16, CI_LDH1 = CI_N1 + 16, CI_LDH2 = CI_N2 + 16;   // rows 32 B (mod 256 B) apart
constexpr int CI_SUB = CI_KC * 64, CI_BBUF = CI_KC * CI_N1;   // one [32][64] sub-tile, one chunk (bf16)
constexpr size_t CI_A = 0, CI_B = CI_A + (size_t)CI_TM * CI_LDA * 2, CI_H1 = CI_B + 2 * (size_t)CI_BBUF * 2;
constexpr size_t CI_H2 = CI_H1 + (size_t)CI_TM * CI_LDH1 * 2, CI_FC_LDS = CI_H2 + (size_t)CI_TM * CI_LDH2 * 2;
constexpr size_t CI_LDS = C12_LDS > CI_FC_LDS ? C12_LDS : CI_FC_LDS;
static_assert(CI_LDS <= 160 * 1024 && CI_B % 16 == 0 && CI_H1 % 16 == 0 && CI_H2 % 16 == 0, "cnn_infer LDS map");
static_assert(CI_NCH % 6 == 0 && CI_BBUF * 2 == 3 * NT * 16, "fc1 pipeline: 3 register sets x 2 buffers, 3 loads per thread");

// A thread's share of one fc1 weight chunk (rows 32c .. 32c + 31 of [2304][384]: 24,576 contiguous
// bytes, three 16-B pieces per thread), held in registers between the global load and the LDS store.
// (named members: see conv2_core.h Slice5)
struct W1Chunk {
  uint4 a, b, c;
  static MDEV W1Chunk load(const bf16* W, int chunk, int tid) {
    const uint4* src = reinterpret_cast<const uint4*>(W + (size_t)chunk * CI_BBUF) + tid;
    return W1Chunk{src[0], src[NT], src[2 * NT]};
  }
  // piece e = row * 48 + cc (16-B chunk cc of k-row `row`) -> sub-tile cc >> 3, swizzled chunk cc & 7
  static MDEV int off(int e) {
    const int row = e / 48, cc = e - row * 48;
    return (cc >> 3) * CI_SUB + mz(row, (cc & 7) * 8);
  }
  MDEV void store(bf16* buf, int o0, int o1, int o2) const {   // o_i = off(tid + i * NT)
    *reinterpret_cast<uint4*>(buf + o0) = a;
    *reinterpret_cast<uint4*>(buf + o1) = b;
    *reinterpret_cast<uint4*>(buf + o2) = c;
  }
};

// bias + ReLU + bf16 of a transposed accumulator tile (lane: outputs n0 .. n0 + 3 of image li) -> LDS row
DEV void ci_store_relu(bf16* h, const f32x4& acc, const float4& b) {
  *reinterpret_cast<bf16x4*>(h) = pack4(fmaxf(acc[0] + b.x, 0.f), fmaxf(acc[1] + b.y, 0.f),
                                        fmaxf(acc[2] + b.z, 0.f), fmaxf(acc[3] + b.w, 0.f));
}

// ---------------------------------------------------------------------------------------------
// fp8 variant (k_cnn_infer<true>): conv2 on v_mfma_scale_f32_16x16x128_f8f6f4, see the header comment.
constexpr int F8_CHUNK = 64 * 128;             // one K chunk (two taps x 64 ci) of all 64 weight rows, bytes
constexpr int F8_SLICE = 4 * F8_CHUNK;         // 32 KB
constexpr int F8_S0 = 0, F8_C12 = F8_S0 + F8_SLICE, F8_S1 = F8_C12 + F8_CHUNK, F8_S2 = F8_S1 + F8_SLICE;
constexpr int F8_X8 = (int)C12_XIN1, F8_RED = F8_X8 + X8_BYTES;
static_assert(F8_S1 + F8_SLICE <= (int)C12_XIN2, "slices 0, 1 and chunk 12 lie in the conv1 output region");
static_assert(F8_S2 + F8_SLICE <= (int)C12_OUT2, "slice 2 ends inside the bf16 p1 image, before conv2's output");
static_assert(F8_RED + 8 * 4 <= (int)C12_LDS && F8_X8 % 16 == 0, "e4m3 input + wave maxima in the conv1 input region");

// XOR key of a weight row's eight 16-B units inside a chunk block [64 rows][128 B]
DEV int w8k(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 2); }
// byte offset in w2f8 [64][1600] of piece P (= LDS unit P of the slice buffer) of slice s < 3
DEV int f8_src(int s, int P) {
  const int cb = P >> 9, row = (P >> 3) & 63, lc = (P & 7) ^ w8k(row);
  return row * 1600 + (4 * s + cb) * 128 + lc * 16;
}
// slice s (1 or 2) -> its LDS home by LDS-DMA: 32 wave-instructions of 1 KB, 4 per wave
DEV void f8_dma(const uint8_t* Wg, int s, uint8_t* buf, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = w * 4 + i;                   // wave-uniform
    __builtin_amdgcn_global_load_lds(Wg + f8_src(s, j * 64 + lane), (LDS_AS void*)(buf + j * 1024), 16, 0, 0);
  }
}
// Slice 0 (a..d) and chunk 12 (e: tap 24 + the zero tap, of which only the first 64 B of a row exist
// in memory -- the other units are stored as zeros) through registers, as conv2_core.h ws_fetch / ws_put.
DEV Slice5 f8_fetch(const uint8_t* Wg, int w, int lane) {
  const int t = w * 64 + lane, row = t >> 3, lc = (t & 7) ^ w8k(row);
  const uint4 e = *reinterpret_cast<const uint4*>(Wg + row * 1600 + 1536 + (lc & 3) * 16);
  const uint4* src = reinterpret_cast<const uint4*>(Wg);
  return Slice5{src[f8_src(0, (w * 4 + 0) * 64 + lane) >> 4], src[f8_src(0, (w * 4 + 1) * 64 + lane) >> 4],
                src[f8_src(0, (w * 4 + 2) * 64 + lane) >> 4], src[f8_src(0, (w * 4 + 3) * 64 + lane) >> 4],
                lc < 4 ? e : make_uint4(0u, 0u, 0u, 0u)};
}
DEV void f8_put(uint8_t* s0, uint8_t* c12, int w, int lane, Slice5 v) {
  uint4* p = reinterpret_cast<uint4*>(s0) + w * 256 + lane;
  p[0] = v.a; p[64] = v.b; p[128] = v.c; p[192] = v.d;
  reinterpret_cast<uint4*>(c12)[w * 64 + lane] = v.e;
}
// A fragment's two 16-B halves, read as vectors: a load of the uint4 STRUCT (fp8_common.h lds_fp8x32) is
// an aggregate copy and carries no type information, and hipcc's waitcnt pass then makes the first such
// LDS read behind an LDS-DMA wait vmcnt(0) for it -- the next slice's copy would not overlap the MFMAs.
typedef int i32x4 __attribute__((ext_vector_type(4)));
DEV fp8x32 lds_f8(const uint8_t* lo, const uint8_t* hi) {
  return __builtin_shufflevector(*reinterpret_cast<const i32x4*>(lo), *reinterpret_cast<const i32x4*>(hi), 0, 1, 2, 3,
                                 4, 5, 6, 7);
}
constexpr int f8_chunk_off(int c) {
  return c < 4 ? F8_S0 + c * F8_CHUNK : c < 8 ? F8_S1 + (c - 4) * F8_CHUNK : c < 12 ? F8_S2 + (c - 8) * F8_CHUNK : F8_C12;
}
constexpr int f8_tap_off(int tap) { return ((tap / 5) * 16 + tap % 5) * 64; }   // padded-pixel byte offset of a tap

// The MFMAs of one image.  Tile ownership is conv2_core's: wave (cp, pg) owns c_out tiles 2cp, 2cp + 1 of
// the pixel tiles pg and pg + 4, waves 0-3 also pixel tile 8 for the one c_out tile 2cp + pg (9 of the
// 36 tile units per SIMD) -- but a pixel tile is a 4x4 block of the 12x12 output, which is what makes
// the e4m3 input image's reads conflict-free under x8_addr's row-parity key.  Lane group g holds
// k = 32g .. 32g + 31 of a chunk: tap 2c + (g >> 1), channels 32 (g & 1) .. + 31, for the weight row and
// the pixel alike.  On entry slice 0 and chunk 12 are in LDS behind a barrier; slice s + 1 is requested
// by LDS-DMA before slice s's MFMAs and awaited (vmcnt(0) + barrier) behind them.
template <bool EXTRA>
DEV void conv2_core_f8(const uint8_t* Wg, char* smem, f32x4 (&acc)[2][2], f32x4& accx, int pg, int cp, int xsel,
                       int g, int li, int w, int lane) {
  constexpr int NPX = EXTRA ? 3 : 2;
  const uint8_t* lds = reinterpret_cast<const uint8_t*>(smem);
  const int u = 2 * (g & 1), gh = g >> 1;
  int xb[NPX];                                 // pixel byte address with the unit XOR of tap (0, 0)
#pragma unroll
  for (int t = 0; t < NPX; ++t) {
    const int T = t < 2 ? pg + 4 * t : 8, ty = T / 3, tx = T - ty * 3;
    const int pb = (4 * ty + (li >> 2)) * 16 + 4 * tx + (li & 3);
    xb[t] = F8_X8 + x8_addr(pb, u);
  }
  const int ao = (32 * cp + li) * 128 + (((2 * g) ^ w8k(li)) << 4);   // (w8k(row) = w8k(li): bits 1 and 3)
#pragma unroll
  for (int t = 0; t < 2; ++t) { acc[0][t] = zero4(); acc[1][t] = zero4(); }
  accx = zero4();
  f8_dma(Wg, 1, reinterpret_cast<uint8_t*>(smem) + F8_S1, w, lane);
  // chunk c: 2 A + NPX B fragments of two 16-B reads each (the halves differ in address bit 4 only: the
  // keys XOR whole units and a lane's first unit is even); taps past 24 read tap 24 against zero weights
  auto load_chunk = [&](int c, fp8x32& a0, fp8x32& a1, fp8x32 (&bx)[NPX]) {
    const int wo = f8_chunk_off(c) + ao;
    a0 = lds_f8(lds + wo, lds + (wo ^ 16));
    a1 = lds_f8(lds + wo + 16 * 128, lds + ((wo + 16 * 128) ^ 16));
    const int t0 = 2 * c, t1 = 2 * c + 1 < 25 ? 2 * c + 1 : 24;
    const int xoff = gh ? f8_tap_off(t1) : f8_tap_off(t0);
    const int flip = (gh ? (t1 / 5) & 1 : (t0 / 5) & 1) << 4;         // the tap's kernel row flips the parity key
#pragma unroll
    for (int t = 0; t < NPX; ++t) {
      const int ad = (xb[t] ^ flip) + xoff;
      bx[t] = lds_f8(lds + ad, lds + (ad ^ 16));
    }
  };
  fp8x32 A0[2], A1[2], BX[2][NPX];
  load_chunk(0, A0[0], A1[0], BX[0]);
#pragma unroll
  for (int c = 0; c < 13; ++c) {
    const int cur = c & 1;
    const bool last_of_slice = c == 3 || c == 7;         // chunk c + 1 lies in a slice still in flight
    wait_lds();
    __builtin_amdgcn_sched_barrier(0);
    if (c + 1 < 13 && !last_of_slice) load_chunk(c + 1, A0[cur ^ 1], A1[cur ^ 1], BX[cur ^ 1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      acc[0][t] = mfma_fp8(A0[cur], BX[cur][t], acc[0][t]);
      acc[1][t] = mfma_fp8(A1[cur], BX[cur][t], acc[1][t]);
    }
    if constexpr (EXTRA) accx = mfma_fp8(xsel ? A1[cur] : A0[cur], BX[cur][NPX - 1], accx);
    __builtin_amdgcn_sched_barrier(0);
    if (last_of_slice) {
      __syncthreads();                                   // (waits vmcnt(0): the next slice has landed)
      if (c == 3) f8_dma(Wg, 2, reinterpret_cast<uint8_t*>(smem) + F8_S2, w, lane);
      load_chunk(c + 1, A0[cur ^ 1], A1[cur ^ 1], BX[cur ^ 1]);
    }
  }
}

template <class F>
DEV void conv2_tiles_f8(const uint8_t* Wg, char* smem, int w, int g, int li, int lane, F&& fn) {
  const int cp = w & 1, pg = w >> 1;
  f32x4 acc[2][2], accx;
  if (w < 4) {
    conv2_core_f8<true>(Wg, smem, acc, accx, pg, cp, pg, g, li, w, lane);
    fn(2 * cp + pg, 8, accx);
  } else {
    conv2_core_f8<false>(Wg, smem, acc, accx, pg, cp, 0, g, li, w, lane);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) { fn(2 * cp, pg + 4 * t, acc[0][t]); fn(2 * cp + 1, pg + 4 * t, acc[1][t]); }
}

// F8: conv2 in e4m3 (a.w2f8, a.scale_w) instead of bf16 (a.w2f); everything else is shared.
template <bool F8>
__global__ __launch_bounds__(NT, 1) void k_cnn_infer(DmlcCnnInferArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // conv map (as k_conv12_fwd)
  bf16* xin = reinterpret_cast<bf16*>(smem + C12_XIN1);
  bf16* cout = reinterpret_cast<bf16*>(smem);
  bf16* xin2 = reinterpret_cast<bf16*>(smem + C12_XIN2);
  bf16* cout2 = reinterpret_cast<bf16*>(smem + C12_OUT2);
  bf16* ws = reinterpret_cast<bf16*>(smem + C12_WS);
  uint8_t* raw = reinterpret_cast<uint8_t*>(cout) + 16;     // the conv1 output region is free until its epilogue
  // fc map
  bf16* As = reinterpret_cast<bf16*>(smem + CI_A);
  bf16* Bs = reinterpret_cast<bf16*>(smem + CI_B);
  bf16* h1 = reinterpret_cast<bf16*>(smem + CI_H1);
  bf16* h2 = reinterpret_cast<bf16*>(smem + CI_H2);
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int g = lane >> 4, li = lane & 15, cp = w & 1, pq = w >> 1;
  const int ntiles = (a.N + CI_TM - 1) / CI_TM;

  // ---- once per workgroup: conv1 weight fragments, both conv bias sets, the fc1 biases of this wave ----
  bf16x8 wa[2][3];
  conv1_wfrags(a.w1f, 32 * cp, g, li, wa);
  float b4[2][4], c2b[4][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) b4[h][i] = a.b1[32 * cp + 16 * h + 4 * g + i];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) c2b[c][i] = a.b2[16 * c + 4 * g + i];
  DmlcConv1FwdArgs c1 = {};                  // the launch-wide centre crop: no augmentation word
  c1.cy = a.cy; c1.cx = a.cx;
  const bf16* W2 = reinterpret_cast<const bf16*>(a.w2f);
  const uint8_t* W8 = a.w2f8;
  // 1 / sw of the e4m3 weights: the scale slot of the step counter's parity, as the fc1n slot below
  float rsw = 1.f;
  if constexpr (F8) rsw = 1.f / a.scale_w[*a.step & 1];
  const bf16* W1 = reinterpret_cast<const bf16*>(a.fc1n) + ((*a.step & 1) ? (size_t)CI_K1 * CI_N1 : 0);
  bf16* slab = reinterpret_cast<bf16*>(a.scratch) + (size_t)blockIdx.x * CI_TM * CI_K1;
  // image n of the launch (clamped: the request past the workgroup's last image re-reads a valid one)
  auto row_of = [&](int n) {
    n = min(n, a.N - 1);
    return min(max(a.idx ? a.idx[n] : n, 0), a.nrows - 1);
  };
  auto fetch_raw = [&](int n, int t) {       // 3072 B = 192 16-B pieces (threads past them re-read the last)
    return reinterpret_cast<const uint4*>(a.data + (size_t)row_of(n) * 3072)[min(t, 191)];
  };
  uint4 rawv = fetch_raw(blockIdx.x * CI_TM, tid);
  // conv2 kernel row 0 (fp8: slice 0 and chunk 12): in flight during conv1 + pool1
  auto fetch_s0 = [&](int l) {
    if constexpr (F8) return f8_fetch(W8, w, l);
    else return ws_fetch(W2, 0, w, l);
  };
  Slice5 s0v = fetch_s0(lane);

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int nv = min(CI_TM, a.N - tile * CI_TM);
    // ======================= conv phase: image i of the tile -> slab row i =======================
    for (int i = 0; i < nv; ++i) {
      // The per-lane addresses of an image's phases are the same for every image; behind this opaque copy
      // of the thread index they are recomputed per image, as in k_conv12_fwd.  (Hoisted out of the loop
      // they stay live across every phase: 256 VGPRs and 123 spilled to scratch.)
      int it = tid;
      asm volatile("" : "+v"(it));
      const int il = it & 63, ig = il >> 4, ili = il & 15;
      // (raw / xin / xin2 were last read before the previous image's post-conv2 barrier, or before the
      // previous tile's closing barrier)
      if (it < 192) reinterpret_cast<uint4*>(raw)[it] = rawv;
      stage_conv1_crop<true>(xin, raw, c1, 0, it);
      for (int s = it; s < 2048; s += NT) {   // conv2's padded input: zero halo (rows/cols 0,1,14,15)
        const int pix = s >> 3, c = s & 7, r = pix >> 4, col = pix & 15;
        if (r < 2 || r >= 14 || col < 2 || col >= 14) *reinterpret_cast<bf16x8*>(xin2 + swzpad(pix, c)) = bf16x8{};
      }
      lds_barrier();
      {
        f32x4 acc[2][9];
        conv1_mfma(xin, wa, acc, pq, ig, ili);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            store_relu_tile(cout, (pq * 9 + t) * 16 + ili, 32 * cp + 16 * h + 4 * ig, acc[h][t], b4[h]);
      }
      lds_barrier();
      if constexpr (!F8) {
        pool_emit<24, false, false>(cout, nullptr, nullptr, it, nullptr, xin2);
        lds_barrier();                                     // conv2 input complete; conv1 region free
        ws_put(ws, w, il, s0v);                            // published by the core's first barrier
        conv2_tiles(W2, xin2, ws, w, ig, ili, it, ws, [&](int ct, int t, const f32x4& acc) {
          store_relu_tile(cout2, 16 * t + ili, 16 * ct + 4 * ig, acc, c2b[ct]);
        });
      } else {
        // pool1 -> the bf16 p1 image as above, and this thread's largest pooled value (as bf16 bits: the
        // values are >= 0, so their bits order like them); the image's own amax in-block
        uint32_t bm = 0;
        pool_emit<24, false, false>(cout, nullptr, nullptr, it, &bm, xin2);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bm = max(bm, (uint32_t)__shfl_xor((int)bm, o));
        uint32_t* red = reinterpret_cast<uint32_t*>(smem + F8_RED);
        if (il == 0) red[w] = bm;
        lds_barrier();                                     // p1 and the wave maxima complete; conv1 region free
        f8_put(reinterpret_cast<uint8_t*>(smem) + F8_S0, reinterpret_cast<uint8_t*>(smem) + F8_C12, w, il, s0v);
        uint32_t am = red[0];
#pragma unroll
        for (int j = 1; j < NT / 64; ++j) am = max(am, red[j]);
        // sx = 2^k, the largest power of two with amax * sx <= 448 = 1.75 * 2^8, from amax's bf16 fields
        // (exact: no log2), k within +-126; amax = 0: sx = 1.  bf16 * sx is then exact in fp32.
        const int ex = (int)(am >> 7), mant = (int)(am & 0x7f);
        const int k = am ? min(max(8 - (ex - 127) - (mant > 0x60 ? 1 : 0), -126), 126) : 0;
        const float sx = __uint_as_float((uint32_t)(127 + k) << 23);
        const float inv = __uint_as_float((uint32_t)(127 - k) << 23) * rsw;   // 1 / (sx * sw)
        uint8_t* x8 = reinterpret_cast<uint8_t*>(smem) + F8_X8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // p1 (halo included: zeros) -> e4m3, 8 channels a task
          const int s = it + j * NT, pix = s >> 3, c = s & 7;
          const uint4 v = *reinterpret_cast<const uint4*>(xin2 + swzpad(pix, c));
          const uint32_t lo = pk_fp8x4(bf16_lo(v.x) * sx, bf16_hi(v.x) * sx, bf16_lo(v.y) * sx, bf16_hi(v.y) * sx);
          const uint32_t hi = pk_fp8x4(bf16_lo(v.z) * sx, bf16_hi(v.z) * sx, bf16_lo(v.w) * sx, bf16_hi(v.w) * sx);
          *reinterpret_cast<uint2*>(x8 + x8_addr(pix, c >> 1) + (c & 1) * 8) = make_uint2(lo, hi);
        }
        lds_barrier();                                     // e4m3 input, slice 0, chunk 12 complete; p1 free
        conv2_tiles_f8(W8, smem, w, ig, ili, il, [&](int ct, int T, f32x4 acc) {
          acc[0] *= inv; acc[1] *= inv; acc[2] *= inv; acc[3] *= inv;
          const int ty = T / 3, tx = T - ty * 3;
          store_relu_tile(cout2, (4 * ty + (ili >> 2)) * 12 + 4 * tx + (ili & 3), 16 * ct + 4 * ig, acc, c2b[ct]);
        });
      }
      __syncthreads();
      // the next image of this workgroup (the next tile's first after the tile's last): its pixels and
      // conv2 kernel row 0 are in flight during pool2 (and, at a tile's end, the fc phase)
      rawv = fetch_raw(i + 1 < nv ? tile * CI_TM + i + 1 : (tile + (int)gridDim.x) * CI_TM, it);
      s0v = fetch_s0(il);
      pool_emit<12, true, false>(cout2, slab + i * CI_K1, nullptr, it);
    }
    wait_vm_all();                         // every wave's slab stores acknowledged by L2 ...
    __syncthreads();                       // ... before any wave loads them; the conv regions are free

    // ================================ fc phase: the tile's 16 rows ================================
    // (per-lane addresses behind an opaque copy of the thread index, as in the image loop: recomputed per
    // tile instead of living, hoisted, across the conv phase)
    int ft = tid;
    asm volatile("" : "+v"(ft));
    const int fl = ft & 63, fg = fl >> 4, fli = fl & 15;
    {                                      // A: slab -> LDS, rows >= nv zero (9 sc1 16-B loads per thread)
      const rsrc_t sr = buf_rsrc(slab);
      uint4 v[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const int e = ft + u * NT, r = e / 288;
        // (masked, not `if (r >= nv) v = 0`: hipcc branched around that and waited vmcnt(0) per load)
        const uint32_t keep = r < nv ? 0xffffffffu : 0u;
        v[u] = ld16(sr, (uint32_t)(r < nv ? e : 0) * 16);
        v[u].x &= keep; v[u].y &= keep; v[u].z &= keep; v[u].w &= keep;
      }
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const int e = ft + u * NT, r = e / 288, cc = e - r * 288;
        *reinterpret_cast<uint4*>(As + r * CI_LDA + cc * 8) = v[u];
      }
    }
    // ---- fc1: C[n][image] = sum_k W1[k][n] * A[image][k], wave w: n-tiles 3w .. 3w + 2 ----
    f32x4 acc1[3] = {zero4(), zero4(), zero4()};
    {
      W1Chunk r0 = W1Chunk::load(W1, 0, ft), r1 = W1Chunk::load(W1, 1, ft), r2 = W1Chunk::load(W1, 2, ft);
      const int q = fli >> 2, p = fli & 3;
      int bo[3][2];                          // the lane's two tr-read offsets per n-tile, in a chunk buffer
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int j = 3 * w + t, sub = (j >> 2) * CI_SUB, c0 = 16 * (j & 3) + 4 * p;
        bo[t][0] = sub + mz(8 * fg + q, c0);
        bo[t][1] = sub + mz(8 * fg + 4 + q, c0);
      }
      const bf16* arow = As + fli * CI_LDA + 8 * fg;
      const int so0 = W1Chunk::off(ft), so1 = W1Chunk::off(ft + NT), so2 = W1Chunk::off(ft + 2 * NT);
      // chunk c: its registers -> buffer c & 1 (last read two chunks ago, behind the barrier in between),
      // the loads of chunk c + 3 into the freed registers (past the end: the last chunk again, so that no
      // load is predicated), one LDS-only barrier -- global loads stay in flight across it -- then 3 MFMAs.
      // (by value in, by value out: through a reference hipcc kept the chunks in scratch)
      auto chunk = [&](W1Chunk r, int c, bf16* buf) {
        r.store(buf, so0, so1, so2);
        const W1Chunk nx = W1Chunk::load(W1, min(c + 3, CI_NCH - 1), ft);
        lds_barrier();
        const bf16x8 x = lds_b128(arow + c * CI_KC);
#pragma unroll
        for (int t = 0; t < 3; ++t) acc1[t] = mfma16(tr_frag(buf + bo[t][0], buf + bo[t][1]), x, acc1[t]);
        return nx;
      };
      bf16* B0 = Bs;
      bf16* B1 = Bs + CI_BBUF;
      for (int c = 0; c < CI_NCH; c += 6) {
        r0 = chunk(r0, c, B0); r1 = chunk(r1, c + 1, B1); r2 = chunk(r2, c + 2, B0);
        r0 = chunk(r0, c + 3, B1); r1 = chunk(r1, c + 4, B0); r2 = chunk(r2, c + 5, B1);
      }
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int n0 = 16 * (3 * w + t) + 4 * fg;
      ci_store_relu(h1 + fli * CI_LDH1 + n0, acc1[t], *reinterpret_cast<const float4*>(a.fb1 + n0));
    }
    lds_barrier();                         // h1 complete
    // ---- fc2: n-tiles w, w + 8 (wave-uniform), weight fragments straight from fc2t [192][384] ----
    for (int j = w; j < CI_N2 / 16; j += NT / 64) {
      const bf16* Wr = reinterpret_cast<const bf16*>(a.fc2t) + (16 * j + fli) * CI_N1 + 8 * fg;
      bf16x8 wf[CI_N1 / 32];
#pragma unroll
      for (int ks = 0; ks < CI_N1 / 32; ++ks) wf[ks] = glb_b128(Wr + 32 * ks);
      f32x4 acc = zero4();
#pragma unroll
      for (int ks = 0; ks < CI_N1 / 32; ++ks) acc = mfma16(wf[ks], lds_b128(h1 + fli * CI_LDH1 + 32 * ks + 8 * fg), acc);
      const int n0 = 16 * j + 4 * fg;
      ci_store_relu(h2 + fli * CI_LDH2 + n0, acc, *reinterpret_cast<const float4*>(a.fb2 + n0));
    }
    lds_barrier();                         // h2 complete
    // ---- fc3 (wave 0): lane (g, li) = (fg, fli) holds logits 4g .. 4g + 3 of image li ----
    if (w == 0) {
      const bf16* Wr = reinterpret_cast<const bf16*>(a.fc3t) + fli * CI_N2 + 8 * fg;
      f32x4 acc = zero4();
#pragma unroll
      for (int ks = 0; ks < CI_N2 / 32; ++ks) acc = mfma16(glb_b128(Wr + 32 * ks), lds_b128(h2 + fli * CI_LDH2 + 32 * ks + 8 * fg), acc);
      const int n = tile * CI_TM + fli;       // the lane's image
      const bool valid = fli < nv;
      float best = -INFINITY;
      int bi = 64;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 4 * fg + i;
        float v = acc[i] + a.fb3[min(k, 9)];
        if (a.relu_logits) v = fmaxf(v, 0.f);
        if (k < 10) {
          if (valid) a.logits[(size_t)n * 10 + k] = v;
          if (v > best) { best = v; bi = k; }            // strict: the first maximum
        }
      }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {                // over the image's four lanes; ties -> smaller index
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (valid && fg == 0) {
        if (a.pred) a.pred[n] = bi;
        if (a.correct) a.correct[n] = bi == a.labels[row_of(n)] ? 1 : 0;
      }
    }
    lds_barrier();                         // h2 read: the next tile's conv1 input overwrites it
  }
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

hipError_t dmlc_cnn_infer_grid(int N, int blocks, int* grid) {
  if (N < 1 || blocks < 0) return hipErrorInvalidValue;
  if (blocks == 0) {                       // one workgroup per CU
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&blocks, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (blocks < 1) blocks = 1;
  }
  const int tiles = (N + CI_TM - 1) / CI_TM;
  *grid = tiles < blocks ? tiles : blocks;
  return hipSuccess;
}

hipError_t dmlc_cnn_infer(const DmlcCnnInferArgs* a, hipStream_t s) {
  if (a->N < 1 || a->nrows < 1 || a->blocks < 0 || (a->correct && !a->labels)) return hipErrorInvalidValue;
  if (!a->w2f8 != !a->scale_w || (!a->w2f8 && !a->w2f)) return hipErrorInvalidValue;
  int grid = 0;
  const hipError_t e = dmlc_cnn_infer_grid(a->N, a->blocks, &grid);
  if (e != hipSuccess) return e;
  if (a->scratch_slabs < grid) return hipErrorInvalidValue;   // one slab per workgroup
  if (a->w2f8) {                           // the fp8 variant: e4m3 conv2 weights + their scale slots
    DMLC_LDS_OPTIN(&k_cnn_infer<true>, CI_LDS);
    hipLaunchKernelGGL(k_cnn_infer<true>, dim3(grid), dim3(NT), CI_LDS, s, *a);
  } else {
    DMLC_LDS_OPTIN(&k_cnn_infer<false>, CI_LDS);
    hipLaunchKernelGGL(k_cnn_infer<false>, dim3(grid), dim3(NT), CI_LDS, s, *a);
  }
  return hipGetLastError();
}

}  // extern "C"
