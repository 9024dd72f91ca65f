// Host-side API of the fp32 kernels (csrc/kernels/f32_gemm.hip): the fp32-accurate path of the
// reference CNN (every reference variable and op is tf.float32, /root/reference/cifar10cnn.py:97-145).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// C[M,N] = op(A)[M,K] . op(B)[K,N] (+ bias[N]) (ReLU), fp32 in, fp32 MFMA (v_mfma_f32_16x16x4_f32),
// fp32 out.  op(A) = A stored [M,K] (row stride lda) or, with ta, A stored [K,M]; likewise op(B) =
// B stored [K,N] (ldb) or, with tb, B stored [N,K].  splits > 1: K is cut into `splits` chunks of
// `kc` (multiple of 16) whose partial products go to ws[splits][M][N] and are summed in slice order
// by a second kernel (deterministic).  ws may be null when splits == 1.
// conv = 1 / 2: A is an NHWC activation and op(A) its implicit im2col matrix (no tb): geometry 1 =
// [B][24][24][3], geometry 2 = [B][12][12][64], 5x5 taps, pad 2; rows = pixels (B*HW*HW), columns
// (kh*5 + kw)*C + c, and column 25*C (if K or M reaches it) is the constant 1 (bias-gradient row).
// With ta the product is im2col(A)^T op(B) (weight gradient); lda is unused.
hipError_t dmlc_f32_gemm(const float* A, const float* B, const float* bias, float* C, float* ws, int M, int N,
                         int K, int lda, int ldb, bool ta, bool tb, bool relu, int splits, int kc, int conv,
                         hipStream_t s);

// im2col of a stride-1, zero-padded KHxKW convolution (TF 'SAME' for odd kernels: pad = k/2):
// x NHWC [B,H,W,C] -> cols [B*H*W][KH*KW*C], column (kh*KW + kw)*C + c (the row order of an HWIO
// weight viewed as [KH*KW*C][CO]).
hipError_t dmlc_f32_im2col(const float* x, float* cols, int B, int H, int W, int C, int KH, int KW, int pad,
                           hipStream_t s);
// Its adjoint, as a gather (fixed summation order, deterministic): dx[b,y,x,c] = sum over the
// (kh,kw) taps of dcols[(b, y-kh+pad, x-kw+pad)][(kh*KW + kw)*C + c].
hipError_t dmlc_f32_col2im(const float* dcols, float* dx, int B, int H, int W, int C, int KH, int KW, int pad,
                           hipStream_t s);
// out[N] = sum over the M rows of x[M][N], in a fixed order (ws: >= splits * N floats).
hipError_t dmlc_f32_colsum(const float* x, float* out, float* ws, int M, int N, int splits, hipStream_t s);

// k_cnn_infer_f32 (csrc/kernels/f32_infer.hip): the eval-mode forward of the CIFAR-10 CNN in true fp32,
// uint8 pixels to fp32 logits in one launch.  Image i of the launch is data[idx[i]] (idx null: data[i]);
// the weights are the TF-layout views of the model's flat fp32 parameter buffer (every pointer 16-byte
// aligned).  scratch: fp32 [scratch_slabs][16][2304], one slab per workgroup; pred / correct optional
// (correct needs labels, one per data row).  blocks: workgroups of the persistent loop, 0 = one per CU.
typedef struct {
  const uint8_t* data;       // [nrows][32][32][3]
  const int* idx;            // [N] or null
  const int* labels;         // [nrows] or null
  const float *w1, *b1;      // [75][64], [64]
  const float *w2, *b2;      // [1600][64], [64]
  const float *fw1, *fb1;    // [2304][384], [384]
  const float *fw2, *fb2;    // [384][192], [192]
  const float *fw3, *fb3;    // [192][10], [10]
  float* scratch;
  float* logits;             // [N][10]
  int* pred;                 // [N] or null
  int* correct;              // [N] or null
  int N, nrows, cy, cx, relu_logits, blocks, scratch_slabs;
} DmlcF32InferArgs;
// the launch's grid: min(ceil(N / 16), blocks or the device's CU count)
hipError_t dmlc_f32_infer_grid(int N, int blocks, int* grid);
hipError_t dmlc_f32_infer(const DmlcF32InferArgs* a, hipStream_t s);

// k_f32_conv2 (csrc/kernels/f32_conv.hip): the stride-1 TF-SAME 5x5 convolution of x NHWC [B][12][12][64]
// with 64 output channels, direct (the image in LDS, the weights streamed as MFMA fragments), no ReLU.
// w: the HWIO weight [5][5][64][64].  dgrad = 0: y = conv(x, w) + bias (bias [64] or null).  dgrad = 1: x is
// dY and y = dX, the data gradient, with w read in place as W[4-kh][4-kw][ci][co] (bias must be null).
// blocks: workgroups of the persistent loop over images, 0 = one per CU.  Every pointer 16-byte aligned.
hipError_t dmlc_f32_conv2(const float* x, const float* w, const float* bias, float* y, int B, int dgrad, int blocks,
                          hipStream_t s);

// k_f32_conv2_wgrad + k_f32_wgrad_reduce (csrc/kernels/f32_conv.hip): conv2's weight and bias gradient, direct.
// x, dy fp32 NHWC [B][12][12][64] -> out [1601][64]: row (kh*5 + kw)*64 + ci = dW[kh][kw][ci][:], row 1600 = db
// (the layout of dmlc_f32_gemm's conv = 2 weight gradient with the ones column).  groups: image groups =
// partial sums per output element, 0 = CUs / 4 (one workgroup per CU), clamped to B; the result is
// bit-reproducible for a fixed (B, groups).  ws: the partials, written and read by this call only; _plan
// returns the group count G used and the floats ws must hold.  Every pointer 16-byte aligned.
hipError_t dmlc_f32_conv2_wgrad_plan(int B, int groups, int* G, size_t* ws_floats);
hipError_t dmlc_f32_conv2_wgrad(const float* x, const float* dy, float* out, float* ws, int B, int groups,
                                hipStream_t s);

// k_f32_conv1_wgrad + k_f32_conv1_reduce (csrc/kernels/f32_conv1.hip): conv1's weight and bias gradient, direct.
// x fp32 NHWC [B][24][24][3] -> out [76][64]: row (kh*5 + kw)*3 + ci = dW[kh][kw][ci][:], row 75 = db (the layout
// of dmlc_f32_gemm's conv = 1 weight gradient with the ones column).  The gradient at the conv output is either
// dy [B][24][24][64] (dp and arg null) or, with dy null, rebuilt inside the kernel from the pooled gradient dp
// [B][12][12][64] and the argmax bytes arg of dmlc_f32_relu_pool_fwd, bit-identical to dmlc_f32_relu_pool_bwd's
// output (any byte value is safe: bytes are compared, never used as an address).  groups: image groups =
// partial sums per output element, 0 = one per CU, clamped to B; bit-reproducible for a fixed (B, groups).
// ws: the partials, written and read by this call only; _plan returns the group count G used and the floats
// ws must hold.  Every pointer 16-byte aligned.
hipError_t dmlc_f32_conv1_wgrad_plan(int B, int groups, int* G, size_t* ws_floats);
hipError_t dmlc_f32_conv1_wgrad(const float* x, const float* dy, const float* dp, const uint8_t* arg, float* out,
                                float* ws, int B, int groups, hipStream_t s);

// csrc/kernels/f32_pool.hip: the ReLU + TF-SAME 3x3/2 max-pool of a conv stage and the loss head.
// k_f32_relu_pool_fwd: y NHWC [B][H][H][64] (H = 24 or 12) -> p [B][H/2][H/2][64] = pool(relu(y)) and
// arg (same shape, one byte each) = kh*3 + kw of the window's first maximum, 255 where it is <= 0.
// blocks: workgroups of the grid-stride loop over the launch's units (0: the default cap).  Every
// pointer 16-byte aligned.
hipError_t dmlc_f32_relu_pool_fwd(const float* y, float* p, uint8_t* arg, int B, int H, int blocks, hipStream_t s);
// k_f32_relu_pool_bwd: dp, arg [B][H/2][H/2][64] -> dy [B][H][H][64], the gradient at the conv output
// (pool and ReLU backward; every element written, fixed summation order).
hipError_t dmlc_f32_relu_pool_bwd(const float* dp, const uint8_t* arg, float* dy, int B, int H, int blocks,
                                  hipStream_t s);
// k_f32_xent_head: logits [B][10] (before the optional logit ReLU), labels [B] (int32, or int64 with
// labels64) -> *loss = mean softmax cross-entropy (of relu(logits) with relu_logits), *hits = rows whose
// first maximum is the label, dlogits [B][10] = d loss / d logits.  One workgroup, deterministic.
hipError_t dmlc_f32_xent_head(const float* logits, const void* labels, int labels64, float* dlogits, float* loss,
                              int* hits, int B, int relu_logits, hipStream_t s);

// csrc/kernels/f32_fc.hip: the fc stack 2304 -> 384 -> 192 -> 10 behind fc1's forward, weights in the TF layout
// [in][out].  1 <= B <= DMLC_F32_FC_MAX_B; every pointer 16-byte aligned except w3, b3, logits and dlogits
// (4 bytes: their rows are 40 bytes).  No launch waits on another workgroup; all results are bit-reproducible.
#define DMLC_F32_FC_MAX_B (1 << 19)
// k_f32_fc_tail_fwd: h1 [B][384] = relu(x W1 + b1) -> h2 [B][192] = relu(h1 W2 + b2), logits [B][10] = h2 W3 + b3.
hipError_t dmlc_f32_fc_tail_fwd(const float* h1, const float* w2, const float* b2, const float* w3, const float* b3,
                                float* h2, float* logits, int B, hipStream_t s);
// k_f32_fc_tail_bwd: dh2 [B][192] = (dlogits W3^T) where h2 > 0, else 0; dh1 [B][384] = (dh2 W2^T) where h1 > 0.
hipError_t dmlc_f32_fc_tail_bwd(const float* dlogits, const float* h1, const float* h2, const float* w2, const float* w3,
                                float* dh2, float* dh1, int B, hipStream_t s);
// k_f32_fc_grads, one launch: g1 [2305][384] = x^T dh1, g2 [385][192] = h1^T dh2, g3 [193][10] = h2^T dlogits, the
// last row of each the bias gradient (the column sums of dh1 / dh2 / dlogits); dx [B][2304] = dh1 W1^T, skipped
// when dx is null.  x [B][2304].
hipError_t dmlc_f32_fc_grads(const float* x, const float* h1, const float* h2, const float* dh1, const float* dh2,
                             const float* dlogits, const float* w1, float* g1, float* g2, float* g3, float* dx, int B,
                             hipStream_t s);

}  // extern "C"
