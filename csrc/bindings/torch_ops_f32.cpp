// torch.ops.dmlc.f32_* bindings of the fp32 kernels (csrc/kernels/f32_gemm.hip, f32_conv.hip, f32_conv1.hip, f32_pool.hip, f32_fc.hip): the building blocks
// of the fp32-accurate CNN path (ops/f32.py).  Functional ops (they allocate their outputs on the
// caching allocator and launch on the current HIP stream, so they compose with autograd and are
// capturable into HIP graphs); every launch is preceded by a full shape / dtype / layout check.
#include <c10/core/DeviceGuard.h>

#include <algorithm>
#include <tuple>

#include "../kernels/api_f32.h"
#include "check.h"

namespace {

using namespace dmlc_bind;

void f32_in(const Tensor& t, const char* n, int64_t dim) {
  dev(t, n);
  TORCH_CHECK(t.scalar_type() == at::kFloat, n, " must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == dim, n, " must be ", dim, "-D, got ", t.sizes());
}

// split-K so that the launch has >= ~512 workgroups (256 CUs x 2) when the output tile grid alone is
// small; each slice keeps >= 256 of K (4 k-steps), and at most 128 slices (the reduction reads them
// in order)
void pick_split(int64_t M, int64_t N, int64_t K, int* splits, int* kc) {
  const int64_t tiles = ((M + 63) / 64) * ((N + 63) / 64);
  int64_t s = tiles >= 256 ? 1 : std::min<int64_t>(std::min<int64_t>((512 + tiles - 1) / tiles, 128), std::max<int64_t>(1, K / 256));
  int64_t c = ((K + s - 1) / s + 63) / 64 * 64;   // multiple of the kernel's 64-deep k-step
  s = (K + c - 1) / c;
  *splits = (int)s;
  *kc = (int)c;
}

Tensor f32_gemm(const Tensor& a, const Tensor& b, const c10::optional<Tensor>& bias, bool ta, bool tb, bool relu) {
  f32_in(a, "a", 2);
  f32_in(b, "b", 2);
  const int64_t M = ta ? a.size(1) : a.size(0), K = ta ? a.size(0) : a.size(1);
  const int64_t Kb = tb ? b.size(1) : b.size(0), N = tb ? b.size(0) : b.size(1);
  TORCH_CHECK(K == Kb, "f32_gemm: inner dimensions differ (", K, " vs ", Kb, ")");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && M < (1 << 30) && N < (1 << 30) && K < (1 << 30), "f32_gemm: bad sizes");
  TORCH_CHECK(b.device() == a.device(), "f32_gemm: a and b on different devices");
  const float* bp = nullptr;
  if (bias.has_value()) {
    check(*bias, "bias", at::kFloat, {N});
    bp = bias->data_ptr<float>();
  }
  const c10::DeviceGuard g(a.device());
  auto out = at::empty({M, N}, a.options());
  int splits, kc;
  pick_split(M, N, K, &splits, &kc);
  Tensor ws;
  if (splits > 1) ws = at::empty({splits, M, N}, a.options());
  CHECK_HIP(dmlc_f32_gemm(a.data_ptr<float>(), b.data_ptr<float>(), bp, out.data_ptr<float>(),
                          splits > 1 ? ws.data_ptr<float>() : nullptr, (int)M, (int)N, (int)K, (int)a.size(1),
                          (int)b.size(1), ta, tb, relu, splits, kc, 0, stream_of(a)));
  return out;
}

// implicit-im2col convolution GEMM (geometries of the reference CNN at the 24x24 crop):
//   ta = false: out[B*HW*HW][N] = im2col(x) . w   (w [25*C][N]; forward, or data gradient with the
//               flipped / transposed weight)
//   ta = true : out[25*C (+1)][N] = im2col(x)^T . w  (w = dY [B*HW*HW][N]; weight gradient, and with
//               ones the bias gradient as the last row)
Tensor f32_conv_gemm(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, bool ta, bool ones) {
  f32_in(x, "x", 4);
  f32_in(w, "w", 2);
  const int64_t B = x.size(0), H = x.size(1), C = x.size(3);
  TORCH_CHECK(x.size(2) == H, "f32_conv_gemm: square images expected");
  int geom = 0;
  if (H == 24 && C == 3) geom = 1;
  else if (H == 12 && C == 64) geom = 2;
  TORCH_CHECK(geom != 0, "f32_conv_gemm: no implicit geometry for [", H, "x", H, "x", C, "] (use im2col)");
  TORCH_CHECK(!ones || ta, "f32_conv_gemm: the ones column is a weight-gradient option");
  TORCH_CHECK(w.device() == x.device(), "f32_conv_gemm: x and w on different devices");
  const int64_t pix = B * H * H, kc = 25 * C;
  TORCH_CHECK(pix > 0 && pix < (1 << 30), "f32_conv_gemm: bad batch");
  const int64_t M = ta ? kc + (ones ? 1 : 0) : pix, K = ta ? pix : kc, N = w.size(1);
  TORCH_CHECK(w.size(0) == K, "f32_conv_gemm: w has ", w.size(0), " rows, expected ", K);
  const float* bp = nullptr;
  if (bias.has_value()) {
    check(*bias, "bias", at::kFloat, {N});
    bp = bias->data_ptr<float>();
  }
  const c10::DeviceGuard g(x.device());
  auto out = at::empty({M, N}, x.options());
  int splits, kcs;
  pick_split(M, N, K, &splits, &kcs);
  Tensor ws;
  if (splits > 1) ws = at::empty({splits, M, N}, x.options());
  CHECK_HIP(dmlc_f32_gemm(x.data_ptr<float>(), w.data_ptr<float>(), bp, out.data_ptr<float>(),
                          splits > 1 ? ws.data_ptr<float>() : nullptr, (int)M, (int)N, (int)K, 0, (int)N, ta, false,
                          false, splits, kcs, geom, stream_of(x)));
  return out;
}

// Direct conv2 (f32_conv.hip): x fp32 NHWC [B, 12, 12, 64], w the HWIO weight [5, 5, 64, 64] (or its
// [1600, 64] view) -> [B, 12, 12, 64].  dgrad = false: conv(x, w) + bias; dgrad = true: x is dY and the result
// dX, with w read in place as the flipped, transposed weight (no bias).  blocks: workgroups (0: one per CU).
Tensor f32_conv2_direct(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, bool dgrad,
                        int64_t blocks) {
  f32_in(x, "x", 4);
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= (1 << 20) && x.size(1) == 12 && x.size(2) == 12 && x.size(3) == 64,
              "f32_conv2_direct: x must be [1 <= B <= 2^20, 12, 12, 64], got ", x.sizes());
  f32_in(w, "w", w.dim() == 2 ? 2 : 4);
  TORCH_CHECK(w.sizes() == at::IntArrayRef({5, 5, 64, 64}) || w.sizes() == at::IntArrayRef({1600, 64}),
              "f32_conv2_direct: w must be [5, 5, 64, 64] or [1600, 64], got ", w.sizes());
  TORCH_CHECK(w.device() == x.device(), "f32_conv2_direct: x and w on different devices");
  TORCH_CHECK(blocks >= 0 && blocks < (1ll << 31), "f32_conv2_direct: blocks must be >= 0 (0: one workgroup per CU)");
  const float* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(!dgrad, "f32_conv2_direct: the data gradient takes no bias");
    check(*bias, "bias", at::kFloat, {64});
    TORCH_CHECK(bias->device() == x.device(), "f32_conv2_direct: x and bias on different devices");
    bp = bias->data_ptr<float>();
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(bp) % 16 == 0,
              "f32_conv2_direct: x, w and bias must be 16-byte aligned");
  const c10::DeviceGuard g(x.device());
  auto y = at::empty({x.size(0), 12, 12, 64}, x.options());
  CHECK_HIP(dmlc_f32_conv2(x.data_ptr<float>(), w.data_ptr<float>(), bp, y.data_ptr<float>(), (int)x.size(0),
                           dgrad ? 1 : 0, (int)blocks, stream_of(x)));
  return y;
}

// Direct conv2 weight + bias gradient (f32_conv.hip k_f32_conv2_wgrad): x, dy fp32 NHWC [B, 12, 12, 64] ->
// [1601, 64], the layout of f32_conv_gemm(x, dy, None, True, True).  groups: image groups = partial sums per
// element (0: CUs / 4, always clamped to B); the partials live in a workspace of this call.
Tensor f32_conv2_wgrad(const Tensor& x, const Tensor& dy, int64_t groups) {
  f32_in(x, "x", 4);
  f32_in(dy, "dy", 4);
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= (1 << 20) && x.size(1) == 12 && x.size(2) == 12 && x.size(3) == 64,
              "f32_conv2_wgrad: x must be [1 <= B <= 2^20, 12, 12, 64], got ", x.sizes());
  TORCH_CHECK(dy.sizes() == x.sizes(), "f32_conv2_wgrad: dy must have x's shape ", x.sizes(), ", got ", dy.sizes());
  TORCH_CHECK(dy.device() == x.device(), "f32_conv2_wgrad: x and dy on different devices");
  TORCH_CHECK(groups >= 0 && groups < (1ll << 31), "f32_conv2_wgrad: groups must be >= 0 (0: CUs / 4)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 == 0,
              "f32_conv2_wgrad: x and dy must be 16-byte aligned");
  const c10::DeviceGuard g(x.device());
  int G = 0;
  size_t n = 0;
  CHECK_HIP(dmlc_f32_conv2_wgrad_plan((int)x.size(0), (int)groups, &G, &n));
  auto ws = at::empty({(int64_t)n}, x.options());
  auto out = at::empty({1601, 64}, x.options());
  CHECK_HIP(dmlc_f32_conv2_wgrad(x.data_ptr<float>(), dy.data_ptr<float>(), out.data_ptr<float>(), ws.data_ptr<float>(),
                                 (int)x.size(0), G, stream_of(x)));
  return out;
}

// Direct conv1 weight + bias gradient (f32_conv1.hip): x fp32 NHWC [B, 24, 24, 3] and the gradient at the conv
// output -> [76, 64], the layout of f32_conv_gemm(x, dy, None, True, True).  f32_conv1_wgrad takes dy fp32
// [B, 24, 24, 64]; f32_conv1_wgrad_pool takes the pooled gradient dp fp32 [B, 12, 12, 64] and the argmax bytes
// of f32_relu_pool_fwd and rebuilds dy inside the kernel (f32_relu_pool_bwd's output, bit for bit, never in
// memory).  groups: image groups = partial sums per element (0: the CU count, always clamped to B).
Tensor conv1_wgrad(const char* op, const Tensor& x, const Tensor* dy, const Tensor* dp, const Tensor* arg, int64_t groups) {
  f32_in(x, "x", 4);
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= (1 << 20) && x.size(1) == 24 && x.size(2) == 24 && x.size(3) == 3, op,
              ": x must be [1 <= B <= 2^20, 24, 24, 3], got ", x.sizes());
  const int64_t B = x.size(0);
  const Tensor& g = dy ? *dy : *dp;
  const char* gn = dy ? "dy" : "dp";
  const int64_t H = dy ? 24 : 12;
  check(g, gn, at::kFloat, {B, H, H, 64});
  TORCH_CHECK(g.device() == x.device(), op, ": x and ", gn, " on different devices");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0, op,
              ": x and ", gn, " must be 16-byte aligned");
  const uint8_t* ap = nullptr;
  if (arg) {
    check(*arg, "arg", at::kByte, {B, 12, 12, 64});
    TORCH_CHECK(arg->device() == x.device(), op, ": x and arg on different devices");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(arg->data_ptr()) % 16 == 0, op, ": arg must be 16-byte aligned");
    ap = arg->data_ptr<uint8_t>();
  }
  TORCH_CHECK(groups >= 0 && groups < (1ll << 31), op, ": groups must be >= 0 (0: one per CU)");
  const c10::DeviceGuard guard(x.device());
  int G = 0;
  size_t n = 0;
  CHECK_HIP(dmlc_f32_conv1_wgrad_plan((int)B, (int)groups, &G, &n));
  auto ws = at::empty({(int64_t)n}, x.options());
  auto out = at::empty({76, 64}, x.options());
  CHECK_HIP(dmlc_f32_conv1_wgrad(x.data_ptr<float>(), dy ? g.data_ptr<float>() : nullptr, dy ? nullptr : g.data_ptr<float>(),
                                 ap, out.data_ptr<float>(), ws.data_ptr<float>(), (int)B, G, stream_of(x)));
  return out;
}

Tensor f32_conv1_wgrad(const Tensor& x, const Tensor& dy, int64_t groups) {
  return conv1_wgrad("f32_conv1_wgrad", x, &dy, nullptr, nullptr, groups);
}

Tensor f32_conv1_wgrad_pool(const Tensor& x, const Tensor& dp, const Tensor& arg, int64_t groups) {
  return conv1_wgrad("f32_conv1_wgrad_pool", x, nullptr, &dp, &arg, groups);
}

Tensor f32_im2col(const Tensor& x, int64_t kh, int64_t kw, int64_t pad) {
  f32_in(x, "x", 4);
  TORCH_CHECK(kh > 0 && kw > 0 && pad >= 0 && pad < kh && pad < kw, "f32_im2col: bad kernel/pad");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(B * H * W * kh * kw * C < ((int64_t)1 << 40), "f32_im2col: too large");
  const c10::DeviceGuard g(x.device());
  auto cols = at::empty({B * H * W, kh * kw * C}, x.options());
  CHECK_HIP(dmlc_f32_im2col(x.data_ptr<float>(), cols.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C, (int)kh,
                            (int)kw, (int)pad, stream_of(x)));
  return cols;
}

Tensor f32_col2im(const Tensor& dcols, int64_t B, int64_t H, int64_t W, int64_t C, int64_t kh, int64_t kw,
                  int64_t pad) {
  check(dcols, "dcols", at::kFloat, {B * H * W, kh * kw * C});
  TORCH_CHECK(pad >= 0 && pad < kh && pad < kw, "f32_col2im: bad kernel/pad");
  const c10::DeviceGuard g(dcols.device());
  auto dx = at::empty({B, H, W, C}, dcols.options());
  CHECK_HIP(dmlc_f32_col2im(dcols.data_ptr<float>(), dx.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C, (int)kh,
                            (int)kw, (int)pad, stream_of(dcols)));
  return dx;
}

Tensor f32_colsum(const Tensor& x) {
  f32_in(x, "x", 2);
  const int64_t M = x.size(0), N = x.size(1);
  TORCH_CHECK(M > 0 && N > 0 && M < (1 << 30) && N < (1 << 30), "f32_colsum: bad sizes");
  const c10::DeviceGuard g(x.device());
  const int splits = (int)std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(1, M / 32), 128),
                                            std::max<int64_t>(1, 2048 / ((N + 63) / 64)));
  auto ws = at::empty({splits, N}, x.options());
  auto out = at::empty({N}, x.options());
  CHECK_HIP(dmlc_f32_colsum(x.data_ptr<float>(), out.data_ptr<float>(), ws.data_ptr<float>(), (int)M, (int)N, splits,
                            stream_of(x)));
  return out;
}

// ReLU + TF-SAME 3x3/2 max-pool of a conv output (f32_pool.hip): y fp32 NHWC [B, H, H, 64], H = 24 or 12 ->
// (p fp32 [B, H/2, H/2, 64] = pool(relu(y)), arg uint8 of the same shape = kh*3 + kw of the first maximum,
// 255 where the window's maximum is <= 0).  blocks: workgroups of the grid-stride loop (0: default).
void pool_geom(const Tensor& t, const char* n, int64_t h0, int64_t h1, int64_t blocks) {
  TORCH_CHECK(t.dim() == 4 && t.size(0) >= 1 && t.size(0) <= (1 << 20) && (t.size(1) == h0 || t.size(1) == h1) &&
                  t.size(2) == t.size(1) && t.size(3) == 64,
              n, " must be [1 <= B <= 2^20, H, H, 64] with H = ", h0, " or ", h1, ", got ", t.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, n, " must be 16-byte aligned");
  TORCH_CHECK(blocks >= 0 && blocks < (1ll << 31), "blocks must be >= 0 (0: the default grid)");
}

std::tuple<Tensor, Tensor> f32_relu_pool_fwd(const Tensor& y, int64_t blocks) {
  f32_in(y, "y", 4);
  pool_geom(y, "y", 24, 12, blocks);
  const int64_t B = y.size(0), H = y.size(1);
  const c10::DeviceGuard g(y.device());
  auto p = at::empty({B, H / 2, H / 2, 64}, y.options());
  auto arg = at::empty({B, H / 2, H / 2, 64}, y.options().dtype(at::kByte));
  CHECK_HIP(dmlc_f32_relu_pool_fwd(y.data_ptr<float>(), p.data_ptr<float>(), arg.data_ptr<uint8_t>(), (int)B, (int)H,
                                   (int)blocks, stream_of(y)));
  return {p, arg};
}

// Its backward and the ReLU's in one pass: dp fp32, arg uint8 [B, H/2, H/2, 64] -> dy fp32 [B, H, H, 64].
Tensor f32_relu_pool_bwd(const Tensor& dp, const Tensor& arg, int64_t blocks) {
  f32_in(dp, "dp", 4);
  pool_geom(dp, "dp", 12, 6, blocks);
  check(arg, "arg", at::kByte, dp.sizes().vec());
  TORCH_CHECK(arg.device() == dp.device(), "f32_relu_pool_bwd: dp and arg on different devices");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(arg.data_ptr()) % 16 == 0, "arg must be 16-byte aligned");
  const int64_t B = dp.size(0), H = 2 * dp.size(1);
  const c10::DeviceGuard g(dp.device());
  auto dy = at::empty({B, H, H, 64}, dp.options());
  CHECK_HIP(dmlc_f32_relu_pool_bwd(dp.data_ptr<float>(), arg.data_ptr<uint8_t>(), dy.data_ptr<float>(), (int)B, (int)H,
                                   (int)blocks, stream_of(dp)));
  return dy;
}

// Softmax cross-entropy head (f32_pool.hip): logits fp32 [B, 10] (before the optional logit ReLU), labels int32
// or int64 [B] -> (loss fp32 [] = mean cross-entropy, of relu(logits) with relu_logits; hits int32 [] = rows
// whose first maximum is the label; dlogits fp32 [B, 10] = d loss / d logits).
std::tuple<Tensor, Tensor, Tensor> f32_xent_head(const Tensor& logits, const Tensor& labels, bool relu_logits) {
  f32_in(logits, "logits", 2);
  const int64_t B = logits.size(0);
  TORCH_CHECK(B >= 1 && B <= (1 << 27) && logits.size(1) == 10, "logits must be [1 <= B <= 2^27, 10], got ",
              logits.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 8 == 0, "logits must be 8-byte aligned");
  const bool l64 = labels.scalar_type() == at::kLong;
  check(labels, "labels", l64 ? at::kLong : at::kInt, {B});
  TORCH_CHECK(labels.device() == logits.device(), "f32_xent_head: logits and labels on different devices");
  const c10::DeviceGuard g(logits.device());
  auto loss = at::empty({}, logits.options());
  auto hits = at::empty({}, logits.options().dtype(at::kInt));
  auto dl = at::empty({B, 10}, logits.options());
  CHECK_HIP(dmlc_f32_xent_head(logits.data_ptr<float>(), labels.data_ptr(), l64 ? 1 : 0, dl.data_ptr<float>(),
                               loss.data_ptr<float>(), hits.data_ptr<int>(), (int)B, relu_logits ? 1 : 0,
                               stream_of(logits)));
  return {loss, hits, dl};
}

// The fc stack behind fc1's forward (f32_fc.hip), 2304 -> 384 -> 192 -> 10, weights [in, out].  fc_arg: one
// operand checked in full -- GPU, contiguous, fp32, the exact shape, on `on`'s device, `align`-byte aligned.
void fc_arg(const char* op, const Tensor& t, const char* n, std::vector<int64_t> shape, const Tensor& on, int align) {
  check(t, n, at::kFloat, std::move(shape));
  TORCH_CHECK(t.device() == on.device(), op, ": ", n, " is on another device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0, op, ": ", n, " must be ", align, "-byte aligned");
}

int64_t fc_batch(const char* op, const Tensor& t, const char* n, int64_t cols) {
  TORCH_CHECK(t.dim() == 2 && t.size(1) == cols && t.size(0) >= 1 && t.size(0) <= DMLC_F32_FC_MAX_B, op, ": ", n,
              " must be [1 <= B <= 2^19, ", cols, "], got ", t.sizes());
  return t.size(0);
}

// h1 [B, 384] = relu(x W1 + b1) -> (h2 [B, 192] = relu(h1 W2 + b2), logits [B, 10] = h2 W3 + b3)
std::tuple<Tensor, Tensor> f32_fc_tail_fwd(const Tensor& h1, const Tensor& w2, const Tensor& b2, const Tensor& w3,
                                           const Tensor& b3) {
  const char* op = "f32_fc_tail_fwd";
  const int64_t B = fc_batch(op, h1, "h1", 384);
  fc_arg(op, h1, "h1", {B, 384}, h1, 16);
  fc_arg(op, w2, "w2", {384, 192}, h1, 16);
  fc_arg(op, b2, "b2", {192}, h1, 16);
  fc_arg(op, w3, "w3", {192, 10}, h1, 4);
  fc_arg(op, b3, "b3", {10}, h1, 4);
  const c10::DeviceGuard g(h1.device());
  auto h2 = at::empty({B, 192}, h1.options());
  auto logits = at::empty({B, 10}, h1.options());
  CHECK_HIP(dmlc_f32_fc_tail_fwd(h1.data_ptr<float>(), w2.data_ptr<float>(), b2.data_ptr<float>(), w3.data_ptr<float>(),
                                 b3.data_ptr<float>(), h2.data_ptr<float>(), logits.data_ptr<float>(), (int)B,
                                 stream_of(h1)));
  return {h2, logits};
}

// -> (dh2 [B, 192] = (dlogits W3^T) where h2 > 0, dh1 [B, 384] = (dh2 W2^T) where h1 > 0; 0 elsewhere)
std::tuple<Tensor, Tensor> f32_fc_tail_bwd(const Tensor& dlogits, const Tensor& h1, const Tensor& h2, const Tensor& w2,
                                           const Tensor& w3) {
  const char* op = "f32_fc_tail_bwd";
  const int64_t B = fc_batch(op, dlogits, "dlogits", 10);
  fc_arg(op, dlogits, "dlogits", {B, 10}, dlogits, 4);
  fc_arg(op, h1, "h1", {B, 384}, dlogits, 16);
  fc_arg(op, h2, "h2", {B, 192}, dlogits, 16);
  fc_arg(op, w2, "w2", {384, 192}, dlogits, 16);
  fc_arg(op, w3, "w3", {192, 10}, dlogits, 4);
  const c10::DeviceGuard g(dlogits.device());
  auto dh2 = at::empty({B, 192}, h1.options());
  auto dh1 = at::empty({B, 384}, h1.options());
  CHECK_HIP(dmlc_f32_fc_tail_bwd(dlogits.data_ptr<float>(), h1.data_ptr<float>(), h2.data_ptr<float>(),
                                 w2.data_ptr<float>(), w3.data_ptr<float>(), dh2.data_ptr<float>(), dh1.data_ptr<float>(),
                                 (int)B, stream_of(dlogits)));
  return {dh2, dh1};
}

// One launch -> (gw1b [2305, 384] = x^T dh1, gw2b [385, 192] = h1^T dh2, gw3b [193, 10] = h2^T dlogits, each with
// the bias gradient as its last row; dx [B, 2304] = dh1 W1^T, or None without need_dx)
std::tuple<Tensor, Tensor, Tensor, c10::optional<Tensor>> f32_fc_grads(const Tensor& x, const Tensor& h1, const Tensor& h2,
                                                                       const Tensor& dh1, const Tensor& dh2,
                                                                       const Tensor& dlogits, const Tensor& w1,
                                                                       bool need_dx) {
  const char* op = "f32_fc_grads";
  const int64_t B = fc_batch(op, x, "x", 2304);
  fc_arg(op, x, "x", {B, 2304}, x, 16);
  fc_arg(op, h1, "h1", {B, 384}, x, 16);
  fc_arg(op, h2, "h2", {B, 192}, x, 16);
  fc_arg(op, dh1, "dh1", {B, 384}, x, 16);
  fc_arg(op, dh2, "dh2", {B, 192}, x, 16);
  fc_arg(op, dlogits, "dlogits", {B, 10}, x, 4);
  fc_arg(op, w1, "w1", {2304, 384}, x, 16);
  const c10::DeviceGuard g(x.device());
  auto g1 = at::empty({2305, 384}, x.options());
  auto g2 = at::empty({385, 192}, x.options());
  auto g3 = at::empty({193, 10}, x.options());
  c10::optional<Tensor> dx;
  if (need_dx) dx = at::empty({B, 2304}, x.options());
  CHECK_HIP(dmlc_f32_fc_grads(x.data_ptr<float>(), h1.data_ptr<float>(), h2.data_ptr<float>(), dh1.data_ptr<float>(),
                              dh2.data_ptr<float>(), dlogits.data_ptr<float>(), w1.data_ptr<float>(), g1.data_ptr<float>(),
                              g2.data_ptr<float>(), g3.data_ptr<float>(), need_dx ? dx->data_ptr<float>() : nullptr, (int)B,
                              stream_of(x)));
  return {g1, g2, g3, dx};
}

// The whole eval-mode forward in true fp32, one launch (f32_infer.hip): image i is data[idx[i]] (idx None:
// data[i], N = data rows); writes logits [N, 10] and, when given, pred [N] and correct [N] (needs labels,
// one per data row).  flat: the model's fp32 parameter buffer, off: the element offsets of its ten TF-layout
// tensors (conv1 kernel, bias, conv2 kernel, bias, fc1 weight, bias, fc2, fc3 likewise); scratch: fp32
// [S, 16, 2304] with S >= the launch's workgroups, min(ceil(N / 16), blocks or the CUs).
void f32_cnn_infer(const Tensor& data, const c10::optional<Tensor>& idx, const c10::optional<Tensor>& labels,
                   int64_t cy, int64_t cx, const Tensor& flat, at::IntArrayRef off, bool relu_logits,
                   const Tensor& scratch, const Tensor& logits, const c10::optional<Tensor>& pred,
                   const c10::optional<Tensor>& correct, int64_t blocks) {
  check_data(data);
  const int64_t rows = data.size(0), N = idx.has_value() ? idx->numel() : rows;
  TORCH_CHECK(rows >= 1 && rows < (1ll << 31) / 3072 * 16, "f32_cnn_infer: data rows out of range");
  TORCH_CHECK(N >= 1 && N < (1ll << 31) / 10, "f32_cnn_infer: 1 <= N < 2^31 / 10");
  TORCH_CHECK(blocks >= 0 && blocks < (1ll << 31), "f32_cnn_infer: blocks must be >= 0 (0: one workgroup per CU)");
  TORCH_CHECK(cy >= 0 && cy <= 8 && cx >= 0 && cx <= 8, "f32_cnn_infer: crop offsets must be in [0,8]");
  const auto same_dev = [&](const Tensor& t, const char* n) {
    TORCH_CHECK(t.device() == data.device(), "f32_cnn_infer: ", n, " must be on data's device");
  };
  DmlcF32InferArgs a;
  memset(&a, 0, sizeof(a));
  a.data = data.data_ptr<uint8_t>(); a.nrows = (int)rows;
  a.N = (int)N; a.cy = (int)cy; a.cx = (int)cx; a.blocks = (int)blocks; a.relu_logits = relu_logits ? 1 : 0;
  if (idx.has_value()) {
    check_numel(*idx, "idx", at::kInt, N);
    same_dev(*idx, "idx");
    a.idx = idx->data_ptr<int>();
  }
  if (labels.has_value()) {
    check_numel(*labels, "labels", at::kInt, rows);
    same_dev(*labels, "labels");
    a.labels = labels->data_ptr<int>();
  }
  // the ten parameter tensors: in order, inside flat, each on a 16-byte boundary (the kernel reads the
  // biases as 16-B vectors)
  static const int64_t numel[10] = {75 * 64, 64, 1600 * 64, 64, 2304 * 384, 384, 384 * 192, 192, 192 * 10, 10};
  f32_in(flat, "flat", 1);
  same_dev(flat, "flat");
  TORCH_CHECK(off.size() == 10, "f32_cnn_infer: off must hold the 10 parameter offsets, got ", off.size());
  int64_t end = 0;
  for (int i = 0; i < 10; ++i) {
    TORCH_CHECK(off[i] >= end && off[i] % 4 == 0, "f32_cnn_infer: parameter offset ", i, " (", off[i],
                ") overlaps its predecessor or is not 16-byte aligned");
    end = off[i] + numel[i];
  }
  TORCH_CHECK(flat.numel() >= end, "f32_cnn_infer: flat has ", flat.numel(), " elements, the parameters need ", end);
  const float* f = flat.data_ptr<float>();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(f) % 16 == 0, "f32_cnn_infer: flat must be 16-byte aligned");
  a.w1 = f + off[0]; a.b1 = f + off[1]; a.w2 = f + off[2]; a.b2 = f + off[3]; a.fw1 = f + off[4]; a.fb1 = f + off[5];
  a.fw2 = f + off[6]; a.fb2 = f + off[7]; a.fw3 = f + off[8]; a.fb3 = f + off[9];
  const c10::DeviceGuard guard(data.device());
  int grid = 0;
  CHECK_HIP(dmlc_f32_infer_grid((int)N, (int)blocks, &grid));
  dev(scratch, "scratch");
  same_dev(scratch, "scratch");
  TORCH_CHECK(scratch.scalar_type() == at::kFloat && scratch.dim() == 3 && scratch.size(1) == 16 &&
                  scratch.size(2) == 2304 && scratch.size(0) >= grid,
              "f32_cnn_infer: scratch must be fp32 [S >= ", grid, " workgroups, 16, 2304], got ", scratch.sizes());
  a.scratch = scratch.data_ptr<float>(); a.scratch_slabs = (int)std::min<int64_t>(scratch.size(0), 1 << 30);
  check(logits, "logits", at::kFloat, {N, 10});
  same_dev(logits, "logits");
  a.logits = logits.data_ptr<float>();
  if (pred.has_value()) {
    check_numel(*pred, "pred", at::kInt, N);
    same_dev(*pred, "pred");
    a.pred = pred->data_ptr<int>();
  }
  if (correct.has_value()) {
    TORCH_CHECK(labels.has_value(), "f32_cnn_infer: correct needs labels");
    check_numel(*correct, "correct", at::kInt, N);
    same_dev(*correct, "correct");
    a.correct = correct->data_ptr<int>();
  }
  CHECK_HIP(dmlc_f32_infer(&a, stream_of(data)));
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(dmlc, m) {
  m.def("f32_cnn_infer(Tensor data, Tensor? idx, Tensor? labels, int cy, int cx, Tensor flat, int[] off, "
        "bool relu_logits, Tensor(a!) scratch, Tensor(b!) logits, Tensor(c!)? pred, Tensor(d!)? correct, "
        "int blocks=0) -> ()");
  m.def("f32_gemm(Tensor a, Tensor b, Tensor? bias, bool ta, bool tb, bool relu) -> Tensor");
  m.def("f32_conv_gemm(Tensor x, Tensor w, Tensor? bias, bool ta, bool ones) -> Tensor");
  m.def("f32_conv2_direct(Tensor x, Tensor w, Tensor? bias, bool dgrad, int blocks=0) -> Tensor");
  m.def("f32_conv2_wgrad(Tensor x, Tensor dy, int groups=0) -> Tensor");
  m.def("f32_conv1_wgrad(Tensor x, Tensor dy, int groups=0) -> Tensor");
  m.def("f32_conv1_wgrad_pool(Tensor x, Tensor dp, Tensor arg, int groups=0) -> Tensor");
  m.def("f32_im2col(Tensor x, int kh, int kw, int pad) -> Tensor");
  m.def("f32_col2im(Tensor dcols, int B, int H, int W, int C, int kh, int kw, int pad) -> Tensor");
  m.def("f32_colsum(Tensor x) -> Tensor");
  m.def("f32_relu_pool_fwd(Tensor y, int blocks=0) -> (Tensor, Tensor)");
  m.def("f32_relu_pool_bwd(Tensor dp, Tensor arg, int blocks=0) -> Tensor");
  m.def("f32_xent_head(Tensor logits, Tensor labels, bool relu_logits) -> (Tensor, Tensor, Tensor)");
  m.def("f32_fc_tail_fwd(Tensor h1, Tensor w2, Tensor b2, Tensor w3, Tensor b3) -> (Tensor, Tensor)");
  m.def("f32_fc_tail_bwd(Tensor dlogits, Tensor h1, Tensor h2, Tensor w2, Tensor w3) -> (Tensor, Tensor)");
  m.def("f32_fc_grads(Tensor x, Tensor h1, Tensor h2, Tensor dh1, Tensor dh2, Tensor dlogits, Tensor w1, "
        "bool need_dx) -> (Tensor, Tensor, Tensor, Tensor?)");
}

TORCH_LIBRARY_IMPL(dmlc, CUDA, m) {
  m.impl("f32_gemm", &f32_gemm);
  m.impl("f32_conv_gemm", &f32_conv_gemm);
  m.impl("f32_conv2_direct", &f32_conv2_direct);
  m.impl("f32_conv2_wgrad", &f32_conv2_wgrad);
  m.impl("f32_conv1_wgrad", &f32_conv1_wgrad);
  m.impl("f32_conv1_wgrad_pool", &f32_conv1_wgrad_pool);
  m.impl("f32_im2col", &f32_im2col);
  m.impl("f32_col2im", &f32_col2im);
  m.impl("f32_colsum", &f32_colsum);
  m.impl("f32_relu_pool_fwd", &f32_relu_pool_fwd);
  m.impl("f32_relu_pool_bwd", &f32_relu_pool_bwd);
  m.impl("f32_xent_head", &f32_xent_head);
  m.impl("f32_fc_tail_fwd", &f32_fc_tail_fwd);
  m.impl("f32_fc_tail_bwd", &f32_fc_tail_bwd);
  m.impl("f32_fc_grads", &f32_fc_grads);
  m.impl("f32_cnn_infer", &f32_cnn_infer);
}
