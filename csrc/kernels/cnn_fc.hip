// k_fc_chain: the whole fully-connected part of a training step in ONE persistent launch (B <= 256),
// optionally with the conv2 input gradient of each workgroup's image behind it.  The device code --
// and the account of its schedule and hand-offs -- is fc_chain_core.h (shared with cnn_bwd.hip's
// k_backward); this file holds the kernel, the host checks and the launcher.
#include <string.h>

#include "fc_chain_core.h"

namespace dmlc {

#ifdef DMLC_EAGER_ARGS                         // A/B build: every field loaded in the entry block
#define late_fc() a
#define late_dg() dg
#else
#define late_fc() late_kernarg<DmlcFcArgs>(0)
#define late_dg() late_kernarg<DmlcConv2DgradArgs>(kernarg_second<DmlcFcArgs, DmlcConv2DgradArgs>())
#endif
__global__ __launch_bounds__(FT, 1) void k_fc_chain(DmlcFcArgs a, DmlcConv2DgradArgs dg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int blk = blockIdx.x;
  const int H = a.B / FC_RB;
  const int64_t step = a.step ? *a.step : 0;   // fc1 shadow parity, LR of the fused SGD
  const unsigned epoch = fc_chain_phase<false>(
      a, [&]() __attribute__((always_inline)) -> const DmlcFcArgs& { return late_fc(); }, step, smem);
  const DmlcFcArgs& L = late_fc();
  // the conv2 input gradient of image blk (dg.B = 0: a separate launch does it): its dp2 row tile
  // comes from this launch's dp2 tasks; everything else it reads was written by earlier launches
  const DmlcConv2DgradArgs& D = late_dg();
  if (D.split) {                               // B <= 128: image b's input-channel half h
    if (blk < 2 * D.B) {
      int b, h;
      split_index<2>(blk, b, h);
      conv2_dgrad_split_image<true>(D, b, h, smem, seamD(L, epoch, b >> 6), L.err);
    }
  } else if (blk < D.B) {
    conv2_dgrad_image<true>(D, blk, smem, seamD(L, epoch, blk >> 6), L.err);
  }
  if (blk < H) DMLC_STAMP(DMLC_TK_HEAD, 7);
  else DMLC_STAMP(DMLC_TK_GEMM, 6);
}

}  // namespace dmlc

using namespace dmlc;

extern "C" hipError_t dmlc_fc_chain_check(const DmlcFcArgs* a, const DmlcConv2DgradArgs* dg) {
  if (a->B < 16 || a->B > 256 || a->B % 16 != 0 || a->mtiles != (a->B + 63) / 64 || !a->sync || !a->err)
    return hipErrorInvalidValue;
  if (dg) {
    // one image per workgroup of the 256: the batch rows are the chain's, dp2 its own output
    if (dg->B != a->B || dg->dp2 != a->dp2 || !dg->am2 || !dg->wd || !dg->dp1 || !dg->dy2) return hipErrorInvalidValue;
    if (dg->split && (2 * dg->B > FC_BLOCKS || dg->B % 8)) return hipErrorInvalidValue;
  }
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return hipErrorInvalidValue;
  }
  if (cus < FC_BLOCKS) return hipErrorInvalidValue;   // every block must be co-resident (one per CU)
  return hipSuccess;
}

extern "C" hipError_t dmlc_fc_chain(const DmlcFcArgs* a, const DmlcConv2DgradArgs* dg, hipStream_t s) {
  const hipError_t e = dmlc_fc_chain_check(a, dg);
  if (e != hipSuccess) return e;
  DmlcConv2DgradArgs d;
  memset(&d, 0, sizeof(d));
  if (dg) d = *dg;
  DMLC_LDS_OPTIN(&k_fc_chain, FC_LDS_ALL);
  hipLaunchKernelGGL(k_fc_chain, dim3(FC_BLOCKS), dim3(FT), d.B ? FC_LDS_ALL : FC_LDS, s, *a, d);
  return hipGetLastError();
}
