// k_wgrad: the weight gradients of the two convolutions in one launch and, in apply mode, the rest of
// the SGD step behind them.  The device code -- and the account of its layouts -- is wgrad_core.h
// (shared with cnn_bwd.hip's k_backward); this file holds the kernel, the host checks and the launcher.
#include "wgrad_core.h"

namespace dmlc {

#ifdef DMLC_EAGER_ARGS                         // A/B build: every field loaded in the entry block
#define late_args() a
#else
#define late_args() late_kernarg<DmlcWgradArgs>(0)
#endif

__global__ __launch_bounds__(W1T, 1) void k_wgrad(DmlcWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned g0 = 0, hg0 = 0;
  int64_t step = 0;
  if (a.apply) {                               // read before this block can arrive
    if (threadIdx.x == 0) wgrad_gens(a, blockIdx.x, g0, hg0);
    step = *a.sgd.step_rd;
  }
  wgrad_role<false>(a, [&]() __attribute__((always_inline)) -> const DmlcWgradArgs& { return late_args(); },
                    blockIdx.x, smem, g0, hg0, step);
}

}  // namespace dmlc

using namespace dmlc;

extern "C" {

hipError_t dmlc_wgrad_check(const DmlcWgradArgs* a) {
  if (a->apply) {
    // every barrier family must fit on the chip at once (one block per CU), fp32 slabs, the step
    // read from the head's copy (a block bumps *step while others may not have read it yet), and
    // the forward's image copy (bidx is rewritten for the next step inside this launch)
    static int cus = 0;
    if (!cus) {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return hipErrorInvalidValue;
    }
    const DmlcSgdArgs& g = a->sgd;
    // mode 1 (data parallel): the reduced conv gradients go to the flat grad (nothing else runs)
    const bool ok_mode = g.mode == 0 ? (g.step_rd != g.step && g.fc1_fused && (!g.w2f8 || (g.amax_w && g.scale_w) ) &&
                                        8 * a->w2.g2 <= 400)
                                     : g.mode == 1;
    if (a->fc_in_launch && (g.mode != 0 || !g.fc1_fused || a->fc.fuse_sgd != 2 || a->fc.B < 16 || a->fc.B > 256 ||
                            !a->fc.p2 || !a->fc.dh1 || !a->fc.mw2 || !a->fc.fc2t))
      return hipErrorInvalidValue;
    if (a->w1.g1 < 1 || a->w1.g1 > cus || 4 * a->w2.g2 > cus || !a->bar || !a->w1.xraw ||
        !ok_mode || g.part1 != a->w1.part1 ||
        g.part2 != a->w2.part2 || g.g1 != a->w1.g1 || g.g2 != a->w2.g2 || g.bidx_n > a->w1.g1 * W1T)
      return hipErrorInvalidValue;
  }
  return hipSuccess;
}

hipError_t dmlc_wgrad(const DmlcWgradArgs* a, hipStream_t s) {
  DMLC_LDS_OPTIN(&k_wgrad, WG_LDS);
  const int blocks = a->w1.g1 + 4 * a->w2.g2;
  const hipError_t e = dmlc_wgrad_check(a);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_wgrad, dim3(blocks), dim3(W1T), WG_LDS, s, *a);
  return hipGetLastError();
}

}  // extern "C"
