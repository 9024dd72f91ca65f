// The whole backward of the single-GPU bf16 step in ONE launch (128 < B <= 256): k_fc_chain's chain
// phase and ticket, the conv2 input gradient of image blockIdx, then one role of k_wgrad in apply mode
// -- the bodies of fc_chain_core.h, conv2_core.h and wgrad_core.h, unchanged; this file adds the role map
// and the per-image hand-offs between them, no arithmetic.  Bitwise the two launches' results: every
// role keeps its image order, so every slab sums in the same order.
//
// Why: both launches are 256 co-resident workgroups of 512 threads.  The chain ends skewed (the
// blocks that run a dW tile before their image's dgrad store dP1 ~3 us after the head blocks, the
// slowest ~6 us after), the whole chip then waits for them and for a launch boundary (~2 us), and
// k_wgrad's critical family -- the conv2 blocks, whose MFMA phase, quarter barrier and 13 MB slab
// reduction end the step -- needs only dY2, which every dgrad stores ~6 us BEFORE its dP1
// (profiles/bwd_fused_before.md).  Here a block starts its weight-gradient role the moment its own
// dgrad is done, prefetches what no hand-off gates (conv2: its input channels of p1; conv1: the raw
// image and the argmax bytes, all from the forward launch) and waits per image instead of per launch.
//
// Role map (bwd_role): blocks 0 .. 4 g2 - 1 -- the head and dp2 blocks, which finish their dgrad
// first -- take the conv2 roles, the rest the conv1 roles (which have slack to spare): k_wgrad's
// grid with the two families swapped.  g1 + 4 g2 == 256 and 4 g2 % 8 == 0, so role == blockIdx (mod 8)
// and every role sits on the XCD it has in k_wgrad (w2_block_pos is called with base = g1, g1 % 8 ==
// 0: `xcd` stays true).  Conv1 role r = block 4 g2 + r takes image r (from an early block) and then
// image r + g1, its own.
//
// Hand-off (common.h Hand): two words per image, "dY2 stored" and "dP1 stored", valued launch epoch
// + 1 (the chain's epoch word, read at entry by every block before any block can bump it).  The dY2
// word is posted from inside the dgrad core, behind its first barrier: that barrier waits vmcnt(0)
// for the kernel-row-0 slice anyway, so draining the dY2 stores there puts no wait in front of the
// weight-slice loads (posting from the storing waves right after the stores would).  The dP1 word
// follows the drained dP1 stores.  Consumers: see wgrad_core.h (INL).
//
// Liveness: every block finishes ALL its producing work (chain tasks, ticket, dgrad) before its first
// image wait, no chain seam depends on a weight-gradient role, and the wgrad barriers are met only by
// blocks past their dgrad -- the wait graph is acyclic with 256 co-resident blocks (host-checked).
//
// What the merged launch must order that a launch boundary ordered before (all in wgrad_core.h, INL):
//  * the conv2 SGD rewrites w2d, which every dgrad reads through its whole core: conv2_apply also
//    waits for every image's dP1 word;
//  * the loss / accuracy partials and the labels' batch rows (bidx) belong to head blocks of this
//    launch: write-through partials (head_task<true>), and the stats, the step bump and the next
//    batch rows move behind the conv1 barrier wait;
//  * the fc SGD roles would read the dW tiles' flat gradient: not supported here -- the chain applies
//    every fc SGD in the tiles' epilogues (fuse_sgd == 2, fc_done; host-checked).
#include "fc_chain_core.h"
#include "wgrad_core.h"

namespace dmlc {

static_assert(kWtStores, "dY2 / dP1 are handed off inside the launch: write-through stores only");
constexpr size_t BWD_LDS = (size_t)FC_LDS_ALL > WG_LDS ? (size_t)FC_LDS_ALL : WG_LDS;
static_assert(BWD_LDS + 64 <= 160 * 1024, "k_backward: one workgroup per CU");

// kernarg offsets of the by-value arguments (laid out in order, each at its own alignment)
constexpr unsigned ka_align(unsigned off, unsigned al) { return (off + al - 1) / al * al; }
constexpr unsigned KA_DG = kernarg_second<DmlcFcArgs, DmlcConv2DgradArgs>();
constexpr unsigned KA_WG = ka_align(KA_DG + sizeof(DmlcConv2DgradArgs), alignof(DmlcWgradArgs));
constexpr unsigned KA_HAND = ka_align(KA_WG + sizeof(DmlcWgradArgs), alignof(unsigned*));
static_assert(KA_HAND + sizeof(unsigned*) <= 4096, "k_backward: the kernarg segment stays under 4 KB");

// weight-gradient role (k_wgrad's blockIdx) of block blk: conv2 role blk on the first 4 g2 blocks,
// conv1 role blk - 4 g2 on the rest.  -DDMLC_BWD_IDENTITY_MAP builds k_wgrad's own map for A/B runs.
DEV int bwd_role(int blk, int g1) {
#ifdef DMLC_BWD_IDENTITY_MAP
  return blk;
#else
  const int n2 = FC_BLOCKS - g1;
  return blk < n2 ? g1 + blk : blk - n2;
#endif
}

__global__ __launch_bounds__(FT, 1) void k_backward(DmlcFcArgs a, DmlcConv2DgradArgs dg, DmlcWgradArgs wa,
                                                    unsigned* hand) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned s_gen[2];
  const int tid = threadIdx.x, blk = blockIdx.x;
  // The step, read once at entry and used throughout (k_wgrad reads the chain's copy instead: there a
  // block of an earlier launch phase cannot be told from a late one).  No block can enter after the
  // bump: publish_step follows the conv1 barrier wait, every conv1 role (blocks >= 4 g2) arrives there
  // itself, and every block below 4 g2 = 128 < B owns an image whose dP1 some arrival waited for.
  const int64_t step = *a.step;
  auto late_fc = [&]() __attribute__((always_inline)) -> const DmlcFcArgs& { return late_kernarg<DmlcFcArgs>(0); };
  auto late_wg = [&]() __attribute__((always_inline)) -> const DmlcWgradArgs& {
    return late_kernarg<DmlcWgradArgs>(KA_WG);
  };
  const unsigned epoch = fc_chain_phase<true>(a, late_fc, step, smem);
  const DmlcFcArgs& L = late_fc();
  const DmlcConv2DgradArgs& D = late_kernarg<DmlcConv2DgradArgs>(KA_DG);
  const Hand h = {late_kernarg<unsigned*>(KA_HAND), epoch + 1u, L.err};
  // the barrier generations of this block's role, before it can arrive (thread 0 writes and reads)
  if (tid == 0) {
    const DmlcWgradArgs& W = late_wg();
    unsigned g0 = 0, hg0 = 0;
    wgrad_gens(W, bwd_role(blk, W.w1.g1), g0, hg0);
    s_gen[0] = g0;
    s_gen[1] = hg0;
  }
  if (blk < D.B) conv2_dgrad_image<true>(D, blk, smem, seamD(L, epoch, blk >> 6), L.err, h);
  if (blk < a.B / FC_RB) DMLC_STAMP(DMLC_TK_HEAD, 7);
  else DMLC_STAMP(DMLC_TK_GEMM, 6);
  // (LDS: the dgrad ends with a workgroup barrier behind its last LDS read; a block without an image
  // passed the chain's barrier in front of the ticket)
  const DmlcWgradArgs& W = late_wg();
  unsigned g0 = 0, hg0 = 0;
  if (tid == 0) { g0 = s_gen[0]; hg0 = s_gen[1]; }
  wgrad_role<true>(W, late_wg, bwd_role(blk, W.w1.g1), smem, g0, hg0, step, h);
}

}  // namespace dmlc

using namespace dmlc;

extern "C" hipError_t dmlc_backward(const DmlcFcArgs* a, const DmlcConv2DgradArgs* dg, const DmlcWgradArgs* w,
                                    unsigned int* hand, hipStream_t s) {
  if (!dg || !hand) return hipErrorInvalidValue;
  hipError_t e = dmlc_fc_chain_check(a, dg);
  if (e == hipSuccess) e = dmlc_wgrad_check(w);
  if (e != hipSuccess) return e;
  const DmlcSgdArgs& g = w->sgd;
  // one image per workgroup and an image on every conv2-role block (128 < B); the chain applies every
  // fc SGD; apply mode 0 on bf16 state; the swapped role map needs the full grid
  if (dg->split || a->B <= 128 || a->fuse_sgd != 2 || !a->dw_tasks || !a->step || a->grad_bf16) return hipErrorInvalidValue;
  if (!w->apply || g.mode != 0 || w->fc_in_launch || !w->fc_done || g.w2f8 || w->w2.x8 || g.grad16)
    return hipErrorInvalidValue;
  if (w->w1.g1 + 4 * w->w2.g2 != FC_BLOCKS || w->w1.g1 % 8 || w->w2.g2 % 8 || w->w1.g1 > a->B) return hipErrorInvalidValue;
  if (w->w1.B != a->B || w->w2.B != a->B || g.step != a->step || w->bar + DMLC_WBAR_ERR != a->err) return hipErrorInvalidValue;
  if (w->w1.dp1 != dg->dp1 || w->w2.dy2 != dg->dy2 || g.w2d != dg->wd || g.loss_part != a->loss_part ||
      g.correct_part != a->correct_part || g.nhead != a->B / FC_RB)
    return hipErrorInvalidValue;
  DMLC_LDS_OPTIN(&k_backward, BWD_LDS);
  hipLaunchKernelGGL(k_backward, dim3(FC_BLOCKS), dim3(FT), BWD_LDS, s, *a, *dg, *w, hand);
  return hipGetLastError();
}
