"""Path selection of the fused CIFAR engine as a pure function.

``plan_step`` decides which execution path every part of a training step takes and the buffer sizes
that follow from it; ``FusedCifarEngine.__init__`` (engine/fused.py) collects its inputs, keeps the
result as ``self.plan``, copies every field onto itself and allocates from it.  Nothing here touches
a device, ``torch.cuda`` or the native extension, so the plan of any configuration can be evaluated
(and is pinned, tests/test_plan.py) without a GPU:

    plan_step(batch_size=256, dtype="bf16", world_size=1, dp_force=False, local_world=1, ndev=8,
              cus=256, have_xgmi=False, comm_dtype="fp32")

Every default is the measured-fastest path of its configuration; the comments next to the predicates
record the A/B numbers and the profile files they came from.
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Mapping, Optional

# The engine's path choices (constructor ``variant=``).  None = chosen per configuration.
VARIANT_DEFAULTS = {
    "split_fwd": False,        # conv1 and conv2 forward as two launches (bitwise reference of conv12_fwd)
    "fc_fused": None,          # the persistent fc chain (B <= 256, one rank per GPU); env DMLC_FC_FUSED=0 off
    "fc_dgrad": None,          # conv2 dgrad inside the fc chain (default: on; two workgroups per image at B <= 128)
    "fc_dw_in_wgrad": None,    # fc dW tiles in the wgrad launch (default: only when the dgrad is not in the chain)
    "fc1_epilogue": True,      # single GPU: the fc1 update in the dW1 epilogue
    "wgrad_sgd": True,         # in-launch SGD / slab reduction of the wgrad launch; env DMLC_WGRAD_SGD=0 off
    "wgrad_sgd_fp8": False,    # the same for --dtype fp8 (bit-identical, measured 1.4 % slower at B=1024)
    "fp8_dgrad": True,         # fp8: the conv2 input gradient on e4m3 too
    "fp8_wgrad": True,         # fp8 (with fp8_dgrad): the conv2 weight gradient on e4m3 MFMA (per-batch scales)
    "comm_sgd": False,         # data parallel over xGMI: the SGD in the exchange kernel's epilogue
    "xraw_prefetch": True,     # the step's raw images gathered by the previous step's finalizer
    "fwd12_split": True,       # B <= 128: conv1 + conv2 forward in one launch, two workgroups per image;
                               # env DMLC_FWD12_SPLIT=0 off
    "fc_sgd_in_chain": None,   # single GPU, dW tiles in the fc chain: every fc SGD in their epilogues (default B < 256)
    "grad16": True,            # data parallel, RCCL, bf16 wire, fc chain: the producers write a bf16 flat gradient
                               # (no cast launches around the all-reduce; bitwise the cast path)
    "bwd_fused": None,         # single GPU, bf16, 128 < B <= 256: fc chain + conv2 dgrad + wgrad/SGD in one launch
}
# int32 words of the SGD arrival ticket (DMLC_TICKET_WORDS in csrc/kernels/api.h)
TICKET_WORDS = 9 * 32
# int32 words of the wgrad apply-mode barriers (DMLC_WBAR_WORDS); the last line is the error word
WBAR_WORDS = 20 * 32
# int32 words of the one-launch backward's per-image hand-off words (DMLC_HAND_WORDS)
HAND_WORDS = 2 * 256 * 32
# index of the sticky error word in the barrier words (DMLC_WBAR_ERR)
ERR_WORD = 10 * 32
# int32 words of the fc chain's sync words (DMLC_FC_SYNC_WORDS; fc_common.h SY_END lines)
FC_SYNC_WORDS = 212 * 32


def head_rows(B: int) -> int:
    """Batch rows per workgroup of the three-launch path's head kernel: 2 up to B=256 (more
    workgroups on the otherwise idle chip, profiles/r2_v26_head_rows_groups_sweep.txt), 4 above
    (each workgroup streams all of fc2)."""
    return 2 if B <= 256 else 4


def _pick_fc1_split(B: int) -> int:
    # the largest power-of-two split in (8, 4, 2) whose (B/64) * 6 tiles * split workgroups stay
    # <= 450: with the XCD-aware GEMM order (cnn_gemm.hip) every XCD gets its own K slice of p2
    # and W1 (split 8: one slice per XCD).  Whole-step sweeps: tools/sweep_fc.py,
    # profiles/r2_v26_fc1_split_sweep.jsonl.
    tiles = max(1, math.ceil(B / 64)) * 6
    for s in (8, 4, 2):
        if tiles * s <= 450:
            return s
    return 1


@dataclasses.dataclass(frozen=True)
class StepPlan:
    """Every path decision of one engine configuration, under the engine's attribute names, and the
    sizes its allocations need."""
    variant: dict              # VARIANT_DEFAULTS with the constructor's overrides
    B: int                     # kernel batch: padded to the 16-row MFMA tile
    Bv: int                    # the batch size asked for
    dp: bool                   # the data-parallel step (all-reduce + apply)
    fp8: bool                  # (the e4m3 shadows w2f8 / amax_x / amax_w / scale_w exist)
    fp8_dgrad: bool
    fp8_wgrad: bool            # (p1f8 / dy2f8 / sx8 / sy_img exist)
    fc1_split: int
    fused_fwd: bool
    conv_split: int
    conv1_split: int
    dgrad_split: int
    g1: int
    g2: int
    groups2: int
    fc_fused: bool
    has_h1part8: bool
    head_rows: int             # batch rows per workgroup of the head
    loss_parts: int            # elements of loss_part / correct_part
    has_grad16: bool
    fc1_epilogue: bool
    wgrad_apply: bool
    _grad_in_launch: bool
    wgrad_reduce: bool
    comm_sgd: bool
    _comm_blocks: int
    xraw_prefetch: bool
    fwd12_split: bool
    c12_flags_words: int
    fc_dgrad: bool
    fc_dw_in_wgrad: bool
    fc_sgd_in_chain: bool
    bwd_fused: bool
    bwd_hand_words: int


def plan_step(*, batch_size: int, dtype: str, world_size: int, dp_force: bool, local_world: int, ndev: int,
              cus: int, have_xgmi: bool, comm_dtype: str, conv_split: Optional[int] = None,
              conv1_split: Optional[int] = None, dgrad_split: Optional[int] = None, g1: Optional[int] = None,
              g2: Optional[int] = None, fc1_split: Optional[int] = None, variant: Optional[dict] = None,
              env: Mapping[str, str] = os.environ) -> StepPlan:
    """The paths a configuration takes.  ``local_world``: ranks on this host (LOCAL_WORLD_SIZE, else
    the world size), ``ndev`` / ``cus``: visible GPUs and compute units of this one (0 off the GPU),
    ``have_xgmi``: the gradient exchange runs over an xGMI context instead of RCCL.  ``env`` is read
    for DMLC_FC_FUSED, DMLC_WGRAD_SGD and DMLC_FWD12_SPLIT only."""
    unknown = set(variant or {}) - set(VARIANT_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown engine variant keys {sorted(unknown)}")
    V = dict(VARIANT_DEFAULTS, **(variant or {}))
    Bv = int(batch_size)
    if Bv < 1:
        raise ValueError("batch size must be >= 1")
    B = -(-Bv // 16) * 16              # kernel batch: padded to the 16-row MFMA tile
    # dp_force: run the data-parallel step (all-reduce + apply) even at world_size 1 -- exercises
    # the collective path (e.g. a captured RCCL all-reduce) on a single GPU
    dp = world_size > 1 or dp_force
    if dtype not in ("bf16", "fp8"):
        raise ValueError("fused engine dtype must be bf16 or fp8")
    # every rank has a GPU of its own: the persistent launches need their workgroups co-resident, so
    # not when several ranks share one GPU (rehearsals / tests: another rank's kernels hold CUs)
    gpu_per_rank = local_world <= max(1, ndev)

    # fp8 conv2 forward + input gradient (BASELINE config 5): e4m3 weight shadows [0] forward
    # (co-major) and [1] the dgrad's flipped ci-major copy, delayed per-tensor weight scale;
    # variant fp8_dgrad=False keeps the conv2 input gradient in bf16
    fp8 = dtype == "fp8"
    fp8_dgrad = fp8 and bool(V["fp8_dgrad"])
    # fp8 conv2 weight gradient (cnn_wgrad.hip w2_fp8_main): the e4m3 X the fp8 forward quantised
    # (per-batch scale sx) and the e4m3 dY2 the fp8 dgrad quantised (a power-of-two scale per
    # image, the MFMA's E8M0 block scale), written by those kernels next to their bf16 outputs
    fp8_wgrad = fp8_dgrad and bool(V["fp8_wgrad"])

    fc1_split = fc1_split or _pick_fc1_split(B)
    # conv1 and conv2 forward in one launch (bf16 path; variant split_fwd: two launches)
    fused_fwd = not V["split_fwd"]
    # channel-split convolutions (cnn_split.hip): conv_split = 2 runs conv1 forward (conv1_split =
    # 2 or 4 workgroups per image), conv2 forward and the conv2 input gradient as 2 workgroups per
    # image, so a small batch fills the 256 CUs; 1 = one workgroup per image (cnn_conv.hip).
    # same-session A/B (r3): B=128 73.5 us (split, conv1 2-way) vs 74.6 (conv1 4-way) vs 79.0 (one
    # workgroup per image); B=256 85.1 vs 82.9 -- the split pays only while the chip is not full
    conv_split = 1 if fp8 else (conv_split or (2 if B <= 128 else 1))
    conv1_split = conv1_split or 2
    # the conv2 input gradient's split, independently of the forward's
    dgrad_split = 1 if fp8 else (dgrad_split or conv_split)
    if conv_split not in (1, 2) or conv1_split not in (2, 4) or dgrad_split not in (1, 2):
        raise ValueError(f"conv_split / dgrad_split must be 1 or 2 and conv1_split 2 or 4 "
                         f"({conv_split}, {dgrad_split}, {conv1_split})")
    # Both weight gradients run in ONE launch (ops.wgrad) of g1 + 4 * g2 <= 256 blocks (one wave
    # of workgroups): conv2 one block per (input-channel quarter, image group), one fp32 slab per
    # group (g2 = slabs the reduction sums); conv1 one block per image group on the CUs the conv2
    # blocks leave.  Multiples of 8 keep every group's images on one XCD (cnn_wgrad.hip).
    # B=128: 32 groups of 4 images -> 69.2 us per step vs 16 groups of 8 -> 73.7 (r3 sweep);
    # B=256: 32 -> 81.7 vs 24 -> 85.1, 40 -> 83.1, 48 -> 86.8.  Past B=256 every conv1 block takes
    # several images instead of the grid growing beyond the chip.
    g2_ = max(1, min(B, 32, B // 4))
    g2 = g2 or (g2_ // 8 * 8 if g2_ >= 8 else g2_)
    g1 = g1 or max(1, min(B, 256 - 4 * g2))

    # the whole fc chain of a training step (fc1 forward, head, fc backward) as ONE persistent
    # launch (cnn_fc.hip) instead of three: B <= 256, 256 co-resident workgroups (one per CU, so
    # not when several ranks share a GPU).  DMLC_FC_FUSED=0 turns it off.
    fc_ok = B <= 256 and cus >= 256 and gpu_per_rank
    fc_fused = (fc_ok if V["fc_fused"] is None else bool(V["fc_fused"]) and fc_ok) \
        and env.get("DMLC_FC_FUSED", "1") != "0"
    # head: head_rows(B) batch rows per workgroup (B / rows workgroups share the fc2 weight reads);
    # the fused fc chain's head takes 4 rows per workgroup
    hr = 4 if fc_fused else head_rows(B)
    # data parallel over RCCL with the bf16 wire: the fc chain (its dW tiles), the wgrad launch's
    # conv-slab reduction / the reduce-only SGD launch write the gradient as bf16 into grad16, the
    # all-reduce runs on it in place and the apply-only SGD reads it (DmlcSgdArgs::grad16) -- the
    # fp32 gradient + t.to(bf16) + all-reduce + copy back, bit for bit, minus two cast launches of
    # 4.27 / 2.1 MB (world-1 A/B: +13.1 us over the single-GPU step with the casts vs +5.7 fp32,
    # profiles/r6s2_dp1_ab_grad16_bf16.jsonl).  The three-launch fc path writes fp32 only: fc chain
    # engines (B <= 256, a GPU per rank) only.
    has_grad16 = dp and comm_dtype == "bf16" and not have_xgmi and fc_fused and bool(V["grad16"])

    # single GPU: the same launch with dW1 as a fused SGD epilogue (c_mode 4) -- the fc1 weights
    # (83 % of the parameters) are updated where their gradient is produced instead of the fp32
    # gradient going through HBM to the SGD kernel (which then updates the fc1 bias only).
    # Bitwise the same update (same lr expression, same fp32 arithmetic); variant fc1_epilogue off
    fc1_epilogue = not dp and bool(V["fc1_epilogue"])
    # single GPU + fc1 epilogue: the merged weight-gradient launch also runs the rest of the SGD
    # (cnn_wgrad.hip apply mode: sub-grid barriers per slab family, the SGD kernel's reduction
    # order -> bit-identical weights) and the step has no SGD launch.  DMLC_WGRAD_SGD=0 off.
    in_launch = (1 <= g1 <= cus and 4 * g2 <= cus and bool(V["wgrad_sgd"])
                 and env.get("DMLC_WGRAD_SGD", "1") != "0")
    # fp8: bit-identical too (the e4m3 shadows + amax slots in-launch), but measured slower at
    # B=1024 (207.5 vs 204.7 us, profiles/r3_fp8_wgrad_sgd_ab.txt): variant wgrad_sgd_fp8 opts in
    wgrad_apply = in_launch and fc1_epilogue and (not fp8 or bool(V["wgrad_sgd_fp8"]))
    # data parallel: the same launch reduces the conv slabs into the flat gradient (the reduce-only
    # SGD launch before the all-reduce goes away).  Needs the launch's blocks co-resident, so not
    # when several ranks share one GPU (rehearsals / tests: another rank's kernels hold CUs).
    reduce_ok = in_launch and dp and gpu_per_rank
    # reduce-only also serves compute_gradients() on one GPU (fp8 included: bit for bit the
    # two-launch path, tests/test_fp8_gpu.py)
    grad_in_launch = in_launch and (wgrad_apply or reduce_ok)
    # the data-parallel step takes the in-launch reduction exactly when compute_gradients() does
    # (one predicate: the DP step and _conv_backward can never disagree)
    wgrad_reduce = dp and grad_in_launch
    # data parallel over xGMI, serial schedule, variant comm_sgd: the exchange kernel applies the
    # SGD in its epilogue (k_xgmi_allreduce_sgd: no SGD launch; bit-identical weights; bf16 shadows
    # only).  Off by default: measured on one GPU (tools/dp1_ab.py, world-1 xGMI context, B=256)
    # the DP step took 103.0 us with the epilogue on the exchange's 128 workgroups and 142.2 us on
    # 512 (every workgroup pays the barriers' system-scope release fences) vs 96.2 us for exchange
    # + the 800-workgroup SGD launch (profiles/r5_dp1_ab_128blocks.jsonl, r5_dp1_ab_512blocks.jsonl).
    comm_sgd = have_xgmi and not fp8 and bool(V["comm_sgd"])
    # workgroups of the exchange + SGD kernel: 2 per CU on a GPU of its own (the epilogue streams
    # the whole flat buffer); ranks sharing one GPU (rehearsals) split the workgroups, since every
    # workgroup waits at the barriers for the same-index workgroup of every peer
    share = max(1, -(-local_world // max(1, ndev)))
    comm_blocks = 512 if share == 1 else max(32, 128 // share)

    # the training forward (conv12_fwd) reads its raw images from xraw, which the previous step's
    # finalizer (wgrad apply mode, the SGD launch or the xGMI+SGD kernel) filled with the next
    # step's rows -- one image load instead of index load -> image load at the head of the step;
    # the host fills it whenever it sets the step (_sync_bidx)
    xraw_prefetch = fused_fwd and not fp8 and conv_split == 1 and bool(V["xraw_prefetch"])
    # B <= 128 (channel-split convs, conv1 in halves): conv1 -> conv2 in ONE launch whose two
    # workgroups per image swap their pool1 halves through sc1 stores + a flag (cnn_split.hip
    # k_conv12_fwd_split) -- one launch boundary and the conv2 input's global round trip less
    fwd12_split = (conv_split == 2 and conv1_split == 2 and not fp8
                   and B * 2 <= cus and gpu_per_rank and bool(V["fwd12_split"])
                   and env.get("DMLC_FWD12_SPLIT", "1") != "0")

    # the plain bf16 conv2 dgrad (one image per workgroup) runs in the fc chain's workgroups, each
    # once its dp2 row tile is published: one launch boundary less, but the hand-off (publish ->
    # poll -> sc1 dp2 loads) costs ~2 us of it back.  With the fc dW tiles kept in the chain (below)
    # it measured 1.8-2.5 us/step faster at B = 144 / 160 / 192 / 224 / 256 (profiles/
    # r4_v8_fc_dgrad_b144_256_ab.txt); at B <= 128 the chain's 256 workgroups run the split dgrad
    # (two per image, cnn_split.hip's halves) instead of its own launch (r5, profiles/
    # r5_fc_split_dgrad_b128_ab.txt).  Variant fc_dgrad forces it on / off.
    fdg = V["fc_dgrad"]
    fc_dgrad = fc_fused and not fp8_dgrad and (bool(fdg) if fdg is not None else True)
    # single GPU, fused fc chain + apply mode: the fc weight-gradient tiles and every fc SGD can run
    # in the wgrad launch's conv1 blocks (between their barrier arrival and the conv1 reduction),
    # so the fc chain launch ends with its dp2 tiles.  Same-box A/B at B=256 (profiles/
    # r4_v7_fc_dgrad_dw_ab.txt, us/step): chain dgrad off: dW in chain 81.8, in wgrad 80.4; chain
    # dgrad on: dW in chain 79.8, in wgrad 80.2 -- so by default the dW tiles move to the wgrad
    # launch only when the dgrad is not in the chain.  Variant fc_dw_in_wgrad forces it.
    # At B <= 128 (the chain's split dgrad) the dW tiles once measured better in the wgrad launch
    # (64.2-64.4 vs 65.6-65.9 us at B = 128, profiles/r5_fc_split_dgrad_b128_ab.txt) -- with the
    # conv1 blocks then too busy to help reduce the conv2 slabs.  With the tiles in the chain the
    # conv1 blocks help again (torch_ops.cpp: helpers whenever they carry no fc tiles): B = 32 71.6
    # -> 64.0, 64 65.3 -> 62.7, 96 65.8 -> 64.7, 112 67.5 -> 65.5, 128 63.6 -> 63.6 us
    # (profiles/r5_dw_placement_helpers_ab.txt).
    fdw = V["fc_dw_in_wgrad"]
    fc_dw_in_wgrad = (fc_fused and wgrad_apply
                      and (bool(fdw) if fdw is not None else not fc_dgrad))
    # the whole backward -- fc chain, conv2 dgrad, both weight gradients and the SGD -- in ONE launch
    # (cnn_bwd.hip k_backward): the chain's and the wgrad launch's 256 workgroups are the same 256, so
    # each block starts its weight-gradient role the moment its own dgrad is done and waits per image
    # instead of per launch, and the blocks that finish the chain first take the conv2 roles, which
    # end the step.  Bitwise the two launches (tests/test_bwd_fused_gpu.py).  Where: the chain with
    # its one-workgroup-per-image dgrad and its dW tiles, the wgrad launch in apply mode on the
    # full 256-block grid, bf16 state, one rank.  The fc SGD roles of the wgrad launch would read
    # the chain's flat gradient inside the launch, so this path has the chain apply every fc SGD in
    # its dW epilogues (fc_sgd_in_chain, also at B = 256) and is off when that variant is forced off.
    fsc = V["fc_sgd_in_chain"]
    bwf = V["bwd_fused"]
    bwd_ok = (fc_fused and fc_dgrad and 128 < B <= 256 and dgrad_split == 1
              and wgrad_apply and not fc_dw_in_wgrad and not fp8 and world_size == 1
              and xraw_prefetch and fsc is not False and g1 + 4 * g2 == 256
              and g1 % 8 == 0 and g2 % 8 == 0)
    bwd_fused = bool(bwd_ok and (bool(bwf) if bwf is not None else True))
    # ... and with the tiles in the chain, the chain can apply every fc SGD in their epilogues (fc2 /
    # fc3 / fc biases too, as the wgrad launch does when it runs them): the wgrad launch's conv1
    # blocks then have no fc SGD roles before their conv1 reduction and conv2 help, while the
    # chain's dW2 / dW3 tiles (whose images' dgrads end the chain) carry the transposed-shadow
    # epilogues.  Same-box A/B (profiles/r5_fc_sgd_in_chain_ab.txt): B = 64 / 128 / 160 / 192 / 224
    # -0.9 / -0.3 / -0.5 / -0.9 / -0.7 us, B = 256 +0.9 us -- on below B = 256, and wherever the
    # backward is one launch.
    fc_sgd_in_chain = bwd_fused or (fc_fused and wgrad_apply and not fc_dw_in_wgrad
                                    and (bool(fsc) if fsc is not None else B < 256))

    return StepPlan(
        variant=V, B=B, Bv=Bv, dp=dp, fp8=fp8, fp8_dgrad=fp8_dgrad, fp8_wgrad=fp8_wgrad, fc1_split=fc1_split,
        fused_fwd=fused_fwd, conv_split=conv_split, conv1_split=conv1_split, dgrad_split=dgrad_split, g1=g1, g2=g2,
        groups2=g2, fc_fused=fc_fused, has_h1part8=fc_fused, head_rows=hr, loss_parts=B // hr,
        has_grad16=has_grad16, fc1_epilogue=fc1_epilogue, wgrad_apply=wgrad_apply,
        _grad_in_launch=grad_in_launch, wgrad_reduce=wgrad_reduce, comm_sgd=comm_sgd, _comm_blocks=comm_blocks,
        xraw_prefetch=xraw_prefetch, fwd12_split=fwd12_split, c12_flags_words=32 * 2 * B if fwd12_split else 1,
        fc_dgrad=fc_dgrad, fc_dw_in_wgrad=fc_dw_in_wgrad, fc_sgd_in_chain=fc_sgd_in_chain, bwd_fused=bwd_fused,
        bwd_hand_words=HAND_WORDS if bwd_fused else 1)
