"""Layer table, path selection and shortcut wiring of the fused ResNet-20 engine as pure functions.

``plan_resnet_step`` decides the kernel batch, the split-K groups of every weight gradient, the
backward schedule and which layer reads which shortcut; ``FusedResNetEngine.__init__``
(engine/fused_resnet.py) keeps the result as ``self.plan``, allocates from it, and its per-layer
launchers read their shortcut from it.  Nothing here touches a device, ``torch.cuda`` or the native
extension, so any configuration's plan is pinned without a GPU (tests/test_rn_plan.py).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, Optional, Sequence, Tuple

from ..models.resnet import BLOCKS, WIDTHS


def layer_table():
    """[(name prefix, cin, cout, hin, stride)] in execution order (l = 0..18)."""
    layers = [("stem", 3, 16, 32, 1)]
    cin, hin = 16, 32
    for s, w in enumerate(WIDTHS):
        for b in range(BLOCKS):
            stride = 2 if (s > 0 and b == 0) else 1
            layers.append((f"stage{s}/block{b}/a", cin, w, hin, stride))
            hin //= stride
            layers.append((f"stage{s}/block{b}/b", w, w, hin, 1))
            cin = w
    return layers


LAYERS = layer_table()
NL = len(LAYERS)
assert NL == 19


def _kp(cin):
    return (9 * max(cin, 8) + 31) // 32 * 32


def _kpd(cout):
    return (9 * cout + 31) // 32 * 32


def _block_sc_mode(b_layer: int) -> int:
    """Shortcut mode of the block whose second conv is ``b_layer`` (1 identity, 2 subsample+pad)."""
    a_layer = b_layer - 1
    return 2 if LAYERS[a_layer][4] == 2 else 1


def _pick_groups(B: int, cin: int, cout: int) -> int:
    """Split-K image groups of one wgrad (grid = groups x m-chunks): enough blocks to fill the chip
    (256) while the fp32 slabs the SGD kernel reads back stay under 16 MB per layer (64 groups for
    the 64-channel layers, 677 -> 667 us/step at B=256, profiles/r1_v17_rn_slab_cap_ab.txt).  A
    power of two in [8, B]."""
    blocks = 256
    cap = 16.0 * 2 ** 20
    mt = _kp(cin) // 16
    mc = 1 if mt <= 12 else (2 if mt <= 24 else 3)      # Wg<>::MC in resnet.hip
    lim = min(blocks / mc, cap / (_kp(cin) * cout * 4))
    g = 1 << max(0, int(math.floor(math.log2(max(1.0, lim)))))
    return int(max(1, min(B, max(8, g))))


# per-image backward (k_rn_bwd_img): the level of bwd_img_level that turns a geometry on
_IMG_LEVEL = {(16, 16, 32, 1): 1, (32, 32, 16, 1): 2}


@dataclasses.dataclass(frozen=True)
class ResNetPlan:
    """Every path decision of one engine configuration and the wiring of its 19 layers."""
    B: int                     # kernel batch: padded to the 16-image tile
    Bv: int                    # the batch size asked for
    dp: bool                   # the data-parallel step (reduce | all-reduce | apply)
    groups: Tuple[int, ...]    # split-K slabs of each layer's weight gradient (part[l].shape[0])
    wgrad_branch: bool         # the wgrads on a side stream (a second graph branch)
    merged_bwd: bool           # dgrad_l + wgrad_l in one launch (when the wgrads are not on a branch)
    sgd_split: bool            # the SGD of stages 3 and 2 on a branch beside the backward
    per_image: Tuple[bool, ...]                     # merged launch of layer l: one workgroup per image
    fwd_sc: Tuple[Tuple[int, Optional[int]], ...]   # conv_l's BN-apply prologue: (shortcut mode, l' of a[l'])
    bwd_sc: Tuple[int, ...]                         # dgrad_l's shortcut-gradient mode (its source is gy[l+1])
    sgd_points: Dict[int, Tuple[int, int]]          # sgd_split: after the bwd launch of layer l, SGD of [lo, hi)


def plan_resnet_step(*, batch_size: int, world_size: int = 1, dp_force: bool = False,
                     groups: Optional[Sequence[int]] = None, wgrad_branch: Optional[bool] = None,
                     merged_bwd: Optional[bool] = None, bwd_img_level: int = 1,
                     sgd_split: bool = False) -> ResNetPlan:
    Bv = int(batch_size)
    if Bv < 1:
        raise ValueError("batch size must be >= 1")
    # any batch size: the kernels run on the batch padded to the 16-image tile; the padding images
    # are excluded from every BatchNorm statistic and get zero loss weight / gradient (nvalid)
    B = -(-Bv // 16) * 16
    dp = world_size > 1 or dp_force     # dp_force: the all-reduce path at world_size 1 (tests)
    # per-image backward (merged backward only): bwd_img_level 0 off, 1 the 16->16 layers (their
    # wgrad keeps one slab per image anyway: _pick_groups(B, 16, 16) = min(B, 256)), 2 also the 32->32
    # stride-1 layers (one slab per image instead of B/2 groups: more slab bytes for the SGD, fewer
    # re-reads).  A layer runs per image exactly when it has one slab per image (G == B, B <= 256).
    lvl = int(bwd_img_level)
    geoms = [L[1:] for L in LAYERS]
    groups = tuple(groups or (B if (lvl >= 2 and B <= 256 and g == (32, 32, 16, 1)) else _pick_groups(B, g[0], g[1])
                              for g in geoms))
    per_image = tuple(bool(lvl >= _IMG_LEVEL.get(g, 99) and G == B) for g, G in zip(geoms, groups))
    # Backward schedule, measured per batch size (graph replay, img/s on 1 MI355X):
    #                          B=256   B=1024
    #   merged dgrad+wgrad     376 k   508 k   one launch per layer, no fork/join edges
    #   two launches, 1 stream 363 k   590 k
    #   wgrads on a branch     336 k   620 k   19 fork/join edges in the graph
    # The merged kernel runs at the occupancy of the larger (wgrad) body, which costs more than the
    # saved launches once each layer has >= ~4 dgrad workgroups per CU; wgrad_branch / merged_bwd
    # override the choice.
    wgrad_branch = (B > 256) if wgrad_branch is None else bool(wgrad_branch)
    merged_bwd = (B <= 256) if merged_bwd is None else bool(merged_bwd)
    # sgd_split=True (single GPU, merged backward): the SGD of stage 3 (layers 13-18) and of
    # stage 2 (7-12) runs on a graph branch as soon as their weight gradients are complete, beside
    # the stage-2 / stage-1 backward; the main-stream SGD does the rest and publishes the step.
    # Measured at B=256: 341 k vs 371 k img/s with one SGD launch -- the co-resident SGD blocks
    # slow the one-image-per-workgroup backward more than the hidden slab reads save: off.
    sgd_split = bool(sgd_split) and not dp and merged_bwd and not wgrad_branch
    # The shortcut wiring.  Layer l applies BN of p = l - 1 in its prologue; an even p >= 2 closes a
    # residual block, whose shortcut is a[p - 2] (the block's input).  Backwards, an odd l opens a
    # block: its input also fed the shortcut, whose gradient is that of the block's output, gy[l + 1].
    fwd_sc = tuple((_block_sc_mode(l - 1), l - 3) if (l >= 3 and l % 2 == 1) else (0, None) for l in range(NL))
    bwd_sc = tuple(_block_sc_mode(l + 1) if l % 2 == 1 else 0 for l in range(NL))
    return ResNetPlan(B=B, Bv=Bv, dp=dp, groups=groups, wgrad_branch=wgrad_branch, merged_bwd=merged_bwd,
                      sgd_split=sgd_split, per_image=per_image, fwd_sc=fwd_sc, bwd_sc=bwd_sc,
                      sgd_points={13: (13, NL), 7: (7, 13)})
