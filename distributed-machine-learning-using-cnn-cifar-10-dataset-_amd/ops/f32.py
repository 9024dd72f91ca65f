"""fp32-accurate CNN path on hand-written HIP kernels (``--dtype fp32`` on the GPU).

The reference keeps every variable and op in ``tf.float32`` (/root/reference/cifar10cnn.py:97-145,
loss/SGD :150-164).  The fused engine trains in bf16 (fp32 accumulation and fp32 master weights);
this module is the reference-precision alternative on the same kind of native code: every
matrix product of the step -- conv forward, conv weight/data gradients, the three fc layers and
their gradients -- runs on ``torch.ops.dmlc.f32_gemm`` (fp32 MFMA ``v_mfma_f32_16x16x4_f32``, true
fp32 operands, deterministic split-K).  The two convolutions are implicit GEMMs
(``f32_conv_gemm``: the tile loader gathers the im2col matrix straight from the NHWC activation;
conv2 also has one direct kernel per role -- ``f32_conv2_direct`` for the forward and the data gradient,
``f32_conv2_wgrad`` for the weight + bias gradient -- chosen by ``conv_same(impl=)`` / ``CONV2_IMPL_F32``:
"direct" runs the first two on the direct kernel and keeps the weight gradient on the GEMM, "direct_all" runs
all three direct):
forward = im2col(x) W, weight + bias gradient = im2col(x)^T dY with a ones column (its output row
is the bias gradient), data gradient = im2col(dY) against the flipped, transposed weight -- no
column matrix is ever written.  conv1 has no data gradient (its input is the image), and its backward has a
direct kernel family too (csrc/kernels/f32_conv1.hip, ``CONV1_IMPL_F32`` / ``conv1_impl`` = "direct"): with
``fused`` the whole first stage is one autograd function whose backward is ONE call of ``f32_conv1_wgrad_pool`` --
the kernel rebuilds the gradient at the conv output from the pooled gradient and the argmax bytes in LDS
(``f32_relu_pool_bwd``'s result, bit for bit) and never writes it to memory --, without ``fused`` the weight
gradient of the [B,24,24,3] geometry runs on ``f32_conv1_wgrad``; "gemm" keeps the implicit GEMM.  Other geometries (e.g. another crop) use ``f32_im2col`` + GEMM with
the gather-form ``f32_col2im`` adjoint.  fc bias gradients: ``f32_colsum``.

The rest of the step is HIP as well (csrc/kernels/f32_pool.hip): ``relu_pool`` is the ReLU + TF-SAME 3x3/2
max-pool of a conv stage in one kernel each way -- the forward also writes a one-byte argmax per pooled
element (255 = masked by the ReLU), the only thing the backward keeps, and the backward writes the gradient
at the conv output in one gather pass (no zero-fill, no atomics) -- and ``xent_head`` is the softmax
cross-entropy, the batch's hit count and dlogits in one launch.  The forward is bit-identical to the PyTorch
ops; the backward differs by the order of at most four addends per element.  ``cnn_forward_f32(fused=False)``
keeps ``torch.relu`` + ``max_pool2d`` as the reference path.

The fully connected stack has a kernel family of its own (csrc/kernels/f32_fc.hip, ``FC_IMPL_F32`` / ``fc_impl`` =
"fused"): one autograd function ``_FcStack`` whose forward is fc1 on ``f32_gemm`` with the ReLU in its split-K
reduction plus ONE launch of ``f32_fc_tail_fwd`` (fc2 + ReLU + fc3), and whose backward is ``f32_fc_tail_bwd`` (both
ReLU-masked data gradients) and ``f32_fc_grads`` (the three weight gradients, their bias gradients as the last row
of each [in + 1, out] result, and the gradient at the stack's input) -- no PyTorch op and no column-sum launch in
between.  "gemm" keeps the chain of ``_Linear`` GEMMs with ``torch.relu`` between them.

Inference and evaluation have a kernel of their own: ``cnn_infer_f32`` runs the whole eval-mode forward,
uint8 pixels to fp32 logits, predictions and hit flags, in ONE launch of ``k_cnn_infer_f32``
(csrc/kernels/f32_infer.hip) -- the same fp32 MFMA, no PyTorch op in between.

Activations are NHWC and weights keep the TF layouts (HWIO / [in, out]), so the weights are
views of the model's flat parameter buffer and the im2col column order (kh, kw, ci) is the row
order of the HWIO weight viewed as [kh*kw*ci, co] -- no transposes anywhere.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _ext


def _ops():
    _ext.hip()          # loud failure when the native library is missing on a GPU box
    return torch.ops.dmlc


class _Linear(torch.autograd.Function):
    """y = x W + b (W stored [in, out])."""

    @staticmethod
    def forward(ctx, x, w, b):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        return _ops().f32_gemm(x, w, b.contiguous(), False, False, False)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        ops = _ops()
        gy = gy.contiguous()
        gx = ops.f32_gemm(gy, w, None, False, True, False) if ctx.needs_input_grad[0] else None   # dY W^T
        gw = ops.f32_gemm(x, gy, None, True, False, False)                                        # X^T dY
        return gx, gw, ops.f32_colsum(gy)


_IMPLICIT = {(24, 3), (12, 64)}          # (H, C) geometries of f32_conv_gemm (5x5, pad 2)


class _ConvImplicit(torch.autograd.Function):
    """Stride-1 TF-'SAME' 5x5 convolution as implicit GEMMs (no column matrix in memory)."""

    @staticmethod
    def forward(ctx, x, w, b, wgrad_direct=False):
        ops = _ops()
        B, H, W, C = x.shape
        co = w.shape[3]
        x = x.contiguous()
        wm = w.contiguous().view(25 * C, co)
        y = ops.f32_conv_gemm(x, wm, b.contiguous(), False, False)
        ctx.save_for_backward(x, w)
        ctx.wgrad_direct = wgrad_direct and (H, C, co) == (24, 3, 64)    # the geometry of k_f32_conv1_wgrad
        return y.view(B, H, W, co)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        ops = _ops()
        B, H, W, C = x.shape
        co = w.shape[3]
        gy = gy.contiguous()
        if ctx.wgrad_direct:
            gwb = ops.f32_conv1_wgrad(x, gy)                                     # [76, 64], the same layout
        else:
            gwb = ops.f32_conv_gemm(x, gy.view(B * H * W, co), None, True, True)   # [25*C + 1, co]
        gw, gb = gwb[:25 * C].view(5, 5, C, co), gwb[25 * C]
        gx = None
        if ctx.needs_input_grad[0] and (H, co) in _IMPLICIT:
            # dx = im2col(dY) . W'  with  W'[(kh, kw, co), ci] = W[4-kh, 4-kw, ci, co]
            wt = w.flip(0, 1).permute(0, 1, 3, 2).contiguous().view(25 * co, C)
            gx = ops.f32_conv_gemm(gy, wt, None, False, False).view(B, H, W, C)
        elif ctx.needs_input_grad[0]:          # dY geometry without an implicit kernel: explicit adjoint
            dcols = ops.f32_gemm(gy.view(B * H * W, co), w.contiguous().view(25 * C, co), None, False, True, False)
            gx = ops.f32_col2im(dcols, B, H, W, C, 5, 5, 2)
        return gx, gw, gb, None


# conv2's forward and data gradient on the fp32 step: "direct" (k_f32_conv2, csrc/kernels/f32_conv.hip) or
# "gemm" (the implicit GEMM of f32_gemm.hip with a flipped, transposed weight copy per backward); set by the
# same-session A/B of tools/f32_conv_ab.py: "direct" only if it wins at B = 256 by more than the larger spread
# of the two paths (profiles/f32_conv_ab.txt: 0.769 ms/step direct against 0.922 ms gemm, spreads 0.047 / 0.043).
# "direct_all" = "direct" with the weight + bias gradient on k_f32_conv2_wgrad too, under the same rule against
# "direct" (profiles/f32_wgrad_ab.txt, B = 256: 0.606 ms/step direct_all against 0.760 ms direct, spreads
# 0.064 / 0.054; B = 128: 0.478 against 0.556 ms, spreads 0.009 / 0.008)
CONV2_IMPL_F32 = "direct_all"
CONV2_IMPLS = ("direct_all", "direct", "gemm")


# conv1's backward on the fp32 step: "direct" (csrc/kernels/f32_conv1.hip: with fused the pool + ReLU backward and
# the weight gradient in one launch, without it the weight gradient alone) or "gemm" (f32_relu_pool_bwd + the
# implicit GEMM); under the rule above on tools/f32_conv_ab.py --stage conv1
# (profiles/f32_conv1_ab.txt, B = 256: 0.503 ms/step direct against 0.637 ms gemm, spreads 0.006 / 0.042; B = 128:
# 0.425 against 0.486 ms, spreads 0.008 / 0.038)
CONV1_IMPL_F32 = "direct"
CONV1_IMPLS = ("direct", "gemm")


def _conv1_impl(impl: Optional[str]) -> str:
    if impl not in (None,) + CONV1_IMPLS:
        raise ValueError(f"conv1_impl must be one of {CONV1_IMPLS} or None, got {impl!r}")
    return impl or CONV1_IMPL_F32


class _Conv1Stage(torch.autograd.Function):
    """The whole first stage pool(relu(conv1(x) + b)) of an image batch x [B,24,24,3] that needs no gradient.
    Forward: the kernels of the "gemm" path (f32_conv_gemm + f32_relu_pool_fwd, the same bits).  Saves x and the
    one-byte argmax only; the backward is one call of f32_conv1_wgrad_pool."""

    @staticmethod
    def forward(ctx, x, w, b):
        ops = _ops()
        x = x.contiguous()
        y = ops.f32_conv_gemm(x, w.contiguous().view(75, 64), b.contiguous(), False, False)
        p, arg = ops.f32_relu_pool_fwd(y.view(x.shape[0], 24, 24, 64), 0)
        ctx.save_for_backward(x, arg)
        return p

    @staticmethod
    def backward(ctx, gp):
        x, arg = ctx.saved_tensors
        gwb = _ops().f32_conv1_wgrad_pool(x, gp.contiguous(), arg)               # [76, 64]
        return None, gwb[:75].view(5, 5, 3, 64), gwb[75]


class _ConvDirect(torch.autograd.Function):
    """conv2 ([B,12,12,64] -> 64 channels, 5x5 TF-'SAME') on k_f32_conv2: the image in LDS, the weights
    streamed as MFMA fragments; the data gradient reads the same HWIO weight in place (no flipped or
    transposed copy).  The weight + bias gradient is the implicit GEMM im2col(x)^T dY ("direct") or, with
    ``wgrad_direct``, k_f32_conv2_wgrad ("direct_all"); both return the same [1601, 64] layout."""

    @staticmethod
    def forward(ctx, x, w, b, wgrad_direct=False):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        ctx.wgrad_direct = wgrad_direct
        return _ops().f32_conv2_direct(x, w, b.contiguous(), False)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        ops = _ops()
        gy = gy.contiguous()
        if ctx.wgrad_direct:
            gwb = ops.f32_conv2_wgrad(x, gy)                                     # [1601, 64]
        else:
            gwb = ops.f32_conv_gemm(x, gy.view(-1, 64), None, True, True)
        gx = ops.f32_conv2_direct(gy, w, None, True) if ctx.needs_input_grad[0] else None
        return gx, gwb[:1600].view(5, 5, 64, 64), gwb[1600], None


class _ConvSame(torch.autograd.Function):
    """Stride-1 TF-'SAME' KxK convolution, x NHWC [B,H,W,C], w HWIO [K,K,C,CO] -> NHWC (explicit
    im2col; geometries without an implicit kernel)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ops = _ops()
        B, H, W, C = x.shape
        k, co = w.shape[0], w.shape[3]
        cols = ops.f32_im2col(x.contiguous(), k, k, k // 2)                   # [B*H*W, K*K*C]
        wm = w.contiguous().view(k * k * C, co)
        y = ops.f32_gemm(cols, wm, b.contiguous(), False, False, False)
        ctx.save_for_backward(cols, wm)
        ctx.geom = (B, H, W, C, k)
        return y.view(B, H, W, co)

    @staticmethod
    def backward(ctx, gy):
        cols, wm = ctx.saved_tensors
        B, H, W, C, k = ctx.geom
        ops = _ops()
        g2 = gy.contiguous().view(B * H * W, wm.shape[1])
        gw = ops.f32_gemm(cols, g2, None, True, False, False).view(k, k, C, wm.shape[1])
        gb = ops.f32_colsum(g2)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = ops.f32_col2im(ops.f32_gemm(g2, wm, None, False, True, False), B, H, W, C, k, k, k // 2)
        return gx, gw, gb


def linear(x, w, b):
    return _Linear.apply(x, w, b)


# The fc stack of the fp32 step: "fused" (csrc/kernels/f32_fc.hip: fc1's forward on the GEMM with its ReLU epilogue,
# then one launch each for the forward tail, the backward tail and all gradients) or "gemm" (three _Linear GEMM
# chains, f32_colsum and the PyTorch ReLUs); under the rule at CONV2_IMPL_F32 on tools/f32_conv_ab.py --stage fc
# (profiles/f32_fc_ab.txt, B = 256: 0.411 ms/step fused against 0.498 ms gemm, spreads 0.008 / 0.007; B = 128: 0.350
# against 0.433 ms, spreads 0.072 / 0.012)
FC_IMPL_F32 = "fused"
FC_IMPLS = ("fused", "gemm")


def _fc_impl(impl: Optional[str]) -> str:
    if impl not in (None,) + FC_IMPLS:
        raise ValueError(f"fc_impl must be one of {FC_IMPLS} or None, got {impl!r}")
    return impl or FC_IMPL_F32


class _FcStack(torch.autograd.Function):
    """logits = relu(relu(x W1 + b1) W2 + b2) W3 + b3 for the model's 2304 -> 384 -> 192 -> 10 (weights [in, out]).
    Saves x, h1, h2; the backward is one call each of f32_fc_tail_bwd and f32_fc_grads."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3):
        ops = _ops()
        x, w1, w2, w3 = x.contiguous(), w1.contiguous(), w2.contiguous(), w3.contiguous()
        h1 = ops.f32_gemm(x, w1, b1.contiguous(), False, False, True)
        h2, logits = ops.f32_fc_tail_fwd(h1, w2, b2.contiguous(), w3, b3.contiguous())
        ctx.save_for_backward(x, h1, h2, w1, w2, w3)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        x, h1, h2, w1, w2, w3 = ctx.saved_tensors
        ops = _ops()
        dlogits = dlogits.contiguous()
        dh2, dh1 = ops.f32_fc_tail_bwd(dlogits, h1, h2, w2, w3)
        g1, g2, g3, dx = ops.f32_fc_grads(x, h1, h2, dh1, dh2, dlogits, w1, ctx.needs_input_grad[0])
        return dx, g1[:2304], g1[2304], g2[:384], g2[384], g3[:192], g3[192]


def fc_stack(x, p: Dict[str, torch.Tensor], impl: Optional[str] = None):
    """The three fc layers on x [B, 2304] -> the fc3 output [B, 10]; ``impl``: "fused" | "gemm" | None (``FC_IMPL_F32``)."""
    w = [p[f"full_{k}_{i}"] for i in (1, 2, 3) for k in ("weight", "bias")]
    if _fc_impl(impl) == "fused" and tuple(x.shape[1:]) == (2304,) \
            and [tuple(t.shape) for t in w] == [(2304, 384), (384,), (384, 192), (192,), (192, 10), (10,)]:
        return _FcStack.apply(x, *w)
    x = torch.relu(linear(x, w[0], w[1]))
    x = torch.relu(linear(x, w[2], w[3]))
    return linear(x, w[4], w[5])


def conv_same(x, w, b, implicit: bool = True, impl: Optional[str] = None, conv1_impl: Optional[str] = None):
    """``conv1_impl``: "direct" | "gemm" | None (``CONV1_IMPL_F32``) -- the weight-gradient kernel of the
    [B,24,24,3] -> 64 geometry (conv1) on the implicit path.  ``impl``: "direct_all" | "direct" | "gemm" | None (``CONV2_IMPL_F32``) -- the kernels of the
    [B,12,12,64] -> 64 geometry (conv2): all three roles direct, forward and data gradient direct with the
    weight gradient on the GEMM, or all GEMM; every other geometry takes the implicit / explicit GEMM path
    whatever ``impl`` says."""
    if impl not in (None,) + CONV2_IMPLS:
        raise ValueError(f"conv_same: impl must be one of {CONV2_IMPLS} or None, got {impl!r}")
    use = impl or CONV2_IMPL_F32
    if use != "gemm" and (implicit or impl) and tuple(x.shape[1:]) == (12, 12, 64) \
            and tuple(w.shape) == (5, 5, 64, 64):
        return _ConvDirect.apply(x, w, b, use == "direct_all")
    if implicit and w.shape[0] == 5 and w.shape[1] == 5 and (x.shape[1], x.shape[3]) in _IMPLICIT \
            and x.shape[1] == x.shape[2]:
        return _ConvImplicit.apply(x, w, b, _conv1_impl(conv1_impl) == "direct")
    return _ConvSame.apply(x, w, b)


def _pool_nhwc(x: torch.Tensor) -> torch.Tensor:
    """TF-SAME 3x3/2 max-pool of an NHWC tensor with no layout copies: for an even input, TF-SAME pads
    one -inf row/column at the bottom/right only, i.e. exactly ceil_mode windows starting at 2i; the
    NCHW view of NHWC memory is channels_last, so the pool runs in place of layout and its output
    permutes back to a contiguous NHWC tensor."""
    y = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
    return y if y.is_contiguous() else y.contiguous()


_FUSED_POOL = {24, 12}                   # H of the [B,H,H,64] conv outputs k_f32_relu_pool_* serve


class _ReluPool(torch.autograd.Function):
    """pool(relu(y)) of a conv output in one kernel each way (csrc/kernels/f32_pool.hip).  Saves the
    one-byte argmax only: the backward needs neither y nor relu(y)."""

    @staticmethod
    def forward(ctx, y, blocks):
        p, arg = _ops().f32_relu_pool_fwd(y.contiguous(), blocks)
        ctx.save_for_backward(arg)
        ctx.blocks = blocks
        return p

    @staticmethod
    def backward(ctx, gp):
        (arg,) = ctx.saved_tensors
        return _ops().f32_relu_pool_bwd(gp.contiguous(), arg, ctx.blocks), None


def relu_pool(y: torch.Tensor, blocks: int = 0) -> torch.Tensor:
    """TF-SAME 3x3/2 max-pool of relu(y), y fp32 NHWC [B,H,H,64] with H = 24 or 12; bit-identical to
    ``_pool_nhwc(torch.relu(y))``.  ``blocks``: workgroups of the kernels' grid-stride loops (0: default)."""
    return _ReluPool.apply(y, int(blocks))


class _XentHead(torch.autograd.Function):
    """(mean softmax cross-entropy, hit count) of the fc3 output in one launch of k_f32_xent_head, which
    also leaves d loss / d logits for the backward."""

    @staticmethod
    def forward(ctx, logits, labels, relu_logits):
        loss, hits, dlogits = _ops().f32_xent_head(logits.contiguous(), labels.contiguous(), relu_logits)
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(hits)
        return loss, hits

    @staticmethod
    def backward(ctx, gloss, _ghits):
        (dlogits,) = ctx.saved_tensors
        return dlogits * gloss, None, None


def xent_head(logits: torch.Tensor, labels: torch.Tensor, relu_logits: bool):
    """``logits``: the fc3 output fp32 [B,10] BEFORE the optional logit ReLU; ``labels``: int32 or int64 [B]
    in [0, 10).  Returns (loss fp32 [] = mean cross-entropy of relu(logits) if ``relu_logits`` else of
    logits, hits int32 [] = rows whose first maximum is the label)."""
    return _XentHead.apply(logits, labels, bool(relu_logits))


class _FlatViews(torch.autograd.Function):
    """The per-variable tensors of a flat parameter buffer whose backward builds the flat gradient
    in ONE concatenation (autograd through plain views of a leaf would zero-fill a full-size
    gradient and add into it once per variable: 10 fills + 10 adds of 4.3 MB per step)."""

    @staticmethod
    def forward(ctx, flat, specs):
        ctx.specs, ctx.n = specs, flat.numel()
        return tuple(flat[s.offset:s.offset + s.numel].view(s.shape) for s in specs)

    @staticmethod
    def backward(ctx, *grads):
        parts, pos = [], 0
        ref = next((g for g in grads if g is not None), None)
        if ref is None:
            return None, None
        for s, g in zip(ctx.specs, grads):
            if s.offset > pos:
                parts.append(ref.new_zeros(s.offset - pos))
            parts.append(g.reshape(-1) if g is not None else ref.new_zeros(s.numel))
            pos = s.offset + s.numel
        if ctx.n > pos:
            parts.append(ref.new_zeros(ctx.n - pos))
        return torch.cat(parts), None


def flat_views(flat: torch.Tensor, specs) -> Dict[str, torch.Tensor]:
    from ..models.cifar_cnn import short
    return {short(s.name): v for s, v in zip(specs, _FlatViews.apply(flat, tuple(specs)))}


_INFER_SCRATCH: Dict[tuple, torch.Tensor] = {}   # (device, workgroups) -> fp32 [workgroups, 16, 2304]


@torch.no_grad()
def cnn_infer_f32(images_u8: torch.Tensor, flat: torch.Tensor, labels: Optional[torch.Tensor] = None,
                  idx: Optional[torch.Tensor] = None, blocks: Optional[int] = None, relu_logits: bool = True,
                  crop_offset=(4, 4)):
    """Eval-mode forward of uint8 [N,32,32,3] images (on any device) in ONE launch of k_cnn_infer_f32
    (csrc/kernels/f32_infer.hip), every product on the fp32 MFMA: (logits fp32 [n,10], pred int32 [n],
    hits int32 [n] or None without ``labels``).  ``flat``: the model's flat fp32 parameter buffer on the
    GPU (models/cifar_cnn.py PARAM_SPECS), read in place; ``idx``: rows of ``images_u8`` to run
    (n = len(idx)), else all of them; ``labels``: one per row of ``images_u8``; ``blocks``: workgroups
    of the persistent loop (None: one per CU); ``crop_offset``: top-left corner of the 24x24 crop."""
    from ..models.cifar_cnn import PARAM_SPECS
    ops = _ops()
    dev = flat.device
    if images_u8.dtype != torch.uint8 or tuple(images_u8.shape[1:]) != (32, 32, 3):
        raise ValueError(f"cnn_infer_f32: images must be uint8 [N,32,32,3], got {images_u8.dtype} {tuple(images_u8.shape)}")
    images_u8 = images_u8.to(dev).contiguous()
    if idx is not None:
        idx = idx.to(dev, torch.int32).reshape(-1).contiguous()
    n = images_u8.shape[0] if idx is None else idx.numel()
    if labels is not None:
        labels = labels.to(dev, torch.int32).reshape(-1).contiguous()
    logits = torch.empty(n, 10, dtype=torch.float32, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    hits = None if labels is None else torch.empty(n, dtype=torch.int32, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    grid = max(1, min(-(-n // 16), int(blocks) if blocks else max(1, cus)))
    key = (dev, grid)
    if key not in _INFER_SCRATCH:        # one [16][2304] slab of pooled activations per workgroup
        _INFER_SCRATCH[key] = torch.empty(grid, 16, 2304, dtype=torch.float32, device=dev)
    ops.f32_cnn_infer(images_u8, idx, labels, int(crop_offset[0]), int(crop_offset[1]), flat.detach(),
                      [s.offset for s in PARAM_SPECS], bool(relu_logits), _INFER_SCRATCH[key], logits, pred, hits,
                      int(blocks or 0))
    return logits, pred, hits


def _conv_stage(x, w, b, fused: bool, impl: Optional[str] = None, conv1_impl: Optional[str] = None):
    if fused and _conv1_impl(conv1_impl) == "direct" and not x.requires_grad \
            and tuple(x.shape[1:]) == (24, 24, 3) and tuple(w.shape) == (5, 5, 3, 64):
        return _Conv1Stage.apply(x, w, b)
    y = conv_same(x, w, b, impl=impl, conv1_impl=conv1_impl)
    if fused and y.shape[1] == y.shape[2] and y.shape[1] in _FUSED_POOL and y.shape[3] == 64:
        return relu_pool(y)
    return _pool_nhwc(torch.relu(y))


def cnn_forward_f32(images_nhwc: torch.Tensor, p: Dict[str, torch.Tensor], relu_logits: bool = True,
                    fused: bool = True, conv2_impl: Optional[str] = None,
                    conv1_impl: Optional[str] = None, fc_impl: Optional[str] = None) -> torch.Tensor:
    """The reference CNN (models/cifar_cnn.py:cnn_forward semantics) on the fp32 HIP kernels.  ``fused``:
    ReLU + pool of the conv stages through ``relu_pool`` where the geometry is one of its two ([B,24,24,64],
    [B,12,12,64]); otherwise, and with ``fused=False``, the PyTorch ops (same logits bit for bit).
    ``conv2_impl``: the second stage's conv kernel, ``conv_same``'s ``impl`` (independent of ``fused``); ``conv1_impl``: the
    first stage's backward, "direct" | "gemm" | None (``CONV1_IMPL_F32``); ``fc_impl``: the fc stack, "fused" | "gemm" |
    None (``FC_IMPL_F32``)."""
    _fc_impl(fc_impl)
    x = images_nhwc.float().contiguous()
    x = _conv_stage(x, p["conv1_kernel"], p["conv1_bias"], fused, conv1_impl=conv1_impl)
    x = _conv_stage(x, p["conv2_kernel"], p["conv2_bias"], fused, conv2_impl)
    x = x.reshape(x.shape[0], -1)                               # NHWC flatten (cifar10cnn.py:126)
    x = fc_stack(x, p, fc_impl)
    return torch.relu(x) if relu_logits else x
