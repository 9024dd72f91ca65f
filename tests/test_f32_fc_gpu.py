"""The fc stack of the fp32 step on its own kernels (csrc/kernels/f32_fc.hip, ops/f32.py fc_impl="fused") against
float64 on the CPU: each kernel exact on integers, the autograd function end to end, floats at the fp32 bound and
against the GEMM chain's own error, bitwise properties, the whole model, a captured step, the argument checks."""
import pytest
import torch
import torch.nn.functional as F

from dmlc.models import cifar_cnn as M
from dmlc.ops import f32

pytestmark = pytest.mark.gpu
BS = [1, 16, 17, 70]     # a nearly empty row tile and K = 1; one tile; a second tile and K % 4 != 0; a 64-row dx tile + tail
SHAPES = {"x": 2304, "h1": 384, "h2": 192, "dh1": 384, "dh2": 192, "dl": 10}
WSHAPES = {"w1": (2304, 384), "b1": (384,), "w2": (384, 192), "b2": (192,), "w3": (192, 10), "b3": (10,)}


def _ops():
    import dmlc.ops._ext as E
    E.hip()
    return torch.ops.dmlc


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30))


def _inputs(B, ints, clamp=True):
    """Independent operands of all three kernels: integers (activations in [-3,3], gradients and weights in [-2,2]) or
    randn (weights scaled by 1 / sqrt(fan-in)); with clamp h1, h2 >= 0, about half their entries exactly 0."""
    g = torch.Generator().manual_seed(100 + B)
    rnd = lambda lim, *s: torch.randint(-lim, lim + 1, s, generator=g).float() if ints else torch.randn(*s, generator=g)
    t = {n: rnd(3 if n in ("x", "h1", "h2") else 2, B, c) for n, c in SHAPES.items()}
    t.update({n: rnd(2, *s) * (1.0 if ints else s[0] ** -0.5) for n, s in WSHAPES.items()})
    if clamp:
        t["h1"], t["h2"] = t["h1"].clamp_min(0), t["h2"].clamp_min(0)
    return {n: v.cuda() for n, v in t.items()}, {n: v.double() for n, v in t.items()}


def _ref(d):
    """float64: the three kernels' outputs from the same independent operands, in the kernels' output order."""
    h2 = torch.relu(d["h1"] @ d["w2"] + d["b2"])
    dh2 = (d["dl"] @ d["w3"].t()) * (d["h2"] > 0)
    rows = lambda a, g: torch.cat([a.t() @ g, g.sum(0)[None]])
    return {"fwd": (h2, h2 @ d["w3"] + d["b3"]), "bwd": (dh2, (dh2 @ d["w2"].t()) * (d["h1"] > 0)),
            "grads": (rows(d["x"], d["dh1"]), rows(d["h1"], d["dh2"]), rows(d["h2"], d["dl"]), d["dh1"] @ d["w1"].t())}


def _run(c, kernel, need_dx=True):
    ops = _ops()
    if kernel == "fwd":
        return ops.f32_fc_tail_fwd(c["h1"], c["w2"], c["b2"], c["w3"], c["b3"])
    if kernel == "bwd":
        return ops.f32_fc_tail_bwd(c["dl"], c["h1"], c["h2"], c["w2"], c["w3"])
    return ops.f32_fc_grads(c["x"], c["h1"], c["h2"], c["dh1"], c["dh2"], c["dl"], c["w1"], need_dx)


@pytest.mark.parametrize("kernel", ["fwd", "bwd", "grads"])
@pytest.mark.parametrize("B", BS)
def test_fc_kernels_are_exact_on_integers(B, kernel):
    """|h2 pre-activation| <= 2306, |logits| <= 885,506, |dh2| <= 40, |dh1| <= 15,360, |dW| <= 6 B, |dx| <= 1536: all
    below 2^24, so every partial sum in any order is exact."""
    c, d = _inputs(B, True, clamp=kernel != "grads")     # grads: h in [-3,3] like x
    assert kernel == "grads" or min(float((c[n] == 0).float().mean()) for n in ("h1", "h2")) > 0.3
    got, ref = _run(c, kernel), _ref(d)[kernel]
    assert all(torch.equal(a.cpu().double(), e) for a, e in zip(got, ref))
    if kernel == "grads":
        no_dx = _run(c, kernel, need_dx=False)
        assert no_dx[3] is None and all(torch.equal(a, e) for a, e in zip(no_dx[:3], got[:3]))


def _stack(impl, x, w, G):
    """logits and the seven gradients of sum(logits * G) through fc_stack(impl) (float64 tensors: the plain formulas)."""
    x, w = x.clone().requires_grad_(), {n: v.clone().requires_grad_() for n, v in w.items()}
    if impl is None:
        logits = torch.relu(torch.relu(x @ w["w1"] + w["b1"]) @ w["w2"] + w["b2"]) @ w["w3"] + w["b3"]
    else:
        names = {f"full_{'weight' if n[0] == 'w' else 'bias'}_{n[1]}": v for n, v in w.items()}
        logits = f32.fc_stack(x, names, impl)
    (logits * G).sum().backward()
    return [logits.detach(), x.grad] + [v.grad for v in w.values()]


@pytest.mark.parametrize("B", BS)
def test_fc_stack_is_exact_on_integers_and_equals_the_gemm_chain(B):
    """W1 is 0 but for one +-1 per column, so h1 = relu(+-x[k] + b1) <= 3 and the bounds above hold through the chain."""
    c, d = _inputs(B, True)
    g = torch.Generator().manual_seed(B)
    w1 = torch.zeros(2304, 384)
    w1[torch.randint(0, 2304, (384,), generator=g), torch.arange(384)] = torch.randint(0, 2, (384,), generator=g).float() * 2 - 1
    w = {n: (w1 if n == "w1" else d[n].float() if n != "b1" else torch.zeros(384)) for n in WSHAPES}
    G = torch.randint(-2, 3, (B, 10), generator=g).float()
    ref = _stack(None, d["x"], {n: v.double() for n, v in w.items()}, G.double())
    cw = {n: v.cuda() for n, v in w.items()}
    fused, gemm = _stack("fused", c["x"], cw, G.cuda()), _stack("gemm", c["x"], cw, G.cuda())
    assert all(torch.equal(a.cpu().double(), e) for a, e in zip(fused, ref))
    assert all(torch.equal(a, e) for a, e in zip(fused, gemm))


def test_fc_kernels_match_fp64_on_floats():
    """Measured on an MI355X at B = 17, relative to float64: gw1b 7.6e-8, gw2b 5.7e-8, gw3b 5.7e-8, dx 3.5e-7; fused against
    the GEMM chain: h2 1.7e-7 / 2.3e-7, logits 2.4e-7 / 2.9e-7, dh2 5.9e-8 / 5.9e-8, dh1 1.8e-7 / 1.9e-7."""
    ops, (c, d) = _ops(), _inputs(17, False)
    ref = _ref(d)
    for a, e, n in zip(_run(c, "grads"), ref["grads"], ("gw1b", "gw2b", "gw3b", "dx")):
        print(f"f32_fc_grads {n}: rel {_rel(a, e):.3g}")
        assert _rel(a, e) < 2e-6         # one fp32-MFMA sum: the bound of tests/test_f32_wgrad_gpu.py
    mm = lambda a, b, bias=None, tb=False: ops.f32_gemm(a, b, bias, False, tb, False)
    h2 = torch.relu(mm(c["h1"], c["w2"], c["b2"]))          # the "gemm" chain on the same inputs
    dh2 = mm(c["dl"], c["w3"], None, True) * (c["h2"] > 0)
    gemm = (h2, mm(h2, c["w3"], c["b3"]), dh2, mm(dh2, c["w2"], None, True) * (c["h1"] > 0))
    for a, y, e, n in zip(_run(c, "fwd") + _run(c, "bwd"), gemm, ref["fwd"] + ref["bwd"], ("h2", "logits", "dh2", "dh1")):
        print(f"fc tail {n}: fused rel {_rel(a, e):.3g}, gemm rel {_rel(y, e):.3g}")
        assert _rel(a, e) <= 2 * _rel(y, e)   # only the order of at most 384 addends differs


def test_fc_tail_is_reproducible_and_row_independent():
    c, _ = _inputs(17, False)
    full = _run(c, "fwd") + _run(c, "bwd")
    assert all(torch.equal(a, e) for a, e in zip(full, _run(c, "fwd") + _run(c, "bwd")))
    for row in (0, 5, 15, 16):          # any position in a tile, and the second tile's only row
        one = {n: (v[row:row + 1].contiguous() if n in SHAPES else v) for n, v in c.items()}
        assert all(torch.equal(a[row:row + 1], e) for a, e in zip(full, _run(one, "fwd") + _run(one, "bwd")))


@pytest.mark.parametrize("B", [1, 8])
def test_model_with_fused_fc_matches_fp64(B):
    """Measured on an MI355X: loss 7.6e-7 / 4.1e-8, flat gradient 6.0e-7 / 1.3e-6 relative at B = 1 / 8."""
    flat = M.init_flat_params(torch.Generator().manual_seed(B))
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 256, (B, 24, 24, 3), generator=g).float().cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    ref = M.CifarCNN(flat.double(), relu_logits=False)
    ref.flat.data = ref.flat.data.double()
    l64 = F.cross_entropy(ref(x.cpu().double()), y.cpu())
    l64.backward()
    hip = M.CifarCNN(flat, relu_logits=False, backend="hip_f32", fc_impl="fused").cuda()
    loss = F.cross_entropy(hip(x), y)
    loss.backward()
    errs = {"loss": _rel(loss.detach(), l64.detach()), "flat gradient": _rel(hip.flat.grad, ref.flat.grad)}
    print(f"fused fc model vs fp64, B={B}: {errs}")
    assert max(errs.values()) < 1e-4, errs      # the bound of tests/test_f32_gpu.py


def test_captured_fused_fc_step_equals_the_eager_step_and_tracks_the_gemm_chain():
    from dmlc.engine.eager import EagerTrainer
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (128, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (128,), dtype=torch.int32, generator=g)
    kw = dict(device="cuda", dtype="fp32", seed=3, lr=1e-4, graph=True, backend="hip_f32")
    tr, ref = (EagerTrainer("cifar_cnn", 16, data, labels, fc_impl=i, **kw) for i in ("fused", "gemm"))
    for _ in range(3):                                  # warm-up steps; the third one captures
        tr.step(), ref.step()
    assert tr.graph is not None and tr.model.fc_impl == "fused"
    for _ in range(3):                                  # replay, then the same step eagerly from the same weights
        before = tr.model.flat.detach().clone()
        tr.step(), ref.step()
        got = [tr.last_loss.clone(), tr.last_acc.clone(), tr.model.flat.detach().clone()]
        with torch.no_grad():
            tr.model.flat.copy_(before)
        tr.model.flat.grad = None
        loss, acc = tr._fwd_bwd_sgd(tr._xs, tr._ys, tr._lr_t)
        assert all(torch.equal(a, e) for a, e in zip(got, [loss, acc, tr.model.flat.detach()]))
        assert _rel(tr.model.flat.detach(), ref.model.flat.detach()) < 1e-6    # trainer against trainer: tests/test_f32_gpu.py


@pytest.mark.parametrize("case", ["dtype", "inner", "strided", "cpu"])
@pytest.mark.parametrize("kernel", ["fwd", "bwd", "grads"])
def test_fc_ops_reject_bad_arguments(kernel, case):
    c, _ = _inputs(2, True)
    n = "h1" if kernel != "grads" else "dh1"
    c[n] = {"dtype": c[n].double(), "inner": torch.zeros(2, 383).cuda(), "strided": torch.zeros(2, 768).cuda()[:, ::2],
            "cpu": c[n].cpu()}[case]
    with pytest.raises(RuntimeError):
        _run(c, kernel)


def test_unknown_fc_impl_is_a_value_error():
    with pytest.raises(ValueError):
        M.CifarCNN(backend="hip_f32", fc_impl="nope")
    with pytest.raises(ValueError):
        f32.cnn_forward_f32(torch.zeros(1, 24, 24, 3), {}, fc_impl="nope")
