"""k_cnn_infer's fp8 variant (csrc/kernels/cnn_infer.hip) through an fp8 FusedCifarEngine, as tests/test_cnn_infer_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from dmlc.engine.fused import SEG_OFF, FusedCifarEngine
from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu
BF16, E4M3 = torch.bfloat16, torch.float8_e4m3fn


def _ref(images, flat, relu_logits, w8=None, sw=None):
    """models/cifar_cnn.py in fp64 on the CPU, centre crop.  With ``w8`` / ``sw`` (the engine's e4m3 conv2 bytes, their
    scale), rounded where the kernel rounds: bf16 conv1 / fc weights, p1, p2, h1, h2; conv2 on w8 / sw and p1 * sx -> e4m3."""
    rb = (lambda t: t.to(BF16).double()) if w8 is not None else (lambda t: t.double())
    p = M.views(flat.float().cpu())
    x = images.cpu()[:, 4:28, 4:28, :].double().permute(0, 3, 1, 2)
    x = F.conv2d(x, rb(p["conv1_kernel"]).permute(3, 2, 0, 1), p["conv1_bias"].double(), padding=2)
    x = rb(M.tf_same_maxpool_3x3s2(F.relu(x)))
    w2 = p["conv2_kernel"].double().permute(3, 2, 0, 1)
    if w8 is not None:
        mant, ex = torch.frexp(x.flatten(1).amax(1))                  # amax = mant * 2^ex, 448 = 0.875 * 2^9
        k = torch.where(mant > 0, (9 - ex - (mant > 0.875).int()).clamp(-126, 126), 0)
        sx = torch.exp2(k.double()).view(-1, 1, 1, 1)
        x = (x * sx).float().to(E4M3).double() / sx
        w2 = (w8.cpu().view(E4M3).float().double() / sw).view(64, 5, 5, 64).permute(0, 3, 1, 2)
    x = rb(M.tf_same_maxpool_3x3s2(F.relu(F.conv2d(x, w2, p["conv2_bias"].double(), padding=2))))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    x = rb(F.relu(x @ rb(p["full_weight_1"]) + p["full_bias_1"].double()))
    x = rb(F.relu(x @ rb(p["full_weight_2"]) + p["full_bias_2"].double()))
    x = x @ rb(p["full_weight_3"]) + p["full_bias_3"].double()
    return F.relu(x) if relu_logits else x


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def _case(relu_logits, steps, seed=0, lr=1e-5, extremes=True):
    """(engine, its 64 images, labels, fp64 logits without and with the kernel's roundings)"""
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (64, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (64,), dtype=torch.int32, generator=g)
    if extremes:                           # a zero amax, and a dark image beside a bright one
        data[20], data[21] = 0, 255
    eng = FusedCifarEngine(64, data, labels, device="cuda", seed=seed, lr=lr, relu_logits=relu_logits, dtype="fp8")
    if steps:                              # w2f8 / scale_w as the SGD kernel leaves them, fc1n parity slot 1
        eng.capture(steps_per_graph=1)
        eng.run(steps)
    flat, sw, one = eng.flat_params(), float(eng.scale_w[steps & 1]), eng.infer_logits(data[:1])
    assert eng.global_step() == steps and torch.isfinite(flat).all() and sw > 0 and torch.isfinite(one).all()
    return eng, data, labels, _ref(data, flat, relu_logits), _ref(data, flat, relu_logits, eng.w2f8[0], sw)


@pytest.fixture(scope="module", params=[(True, 0), (False, 3)], ids=["relu-fresh", "linear-trained"])
def case(request):
    return _case(*request.param)


@pytest.mark.parametrize("n,blocks", [(1, None), (16, None), (17, None), (37, 2), (5, 8)])
def test_logits_against_fp64(case, n, blocks):
    """rel(kernel, fp64) <= 3 * e_model; rel(kernel, rounded fp64) <= e_model = rel(rounded fp64, fp64): only fp32 sums and
    the rare tie they flip lie between (a wrong tap, scale or slice is O(1)).  Measured on an MI355X, the three figures
    in turn: fresh 2.4e-2..3.0e-2, 2.5e-4..1.5e-3, 2.4e-2..3.0e-2; trained 4.3e-2..5.1e-2, 1.0e-7..2.6e-3, 4.3e-2..5.1e-2."""
    eng, data, labels, ref, ref_q = case
    got, pred, correct = eng.infer(data[:n], labels[:n], blocks=blocks)
    e_model, err, err_q = _rel(ref_q[:n], ref[:n]), _rel(got, ref[:n]), _rel(got, ref_q[:n])
    print(f"cnn_infer fp8 n={n} blocks={blocks}: rel to fp64 {err:.3e}, to rounded fp64 {err_q:.3e}, e_model {e_model:.3e}")
    assert got.shape == (n, 10) and got.dtype == torch.float32 and err <= 3 * e_model and err_q <= e_model
    assert torch.equal(pred.long(), got.argmax(1)) and torch.equal(correct, (pred == labels[:n].cuda()).int())
    assert torch.isfinite(got[20:21]).all()            # the all-zero image


def test_image_independence_bitwise(case):
    """An image's logits depend on nothing but the image (rows 20, 21: the zero image beside the all-255 one)."""
    eng, data, labels, _, _ = case
    full, pred, _ = eng.infer(data[:37], labels[:37])
    for blocks in (1, 2, 3):
        assert torch.equal(eng.infer_logits(data[:37], blocks=blocks), full), blocks
    for i, j in ((0, 1), (15, 16), (16, 17), (36, 37), (5, 30)):      # single images, a slice
        assert torch.equal(eng.infer_logits(data[i:j]), full[i:j]), i
    perm = torch.cat([torch.randperm(37, generator=torch.Generator().manual_seed(3)), torch.tensor([4, 4, 36, 0])])
    lg, pr, co = eng.infer(data[:37], labels[:37], idx=perm, blocks=2)
    assert torch.equal(lg, full[perm.cuda()]) and torch.equal(pr, pred[perm.cuda()])
    assert torch.equal(co, (pr == labels[perm].cuda()).int())


def test_evaluate_leaves_training_alone():
    # (plain random images: the zero image's logits are its biases, no seed lifts their top-2 gap over the bound.  The
    # bound is 3 x the e4m3 roundings' 2e-2 x the norm of all 640 logits: of 2000 seeds tried in fp64 this one clears it)
    eng, data, labels, ref, ref_q = _case(False, 3, seed=938, lr=1e-6, extremes=False)
    e_model, top2 = _rel(ref_q, ref), ref.topk(2, dim=1).values
    gap, bound = float((top2[:, 0] - top2[:, 1]).min()), 3 * e_model * float(ref.norm())
    print(f"evaluate fp8: smallest fp64 top-2 gap {gap:.3f}, bound {bound:.3f}, e_model {e_model:.3e}")
    assert gap > bound, "pick another seed"
    names = ("master", "fc1n", "w1f", "w2f8", "scale_w", "amax_w", "fc2t", "fc3t", "bidx", "xraw", "stats", "step_t")
    before = [getattr(eng, k).clone() for k in names]
    acc = eng.evaluate(data, labels, impl="hip")
    for k, b in zip(names, before):
        assert torch.equal(getattr(eng, k).view(torch.uint8), b.view(torch.uint8)), k
    assert acc == int(eng.infer(data, labels)[2].sum()) / 64 == int((ref_q.argmax(1) == labels.long()).sum()) / 64
    eng.run(1)                             # and training goes on
    assert eng.global_step() == 4 and torch.isfinite(eng.master).all()


@pytest.mark.parametrize("bad", ["w2f8_dtype", "w2f8_shape", "scale_w_missing"])
def test_binding_rejects_bad_arguments(case, bad):
    """Each bad fp8 argument raises in the binding, before any launch (the outputs stay as they were)."""
    (eng, data, labels), dev, n = case[:3], "cuda", 40
    logits, correct = torch.full((n, 10), -7.0, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
    w8 = {"w2f8_dtype": eng.w2f8[0].to(torch.int8), "w2f8_shape": eng.w2f8[0][:, :1536].contiguous()}.get(bad, eng.w2f8[0])
    with pytest.raises(RuntimeError):
        eng.ops.cnn_infer(data[:n].to(dev), None, labels[:n].to(dev), 4, 4, eng.w1f, eng.w2f, eng.fc1n, eng.step_t,
                          eng.fc2t, eng.fc3t, eng.master, SEG_OFF, True, torch.empty(3, 16, 2304, dtype=BF16, device=dev),
                          logits, None, correct, 0, w8, None if bad == "scale_w_missing" else eng.scale_w)
    assert bool((logits == -7.0).all()) and bool((correct == -7).all())
