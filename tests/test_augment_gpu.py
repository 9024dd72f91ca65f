"""Per-image random crop + flip inside the fused CIFAR step, on the GPU.

Exact part: the integer cases of tests/aug_ref.py -- the oracle of tests/exact_ref.py run on the host
reference's augmented images -- through every forward launch and both weight-gradient paths, bit for
bit (torch.equal, mismatches named by image, row, column, channel).  Engine part: the three finalizers
write the next step's table, graph replays equal eager steps, resume, the data-parallel step, the fp8
step, and training against the eager fp32 engine, which draws the same words through the host twin."""
import json
import math
import os
import sys

import pytest
import torch

import aug_ref as A
import test_cnn_exact_gpu as E
from dmlc.data import synthetic
from dmlc.data.order import OrderSpec, apply_augment
from dmlc.engine.fused import FusedCifarEngine
from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(case, words=None, Bv=None, **kw):
    eng = E._engine(case, Bv=Bv, augment=True, **kw)
    assert eng.aug is not None and eng.buf["aug"] is eng.aug
    words = case.words if words is None else words
    eng.aug.copy_(words)
    return eng


def _check_forward(t, eng, case, rows, words, what):
    rows = rows.cpu().long()
    ref = A.rows_case(case, rows, words)
    t.equal(f"p1[{what}]", eng.p1, ref.p1)
    t.equal(f"am1[{what}]", eng.am1, ref.am1)
    t.equal(f"p2[{what}]", eng.p2, ref.p2)
    t.equal(f"am2[{what}]", eng.am2, ref.am2)
    # xraw holds the RAW rows, with or without augmentation (api.h)
    assert torch.equal(eng.xraw.cpu(), case.data[rows].view(-1, 3072)), f"{t.tag} xraw[{what}]"
    return ref


@pytest.mark.parametrize("name", list(E.FWD))
def test_forward_is_bit_exact(name):
    """B = 16, the 16-word table (corners, centre, mixed offsets; flipped and not): every forward launch,
    through the engine's own batch rows and through an explicit list in another order -- the table is by
    batch row, so the list pairs other images with the same words."""
    case = A.make_aug_case(16, 1)
    kw, selected = E.FWD[name]
    eng = _engine(case, **kw)
    assert selected(eng), f"{name}: the engine chose another forward path"
    t = E._Tally(f"aug_fwd_{name}")
    E._forward(eng, eng.bidx)
    _check_forward(t, eng, case, eng.bidx, case.words, "bidx")
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    assert not torch.equal(perm, eng.bidx.cpu())
    E._forward(eng, eng._padded(perm))
    _check_forward(t, eng, case, perm, case.words, "list")
    t.write()


@pytest.mark.parametrize("split", [1, 2])
def test_forward_padded_batch_repeats_last_row(split):
    """Bv = 12 in a kernel batch of 16: the padding rows carry row 11's image and word."""
    case = A.make_aug_case(16, 1)
    words = torch.cat([case.words[:12], case.words[11:12].expand(4)])
    eng = _engine(case, words, Bv=12, conv_split=split, conv1_split=2)
    assert (eng.Bv, eng.B) == (12, 16)
    # the engine's own table pads the same way
    assert torch.equal(eng.order.augment(0, pad_to=16)[12:], eng.order.augment(0)[11:].expand(4))
    t = E._Tally(f"aug_fwd_bv12_split{split}")
    for what, idx in (("bidx", eng.bidx), ("list", eng._padded(torch.tensor([9, 3, 15, 0, 7, 1, 12, 5, 2, 14, 6, 10],
                                                                           dtype=torch.int32)))):
        rows = idx.cpu().long()
        assert bool((rows[12:] == rows[11]).all())
        E._forward(eng, idx)
        _check_forward(t, eng, case, rows, words, what)
        for buf in (eng.p1, eng.am1, eng.p2, eng.am2):
            assert torch.equal(buf[12:], buf[11:12].expand_as(buf[12:]))
    t.write()


def _backward(t, case, reduce, **kw):
    """tests/test_cnn_exact_gpu.py _backward with the word table: an explicit list, an integer dp2,
    conv2 dgrad + both weight gradients + the slab reduction against the oracle."""
    eng = _engine(case, variant=None if reduce else {"wgrad_sgd": False}, **kw)
    assert eng._grad_in_launch == reduce
    eng.keep_dp1 = True
    perm = torch.randperm(case.B, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    ids = eng._padded(perm)
    E._forward(eng, ids)
    ref = _check_forward(t, eng, case, perm, case.words, "list")
    eng.dp2.copy_(ref.dp2.to(BF16))
    for buf in (eng.dy2, eng.dp1, eng.grad):
        buf.fill_(float("nan"))
    if reduce:
        eng._conv_backward(src=(ids, None, 1), reduce=True)
    else:
        eng._conv_backward(src=(ids, None, 1))
        eng._sgd(mode=1)
    torch.cuda.synchronize()
    eng.check_barriers()
    t.equal("dy2", eng.dy2, ref.dy2)
    t.equal("dp1", eng.dp1, ref.dp1)
    g = M.views(eng.grad)
    t.equal("conv2_kernel grad", g["conv2_kernel"], ref.gw2, E.HWIO)
    t.equal("conv2_bias grad", g["conv2_bias"], ref.gb2, ("co",))
    t.equal("conv1_kernel grad", g["conv1_kernel"], ref.gw1, E.HWIO)
    t.equal("conv1_bias grad", g["conv1_bias"], ref.gb1, ("co",))
    assert torch.equal(eng.aug.cpu(), case.words), "a reduce-only launch rewrote the table"
    return eng


@pytest.mark.parametrize("dsplit", [1, 2])
@pytest.mark.parametrize("reduce", [False, True], ids=["wgrad+sgd", "wgrad_sgd"])
def test_conv_backward_is_bit_exact(reduce, dsplit):
    case = A.make_aug_case(16, 2)
    t = E._Tally(f"aug_bwd_{'reduce' if reduce else 'launches'}_d{dsplit}")
    eng = _backward(t, case, reduce, dgrad_split=dsplit)
    assert eng.dgrad_split == dsplit
    t.write()


def test_conv_backward_is_bit_exact_on_the_ragged_256_block_map():
    """B = 144, the words of seed 11 / step 3, through the in-launch reduction: 16 of the 128 conv1
    roles take two images, each with its own word."""
    case = A.make_aug_case(144, 4)
    t = E._Tally("aug_bwd_reduce_b144")
    eng = _backward(t, case, True)
    assert (eng.B, eng.g1, eng.g2) == (144, 128, 32)
    t.write()


def _random_u8(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 32, 32, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), generator=g, dtype=torch.int32))


@pytest.mark.parametrize("B", [16, 144])
def test_centre_words_equal_the_unaugmented_engine(B):
    """A table of word 68 (centre crop, no flip) on random uint8 images: outputs and the flat gradient
    equal the engine without augmentation, bit for bit."""
    data, labels = _random_u8(2 * B, seed=31)
    kw = dict(seed=32, lr=1e-4, relu_logits=False)
    on = FusedCifarEngine(B, data, labels, **kw, augment=True)
    off = FusedCifarEngine(B, data, labels, **kw)
    assert off.aug is None and "aug" not in off.buf
    assert not bool((on.aug == A.CENTRE).all())
    on.aug.fill_(A.CENTRE)
    grads = [eng.compute_gradients().clone() for eng in (on, off)]
    torch.cuda.synchronize()
    for k in ("p1", "am1", "p2", "am2", "xraw"):
        assert torch.equal(getattr(on, k), getattr(off, k)), k
    assert torch.isfinite(grads[1]).all() and torch.equal(grads[0], grads[1])


def _state(eng):
    return eng.global_step(), eng.master.clone(), eng.stats[:8].clone()


def test_one_launch_backward_and_prefetch_are_bit_identical():
    """B = 144 with augmentation: the one-launch backward (k_backward) against the two-launch backward,
    and the prefetching forward against the gathering one; 5 steps, masters and stats equal."""
    B = 144
    data, labels = _random_u8(3 * B, seed=41)
    kw = dict(seed=42, lr=1e-4, relu_logits=False, augment=True)
    eng = FusedCifarEngine(B, data, labels, **kw)
    two = FusedCifarEngine(B, data, labels, **kw, variant={"bwd_fused": False})
    gather = FusedCifarEngine(B, data, labels, **kw, variant={"xraw_prefetch": False})
    plain = FusedCifarEngine(B, data, labels, **dict(kw, augment=False))
    assert eng.bwd_fused and eng.xraw_prefetch and not two.bwd_fused and not gather.xraw_prefetch
    for e in (eng, two, gather, plain):
        for _ in range(5):
            e.step()
        torch.cuda.synchronize()
        e.check_barriers()
    s = _state(eng)
    assert s[0] == 5 and torch.isfinite(s[1]).all()
    for other in (two, gather):
        o = _state(other)
        assert o[0] == 5 and torch.equal(o[1], s[1]) and torch.equal(o[2], s[2])
        assert torch.equal(other.aug, eng.aug)
    assert not torch.equal(plain.master, eng.master), "augmentation changed nothing"


WRITERS = {
    "wgrad_apply": (32, dict(), lambda e: e.wgrad_apply and not e.bwd_fused),
    "k_backward": (144, dict(), lambda e: e.bwd_fused),
    "sgd_launch": (32, dict(variant={"wgrad_sgd": False}), lambda e: not e.wgrad_apply and not e.dp),
    "xgmi_epilogue": (32, dict(dp_force=True, allreduce="xgmi", dp_schedule="serial", variant={"comm_sgd": True}),
                      lambda e: e.comm_sgd),
}


@pytest.mark.parametrize("name", list(WRITERS))
def test_finalizers_write_the_next_table(name):
    """Each launch that finalizes a step writes the next step's words: after 6 steps across an epoch
    boundary (4 steps per epoch) the device table equals the host twin's for step 6 -- after eager
    steps and after chained graph replays, whose weights also agree bit for bit."""
    B, kw, selected = WRITERS[name]
    data, labels = _random_u8(4 * B, seed=51)
    base = dict(seed=52, lr=1e-4, relu_logits=False, augment=True, **kw)
    eager = FusedCifarEngine(B, data, labels, **base)
    graph = FusedCifarEngine(B, data, labels, **base)
    assert selected(eager), f"{name}: the engine chose another path"
    assert eager.period == 4
    assert torch.equal(eager.aug.cpu(), eager.order.augment(0, pad_to=eager.B))
    for _ in range(6):
        eager.step()
    graph.step()
    graph.capture(steps_per_graph=4)
    graph.run(5)
    torch.cuda.synchronize()
    for e in (eager, graph):
        e.check_barriers()
        assert e.global_step() == e.host_step == 6
        want = OrderSpec(4 * B, B, seed=52).augment(6, pad_to=e.B)
        assert not torch.equal(want, e.order.augment(5, pad_to=e.B))
        assert torch.equal(e.aug.cpu(), want), (e.aug.cpu().tolist(), want.tolist())
        assert torch.equal(e.bidx.cpu(), e._padded(e.batch_indices(6)).cpu())
    assert torch.isfinite(eager.master).all() and torch.equal(eager.master, graph.master)
    assert torch.equal(eager.stats[:7], graph.stats[:7])


def test_resume_continues_the_augmented_run():
    B = 32
    data, labels = _random_u8(4 * B, seed=61)
    kw = dict(seed=62, lr=1e-4, relu_logits=False, augment=True)
    whole = FusedCifarEngine(B, data, labels, **kw)
    for _ in range(6):
        whole.step()
    first = FusedCifarEngine(B, data, labels, **kw)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    second = FusedCifarEngine(B, data, labels, **kw)
    second.load_flat_params(first.flat_params())
    second.set_step(3)
    assert torch.equal(second.aug.cpu(), second.order.augment(3, pad_to=B))
    for _ in range(3):
        second.step()
    torch.cuda.synchronize()
    assert second.global_step() == 6 and torch.equal(second.master, whole.master)


def test_augment_needs_the_centre_crop_offsets():
    data, labels = _random_u8(32, seed=1)
    with pytest.raises(ValueError):
        FusedCifarEngine(16, data, labels, crop_offset=(0, 8), augment=True)


def _nccl1_rank(rank, world, port, out, steps, B):
    sys.path.insert(0, REPO)
    import datetime
    import torch.distributed as dist
    import dmlc  # noqa: F401
    from dmlc.engine.fused import FusedCifarEngine as Eng
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60), device_id=torch.device("cuda", 0))
    x, y = _random_u8(4 * B, seed=71)
    eng = Eng(B, x, y, device="cuda:0", seed=72, lr=1e-4, relu_logits=False, dp_force=True, dp_schedule="serial",
              allreduce="rccl", augment=True)
    assert eng.dp and eng.capture_comm
    eng.step()
    eng.capture(steps_per_graph=2)
    eng.run(steps - 1)
    torch.cuda.synchronize()
    torch.save({"flat": eng.flat_params(), "step": eng.global_step(), "aug": eng.aug.cpu()}, os.path.join(out, "aug1.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_rccl_world1_equals_single_gpu(tmp_path):
    """The data-parallel step (conv slabs reduced in the wgrad launch, all-reduce, apply-only SGD that
    finalizes) on a 1-rank nccl group with augmentation equals the single-GPU augment engine."""
    import torch.multiprocessing as mp
    from dmlc.cli import free_port
    B, steps = 32, 4
    mp.spawn(_nccl1_rank, args=(1, free_port(), str(tmp_path), steps, B), nprocs=1, join=True)
    res = torch.load(tmp_path / "aug1.pt", weights_only=True)
    x, y = _random_u8(4 * B, seed=71)
    ref = FusedCifarEngine(B, x, y, device="cuda:0", seed=72, lr=1e-4, relu_logits=False, augment=True)
    for _ in range(steps):
        ref.step()
    torch.cuda.synchronize()
    assert res["step"] == steps
    assert torch.equal(res["aug"], ref.aug.cpu())
    assert torch.equal(res["flat"], ref.flat_params())


def test_training_curve_tracks_eager_fp32_with_augmentation():
    """tests/test_cnn_kernels_gpu.py's curve comparison (linear logits, lr 1e-4, B = 128, 25-step
    windows, 8 %) with augmentation on both engines: the eager fp32 engine draws the same per-image
    words through the host twin, so it stays the fused engine's step-by-step oracle."""
    from dmlc.engine.eager import EagerTrainer
    B, steps, win = 128, 300, 25
    data, labels = synthetic(8192, seed=5, learnable=True)
    kw = dict(seed=6, lr=1e-4, relu_logits=False, staircase=False, augment=True)
    fused = FusedCifarEngine(B, data, labels, **kw)
    fused.step()
    fused.capture()
    fused.run(steps - 1)
    torch.cuda.synchronize()
    fused.check_barriers()
    lf = torch.tensor([fused.read_stats(k)["loss"] for k in range(1, steps + 1)])
    eager = EagerTrainer("cifar_cnn", B, data, labels, device="cuda", dtype="fp32", **kw)
    le = []
    for _ in range(steps):
        eager.step()
        le.append(float(eager.last_loss))
    le = torch.tensor(le)
    wf, we = lf.view(-1, win).mean(1), le.view(-1, win).mean(1)
    dev = ((wf - we).abs() / we).max()
    print(json.dumps({"fused": wf.tolist(), "eager": we.tolist(), "max_dev": float(dev)}))
    assert torch.isfinite(lf).all() and torch.isfinite(le).all()
    assert wf[-1] < math.log(10) and we[-1] < math.log(10), (wf.tolist(), we.tolist())
    assert dev < 0.08, (float(dev), wf.tolist(), we.tolist())


def test_gradients_match_fp32_autograd_on_the_augmented_rows():
    B = 32
    data, labels = synthetic(4 * B, seed=3)
    eng = FusedCifarEngine(B, data, labels, seed=2, augment=True)
    idx = eng.batch_indices(eng.host_step).long()
    words = eng.order.augment(eng.host_step)
    assert torch.equal(eng.aug.cpu(), words) and not bool((words == A.CENTRE).all())
    grad = eng.compute_gradients().cpu()
    flat = eng.flat_params().to("cuda").clone().requires_grad_(True)
    x = apply_augment(data[idx], words).float().to("cuda")
    loss = M.cifar_loss(M.cnn_forward(x, M.views(flat), True), labels[idx].to("cuda"))
    loss.backward()
    gref = flat.grad.detach().cpu()
    for s in M.PARAM_SPECS:
        a, b = grad[s.offset:s.offset + s.numel], gref[s.offset:s.offset + s.numel]
        if b.norm() < 1e-8:
            assert a.norm() < 1e-4, s.name
            continue
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        assert cos > 0.995, (s.name, cos)


def test_fp8_step_takes_the_same_augmented_conv1():
    """fp8 (conv2 on e4m3 operands): one forward + backward at B = 64 with augmentation runs clean, and
    its p1 -- conv1 is bf16 on both paths -- equals the bf16 engine's bit for bit."""
    B = 64
    data, labels = _random_u8(2 * B, seed=81)
    kw = dict(seed=82, lr=1e-4, relu_logits=False, augment=True)
    f8 = FusedCifarEngine(B, data, labels, **kw, dtype="fp8")
    bf = FusedCifarEngine(B, data, labels, **kw)
    assert f8.fp8 and not bf.fp8
    for e in (f8, bf):
        g = e.compute_gradients()
        torch.cuda.synchronize()
        e.check_barriers()
        assert torch.isfinite(g).all()
    assert torch.equal(f8.aug, bf.aug) and torch.equal(f8.p1, bf.p1) and torch.equal(f8.am1, bf.am1)
    plain = FusedCifarEngine(B, data, labels, **dict(kw, augment=False), dtype="fp8")
    plain.compute_gradients()
    assert not torch.equal(plain.p1, f8.p1)
