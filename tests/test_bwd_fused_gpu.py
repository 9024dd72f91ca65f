"""The one-launch backward (engine variant bwd_fused, cnn_bwd.hip k_backward) against the two launches
it merges (k_fc_chain + k_wgrad): the same bodies in the same image order, so every buffer must be
bit-identical -- after an eager step and after chains of captured steps of unequal length (both launch
epoch parities, more than ten launches)."""
import pytest
import torch

from dmlc.engine.fused import FusedCifarEngine

pytestmark = pytest.mark.gpu

SHADOWS = ("w1f", "w2f", "w2d", "fc1n", "fc2t", "fc2n", "fc3t", "fc3d")
BUFFERS = ("master", "stats", "dy2", "dp1", "part1", "part2") + SHADOWS


def _synthetic(n, seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, generator=g)
    return data, labels


def _train(B, relu_logits, fused):
    data, labels = _synthetic(3 * B + 16, seed=B)       # (period 3: the chains cross epoch boundaries)
    eng = FusedCifarEngine(B, data, labels, seed=5, lr=1e-4, relu_logits=relu_logits,
                           variant={"bwd_fused": fused})
    eng.step()
    eng.capture(steps_per_graph=4)
    eng.run(9)                                          # chains of 4, 4 and 1 steps
    torch.cuda.synchronize()
    eng.check_barriers()
    return eng


# B = 144: the smallest batch on this path and the most ragged (a 16-row third row tile, blocks
# 144..255 with a role but no image, conv1 roles 16..127 with one image, conv2 groups of 4 or 5 images);
# B = 176: two-image conv1 roles beside one-image ones, uneven conv2 groups; B = 256: the full map
@pytest.mark.parametrize("B,relu_logits", [(144, False), (176, False), (176, True), (256, False)])
def test_bwd_fused_is_bitwise_the_two_launches(B, relu_logits):
    fused = _train(B, relu_logits, True)
    ref = _train(B, relu_logits, False)
    assert fused.bwd_fused and not ref.bwd_fused
    assert fused.global_step() == ref.global_step() == 10
    assert bool(torch.isfinite(ref.master).all())
    for name in BUFFERS:
        a, b = getattr(fused, name), getattr(ref, name)
        assert torch.equal(a, b), (B, name, int((a != b).sum()))


def test_fc_fused_off_turns_bwd_fused_off_and_still_trains(monkeypatch):
    monkeypatch.setenv("DMLC_FC_FUSED", "0")
    B = 144
    data, labels = _synthetic(2 * B, seed=1)
    eng = FusedCifarEngine(B, data, labels, seed=5, lr=1e-4, relu_logits=False)
    assert not eng.fc_fused and not eng.bwd_fused
    for _ in range(3):
        eng.step()
    torch.cuda.synchronize()
    eng.check_barriers()
    st = eng.read_stats(3)
    assert eng.global_step() == 3 and st["global_step"] == 3 and st["loss"] == st["loss"], st
