"""The trunk's backward plan with the paired BatchNorm backward of its downsample blocks
(MMDX_BN_BWD_PAIR=1, the default: mmdx_bn_bwd_pair) against the same plan with the two
separate BN backwards (MMDX_BN_BWD_PAIR=0): one forward + backward each, every parameter
gradient and every running statistic bit-identical."""
import os

import pytest
import torch

import mmdx
import mmdx._lib as L
from parity_util import synth_batch

pytestmark = pytest.mark.gpu


def _step(dev, arch, knob):
    os.environ["MMDX_BN_BWD_PAIR"] = knob
    L.reload_config()
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN(arch, 1024, 13, compute_dtype=torch.bfloat16).to(dev)
    img.unfreeze_backbone()
    trunk = img.backbone
    x, _, _, _ = synth_batch(2, 8, hw=64)
    feats = trunk(x.to(dev))
    g = torch.Generator().manual_seed(3)
    feats.backward(torch.randn(feats.shape, generator=g).to(dev))
    torch.cuda.synchronize()
    plans = [pl for lst in trunk.__dict__["_mmdx_plans"].values() for pl in lst]
    assert len(plans) == 1
    bwd = plans[0].bwd
    n_pair = sum(bwd.arr[k].op == L.OP_BN_BWD_PAIR for k in range(bwd.n))
    n_masked = sum(bwd.arr[k].op == L.OP_BN_BWD_MASKED_DY for k in range(bwd.n))
    grads = {n: p.grad.clone() for n, p in trunk.named_parameters()}
    stats = {n: b.clone() for n, b in trunk.named_buffers()}
    return n_pair, n_masked, grads, stats


@pytest.mark.parametrize("arch,n_ds", [("resnet50", 4), ("resnet18", 3)])
def test_pair_plan_equals_separate_plan(dev, arch, n_ds):
    old = os.environ.get("MMDX_BN_BWD_PAIR")
    try:
        on = _step(dev, arch, "1")
        off = _step(dev, arch, "0")
    finally:
        if old is None:
            os.environ.pop("MMDX_BN_BWD_PAIR", None)
        else:
            os.environ["MMDX_BN_BWD_PAIR"] = old
        L.reload_config()
    # every downsample block's two BN backwards: one paired op, or bn3's + the masked one
    assert (on[0], on[1]) == (n_ds, 0)
    assert (off[0], off[1]) == (0, n_ds)
    assert on[2].keys() == off[2].keys() and len(on[2]) > 20
    for n in on[2]:
        assert torch.equal(on[2][n], off[2][n]), f"grad {n}"
    assert on[3].keys() == off[3].keys() and len(on[3]) > 20
    for n in on[3]:
        assert torch.equal(on[3][n], off[3][n]), f"buffer {n}"
