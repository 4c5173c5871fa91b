"""Structure of the ResNet trunk's launch plans (mmdx.resnet._Plan), recorded on the host with
CPU tensors standing in for device memory (nothing is launched; the arena's events are host
stand-ins): every workspace placeholder patched, the timed-op events paired, one forward
conv / weight gradient per Conv2d and one dgrad per Conv2d but the stem, every stream wait
preceded by its signal on another stream, the op variants each dtype picks, and the
parameter-gradient layout and data-parallel regions tiling the flat gradient arena.  No
golden op list: tools/plan_dump.py diffs two revisions of the planner op for op; the plans'
arithmetic is checked on the GPU (test_trunk_launches_gpu.py, test_trunk_pair_plan_gpu.py).
"""
import functools
import os

import pytest
import torch

from mmdx import _lib as L
from mmdx import resnet as RN

CPU = torch.device("cpu")
BF16, F32 = torch.bfloat16, torch.float32
N_CONV = {"resnet50": 53, "resnet18": 20}
DGRADS = (L.OP_CONV_DGRAD, L.OP_CONV_DGRAD_ACCMASK, L.OP_CONV_DGRAD_BNSTAT)

# arch, dtype, train, keep (a backward is recorded), all at 2 x 3 x 64 x 64 NCHW input
WITH_BWD = [("resnet50", BF16, True, True), ("resnet18", BF16, True, True),
            ("resnet50", F32, True, True), ("resnet18", F32, False, True)]
FOLDED = ("resnet50", BF16, False, False)


def _cases(cfgs):
    return [pytest.param(*c, id=f"{c[0]}-{str(c[1])[6:]}-{'train' if c[2] else 'eval'}"
                         + ("" if c[3] else "-folded")) for c in cfgs]


@functools.lru_cache(maxsize=None)
def _trunk(arch):
    torch.manual_seed(0)
    return RN.ResNetTrunk(arch)


@functools.lru_cache(maxsize=None)
def _plan(arch, T, train, keep, pair="1"):
    """(trunk, plan); `pair`: MMDX_BN_BWD_PAIR while recording."""
    trunk = _trunk(arch)
    old = os.environ.get("MMDX_BN_BWD_PAIR")
    os.environ["MMDX_BN_BWD_PAIR"] = pair
    try:
        L.reload_config()
        return trunk, RN._Plan(trunk, 2, 64, 64, True, 3, T, train, keep, CPU)
    finally:
        if old is None:
            os.environ.pop("MMDX_BN_BWD_PAIR", None)
        else:
            os.environ["MMDX_BN_BWD_PAIR"] = old
        L.reload_config()


def _ops(lst):
    return [lst.arr[i] for i in range(lst.n)]


def _count(ops, *codes):
    return sum(o.op in codes for o in ops)


def _check_list(lst):
    ops = _ops(lst)
    for o in ops:
        for j in range(12):
            assert not (o.ext[j] == -1 and o.p[j] in (1, 2)), "unpatched workspace placeholder"
    assert _count(ops, L.OP_EVENT) == 2 * len(lst.conv_names)
    signalled = {}   # event -> stream that signalled it
    for k, o in enumerate(ops):
        if o.op == L.OP_SIGNAL:
            signalled[o.p[0]] = o.stream
        elif o.op == L.OP_WAIT:
            assert o.p[0] in signalled, f"op {k}: wait for an event nothing signalled before"
            assert signalled[o.p[0]] != o.stream, f"op {k}: wait on the signalling stream"
    return ops


@pytest.mark.parametrize("arch,T,train,keep", _cases(WITH_BWD + [FOLDED]))
def test_forward_plan(arch, T, train, keep):
    _, plan = _plan(arch, T, train, keep)
    fwd = _check_list(plan.fwd)
    assert _count(fwd, L.OP_CONV_FWD, L.OP_CONV_FWD_BNEVAL) == N_CONV[arch]
    if not train and not keep:   # eval-mode BN folded into every conv's epilogue
        assert plan.bwd is None
        assert _count(fwd, L.OP_CONV_FWD) == 0 and _count(fwd, L.OP_BN_FWD) == 0


@pytest.mark.parametrize("arch,T,train,keep", _cases(WITH_BWD))
def test_backward_plan(arch, T, train, keep):
    _, plan = _plan(arch, T, train, keep)
    bwd = _check_list(plan.bwd)
    wgrads = [o for o in bwd if o.op == L.OP_CONV_WGRAD]
    assert len(wgrads) == N_CONV[arch] and all(o.stream == 1 for o in wgrads)
    assert _count(bwd, *DGRADS) == N_CONV[arch] - 1    # none into the image
    got = tuple(_count(bwd, c) for c in (L.OP_BN_BWD_PAIR, L.OP_BN_BWD_MASKED_DY,
                                         L.OP_CONV_DGRAD_ACCMASK, L.OP_CONV_DGRAD_BNSTAT))
    want = {("resnet50", BF16): (4, 0, 12, 32), ("resnet18", BF16): (3, 0, 5, 8)}
    assert got == want.get((arch, T), (0, 0, 0, 0))


@pytest.mark.parametrize("arch,n_ds", [("resnet50", 4), ("resnet18", 3)])
def test_backward_plan_unpaired(arch, n_ds):
    """MMDX_BN_BWD_PAIR=0: each downsample block's two BN backwards stay separate ops."""
    _, plan = _plan(arch, BF16, True, True, pair="0")
    bwd = _check_list(plan.bwd)
    assert (_count(bwd, L.OP_BN_BWD_PAIR), _count(bwd, L.OP_BN_BWD_MASKED_DY)) == (0, n_ds)


@pytest.mark.parametrize("arch,T,train,keep", _cases(WITH_BWD))
def test_gradient_layout_and_regions(arch, T, train, keep):
    trunk, plan = _plan(arch, T, train, keep)
    off = 0
    for q in trunk.engine_params():
        assert plan.grad_off[id(q)] == off, "gap, overlap or order in the gradient arena"
        off += (q.numel() * 4 + 15) // 16 * 16
    assert off == plan.grad_bytes
    # layers 4, 3, 2 (backward order) tile the arena's tail; stem + layer 1 are its head
    regions = [(lo, hi) for lo, hi, _event in plan.grad_regions]
    assert len(regions) == 3
    layer2_lo = plan.grad_off[id(trunk[5][0].conv1.weight)] // 4   # its first engine param
    assert regions[-1][0] == layer2_lo and regions[0][1] == plan.grad_bytes // 4
    assert all(lo < hi for lo, hi in regions)
    assert all(a[0] == b[1] for a, b in zip(regions[:-1], regions[1:]))
    assert plan.grad_tail == regions[0][0]
    assert len(plan.bwd.bounds) == len(regions) + 2
