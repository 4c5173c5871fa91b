"""CPU: the fp64 GEMM reference of tests/gemm_ref.py against the definition, its case table
against the library's own description of the dense dispatch (mmdx_gemm_describe and the
workspace queries are host-only), the edge every case is in the table for, the preconditions of
the exact comparisons, and how sensitive the comparisons of tests/test_gemm_reference_gpu.py are
next to the whole-tensor bar of tests/test_kernels_gpu.py."""
import os
import re

import pytest
import torch

import gemm_ref as R
from gemm_ref import BF16, F32

import mmdx._lib as L


@pytest.fixture
def knobs_for():
    """Sets the MMDX_* knobs of a case (the library re-reads them); restores the environment."""
    saved = {k: os.environ.get(k) for k in R.KNOB_NAMES}

    def set_(c):
        for k in R.KNOB_NAMES:
            os.environ.pop(k, None)
        for k, v in c.knobs.items():
            os.environ[k] = str(v)
        L.reload_config()
    yield set_
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    L.reload_config()


# -------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 2, 9)])
def test_reference_matches_triple_loop(shape):
    """A B^T by the definition, both operand families; the integer one is exact."""
    M, N, K = shape
    g = torch.Generator().manual_seed(M * N * K)
    A, B = R.gen_integer((M, K), g), R.gen_integer((N, K), g)
    r = R.ref_gemm(A, B)
    assert torch.equal(r.acc, R.triple_loop(A, B))
    assert torch.equal(r.z_terms, R.triple_loop(A.abs(), B.abs()))
    A, B = R.gen_gaussian((M, K), g, BF16), R.gen_gaussian((N, K), g, BF16)
    r = R.ref_gemm(A, B)
    assert (r.acc - R.triple_loop(A, B)).abs().max() <= 1e-14 * r.z_terms.max()
    w = R.ref_wgrad_bias(A.T, B.T)      # dY = A^T [K, M], X = B^T [K, N]
    assert torch.equal(w.dW, r.acc) and torch.equal(w.db, A.sum(1))


def test_reference_epilogue_order():
    """apply()'s order on values where the order shows: alpha before the bias, the activation
    before beta * C0 and the residual, gelu' before bias and addend."""
    A, B = torch.tensor([[2.0, -1.0]]), torch.tensor([[3.0, 1.0], [-1.0, 1.0]])   # acc = 5, -3
    bias, add = torch.tensor([1.0, 1.0]), torch.tensor([[-2.0, 0.5]])
    C0, res = torch.tensor([[4.0, 4.0]]), torch.tensor([[0.25, -0.25]])
    r = R.ref_gemm(A, B, 2.0, bias, add, "relu", 0.5, C0, res)
    assert r.z.tolist() == [[9.0, -4.5]] and r.y.tolist() == [[11.25, 1.75]]
    assert r.z_terms.tolist() == [[17.0, 7.5]] and r.y_terms.tolist() == [[19.25, 9.75]]
    pre = torch.tensor([[0.0, 30.0]])                                            # gelu' = 0.5, 1
    r = R.ref_gemm(A, B, 2.0, bias, add, "gelu_bwd", 0.0, None, None, pre)
    assert r.y.tolist() == [[4.0, -4.5]]
    x = torch.linspace(-6, 6, 2001, dtype=torch.float64)
    assert (R.gelu(x) - torch.nn.functional.gelu(x)).abs().max() < 1e-15
    xg = x.clone().requires_grad_()
    torch.nn.functional.gelu(xg).sum().backward()
    assert (R.gelu_grad(x) - xg.grad).abs().max() < 1e-14
    assert R.gelu_grad(x).abs().max() <= R.GELU_LIP


def test_reference_matches_torch_fp32_on_the_integer_family():
    """Integer operands: an fp32 matmul is exact, so it equals the fp64 reference."""
    for c in R.CASES:
        if "int" not in c.families or c.kind != "gemm":
            continue
        h = R.host(c, "int")
        assert torch.equal((h.A.float() @ h.B.float().T).double(), h.r.acc), c.id


def test_layouts():
    m = torch.arange(6, dtype=torch.float64).view(2, 3)          # R = 2 rows, K = 3
    buf, ld = R.store(m, 1, 2, 1, F32)
    assert ld == 5 and buf.isnan().tolist() == [True, False, False, False, True, True,
                                                False, False, False, True, True]
    assert buf[1:4].tolist() == [0.0, 1.0, 2.0] and buf[6:9].tolist() == [3.0, 4.0, 5.0]
    buf, ld = R.store(m, 0, 1, 0, F32)                           # element (r, k) at k * ld + r
    assert ld == 3 and buf[[0, 1, 3, 4, 6, 7]].tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0]
    assert buf[[2, 5, 8]].isnan().all()
    out = R.matrix((2, 3), 4, 2, F32, -7.0, m, guard=3)
    assert out.tolist() == [-7.0, -7.0, 0.0, 1.0, 2.0, -7.0, 3.0, 4.0, 5.0, -7.0, -7.0, -7.0, -7.0]
    assert torch.equal(R.view(out, (2, 3), 4, 2)[:, :3], m.float())


# ------------------------------------------------------------------- the table and the library
def test_mirror_equals_describe_on_every_case(knobs_for):
    lib = L.lib()
    for c in R.CASES:
        knobs_for(c)
        assert R.expected_path(c).desc == R.describe(lib, c), c.id


def test_describe_follows_the_address_bits_and_rejects_bad_arguments(knobs_for):
    import ctypes
    lib = L.lib()
    c = R.BY_ID["bf16-dma-k72-kk"]
    knobs_for(c)
    assert R.describe(lib, c).startswith("dma8/")
    for low in (2, 8):
        assert R.describe(lib, c, a_low4=low).startswith("kload/")
        assert R.describe(lib, c, b_low4=low).startswith("kload/")
    buf = ctypes.create_string_buffer(64)
    assert lib.mmdx_gemm_describe(1, 136, 200, 72, 72, 1, 0, 72, 1, 0, 0, buf, 4) != 0
    assert lib.mmdx_gemm_describe(7, 136, 200, 72, 72, 1, 0, 72, 1, 0, 0, buf, 64) != 0
    assert lib.mmdx_gemm_describe(1, 136, 0, 72, 72, 1, 0, 72, 1, 0, 0, buf, 64) != 0
    assert lib.mmdx_gemm_describe(1, 136, 200, 72, 72, 1, 0, 72, 1, 0, 1, buf, 64) != 0


def test_splits_equal_the_workspace_queries(knobs_for):
    lib = L.lib()
    for c in R.CASES:
        knobs_for(c)
        M, N, K, _, _ = R.shapes(c)
        s = R.expected_path(c).splits
        code = L.dtype_code(c.dt)
        gemm_ws = lib.mmdx_gemm_workspace_size(code, M, N, K)
        assert gemm_ws == (s * 4 * M * N if s > 1 else 0), c.id
        if c.kind == "wb":
            fused = s * (M * N + M) * 4 if s > 1 else 0
            want = max(fused, gemm_ws, lib.mmdx_bias_grad_workspace_size(K, M))
            assert lib.mmdx_gemm_bias_grad_workspace_size(code, M, N, K) == want, c.id
            if R.expected_path(c).fused:
                assert want == fused


# The paths the table must keep reaching, per dtype class.  This is NOT the product of kernel
# paths and reduce / epilogue kinds (dma4/64x64 with a per-element epilogue, or dma4 with
# reduce1, can be produced and are absent); it is their union: every kernel path (family, tile,
# stages, one | split) at least once, and every (partial store, reduce, epilogue) kind at least
# once, on the paths listed.  16-bit kernel paths: kload on all four tiles; dma4 on the three
# 64-wide tiles and (MMDX_GEMM_8W128=0) on 128 x 128, each with 2 and 3 stages; dma8 on
# 128 x 128 with 2 and 3 stages and on 256 x 256; the fused weight + bias gradient on its three
# kernels.  Kinds: both reduces after both partial stores; the EpiStore through apply8_fast
# (vec8), apply4's 4-wide stores (vec4; every fourth row at ldc % 4 != 0: vec4+elem) and apply()
# (elem).  fp32: kload only.
_PATHS_16 = """
dma4/128x128/ns2/one|none>none|vec8
dma4/128x128/ns3/one|none>none|vec8
dma4/128x128/ns3/split|p8>reduce4|vec4
dma4/128x64/ns2/one|none>none|vec8
dma4/128x64/ns3/one|none>none|vec8
dma4/128x64/ns3/split|p8>reduce4|vec4
dma4/64x128/ns2/one|none>none|vec8
dma4/64x128/ns3/one|none>none|vec8
dma4/64x128/ns3/split|p8>reduce4|vec4
dma4/64x64/ns2/one|none>none|vec8
dma4/64x64/ns3/one|none>none|vec8
dma4/64x64/ns3/split|p8>reduce4|vec4
dma8/128x128/ns2/one|none>none|elem
dma8/128x128/ns2/one|none>none|vec4
dma8/128x128/ns2/one|none>none|vec4+elem
dma8/128x128/ns2/one|none>none|vec8
dma8/128x128/ns3/one|none>none|vec8
dma8/128x128/ns3/split|p4>reduce1|elem
dma8/128x128/ns3/split|p8>reduce1|elem
dma8/128x128/ns3/split|p8>reduce4|elem
dma8/128x128/ns3/split|p8>reduce4|vec4
dma8/128x128/ns3/split|p8>reduce4|vec4+elem
dma8/256x256/ns2/one|none>none|elem
dma8/256x256/ns2/one|none>none|vec4
dma8/256x256/ns2/one|none>none|vec4+elem
dma8/256x256/ns2/one|none>none|vec8
kload/128x128/ns2/one|none>none|elem
kload/128x128/ns2/one|none>none|vec4
kload/128x128/ns2/one|none>none|vec4+elem
kload/128x128/ns2/split|p4>reduce1|elem
kload/128x128/ns2/split|p4>reduce4|vec4
kload/128x64/ns2/one|none>none|vec4
kload/64x128/ns2/one|none>none|vec4
kload/64x64/ns2/one|none>none|vec4
wb-fused/dma4/128x128/ns3/split|p8>reduce4|vec4
wb-fused/dma4/128x64/ns3/split|p8>reduce4|vec4
wb-fused/dma8/128x128/ns3/split|p8>reduce4|vec4
wb-unfused/dma8/128x128/ns2/one|none>none|vec8
wb-unfused/dma8/128x128/ns3/split|p8>reduce4|vec4
wb-unfused/kload/128x128/ns2/split|p4>reduce4|vec4
""".split()
_PATHS_32 = """
kload/128x128/ns2/one|none>none|elem
kload/128x128/ns2/one|none>none|vec4
kload/128x128/ns2/split|p4>reduce1|elem
kload/128x128/ns2/split|p4>reduce4|vec4
kload/64x64/ns2/one|none>none|vec4
wb-unfused/kload/128x128/ns2/split|p4>reduce4|vec4
""".split()
REQUIRED_PATHS = sorted([f"{t}:{p}" for t in ("bf16", "f16") for p in _PATHS_16] +
                        [f"f32:{p}" for p in _PATHS_32])


def test_case_table_reaches_every_dispatcher_path():
    reached = sorted({R.expected_path(c).key for c in R.CASES})
    assert reached == REQUIRED_PATHS, (sorted(set(REQUIRED_PATHS) - set(reached)),
                                       sorted(set(reached) - set(REQUIRED_PATHS)))


def facts(c):
    """What a case exercises, from the mirror: the fields EDGES asserts."""
    e = R.expected_path(c)
    M, N, K, ak, bk = R.shapes(c)
    p, d = e.plan, e.path
    return dict(family=d.family, tile=f"{d.bm}x{d.bn}", ns=d.ns, splits=p.splits, asked=p.asked,
                kper=p.kper, ktail=K % R.BK[c.dt], last=K - (p.splits - 1) * p.kper, va=d.va,
                vb=d.vb, reduce=e.reduce, partial=e.partial, epi=e.epi, fused=e.fused,
                vtail=K % (16 // R.ESIZE[c.dt]), mrag=M % d.bm, nrag=N % d.bn, n4=N % 4, n8=N % 8)


# (pattern of the case ids, how many cases it names, the edge they are in the table for).  A
# case no pattern names, a pattern with another count, or a fact that moved fails
# test_every_case_sits_on_its_edge: removing or reshaping a case shows here.
D8 = dict(family="dma8", tile="128x128", va=True, vb=True, mrag=8, nrag=72)
EDGES = [
    (r"^(bf16|f16)-dma-k72-(kk|kr|rr|rk)$", 8, dict(D8, ns=2, splits=1, ktail=8, epi="vec8")),
    (r"^(bf16|f16)-dma-k328-", 8, dict(D8, ns=3, splits=1, kper=384, ktail=8)),
    (r"^(bf16|f16)-dma-k520-(kk|kr|rr|rk)$", 8,
     dict(D8, ns=3, splits=2, asked=2, last=200, reduce="reduce4", partial="p8")),
    (r"-dma-k776$", 2, dict(D8, splits=3, asked=3, last=136, reduce="reduce4")),
    (r"-dma-k1160$", 2, dict(D8, splits=4, asked=4, last=200, reduce="reduce4")),
    (r"-dma-k1600$", 2, dict(D8, splits=5, asked=6, kper=320, last=320, reduce="reduce4")),
    (r"-dma-k1736$", 2, dict(D8, splits=7, asked=7, kper=256, last=200, reduce="reduce4")),
    (r"-dma-n201$", 2, dict(family="dma8", splits=2, n4=1, partial="p4", reduce="reduce1")),
    (r"-dma-n203$", 2, dict(family="dma8", splits=2, n4=3, partial="p4", reduce="reduce1")),
    (r"-dma-n204-split$", 2, dict(family="dma8", splits=2, n4=0, n8=4, partial="p8",
                                  reduce="reduce4")),
    (r"-dma-n204$", 2, dict(family="dma8", splits=1, n8=4, epi="vec8")),
    (r"-dma-n203-ldc208$", 2, dict(family="dma8", splits=1, n8=3, epi="vec8")),
    (r"-dma-k520-novec$", 2, dict(D8, splits=2, n4=0, partial="p8", reduce="reduce1",
                                  epi="elem")),
    (r"-t40x48-k72$", 2, dict(family="dma4", tile="64x64", ns=2, splits=1, ktail=8)),
    (r"-t40x200-k72$", 2, dict(family="dma4", tile="64x128", ns=2, splits=1, ktail=8)),
    (r"-t200x40-k72$", 2, dict(family="dma4", tile="128x64", ns=2, splits=1, ktail=8)),
    (r"-t40x48-k328$", 2, dict(family="dma4", tile="64x64", ns=3, splits=1)),
    (r"-t40x200-k328$", 2, dict(family="dma4", tile="64x128", ns=3, splits=1)),
    (r"-t200x40-k328$", 2, dict(family="dma4", tile="128x64", ns=3, splits=1)),
    (r"-t40x48-k520$", 2, dict(family="dma4", tile="64x64", ns=3, splits=2, last=200)),
    (r"-t40x200-k520$", 2, dict(family="dma4", tile="64x128", ns=3, splits=2, last=200)),
    (r"-t200x40-k520$", 2, dict(family="dma4", tile="128x64", ns=3, splits=2, last=200)),
    (r"-t64x64$", 2, dict(family="dma4", tile="64x64", mrag=0, nrag=0)),
    (r"-t65x65$", 2, dict(family="dma8", tile="128x128", mrag=65, nrag=65)),
    (r"-t40x48-rr$", 2, dict(family="dma4", tile="64x64")),
    (r"-w4-k72$", 2, dict(family="dma4", tile="128x128", ns=2, splits=1)),
    (r"-w4-k328$", 2, dict(family="dma4", tile="128x128", ns=3, splits=1)),
    (r"-w4-k520(-rr)?$", 4, dict(family="dma4", tile="128x128", ns=3, splits=2)),
    (r"-256-k136$", 2, dict(family="dma8", tile="256x256", ktail=8, mrag=44, nrag=4)),
    (r"-256-k128$", 2, dict(family="dma8", tile="256x256", ktail=0, kper=128, epi="vec8")),
    (r"-256-k120$", 2, dict(family="dma8", tile="128x128", splits=1)),
    (r"-256-n513$", 2, dict(family="dma8", tile="256x256", mrag=1, nrag=1)),
    (r"^(bf16|f16)-256-gelu$", 2, dict(family="dma8", tile="256x256", epi="vec8")),
    (r"-pad-k72-(kk|rr)$", 4, dict(D8, splits=1, epi="vec8")),
    (r"-pad-k520$", 2, dict(D8, splits=2)),
    (r"-pad-256$", 2, dict(family="dma8", tile="256x256", epi="vec8")),
    (r"-kl-k75$", 2, dict(family="kload", va=False, vb=False, vtail=3, ktail=11)),
    (r"-kl-k13$", 2, dict(family="kload", va=False, vtail=5, ktail=13)),
    (r"-kl-k76-vec$", 2, dict(family="kload", va=True, vb=True, vtail=4, ktail=12)),
    (r"-kl-k523$", 2, dict(family="kload", va=False, splits=2, last=203, reduce="reduce4")),
    (r"-kl-k523-vec$", 2, dict(family="kload", va=True, vb=True, splits=2, last=203)),
    (r"-kl-k523-n201$", 2, dict(family="kload", splits=2, reduce="reduce1")),
    (r"-kl-rr$", 2, dict(family="kload", va=False, vb=False, mrag=2, nrag=74)),
    (r"-kl-rr-vec$", 2, dict(family="kload", va=True, vb=True, mrag=2, nrag=74)),
    (r"-kl-lda1$", 2, dict(family="kload", va=False, vb=True, vtail=0)),
    (r"-kl-aoff$", 2, dict(family="kload", va=False, vb=True, vtail=0)),
    (r"-kl-boff-rr$", 2, dict(family="kload", va=True, vb=False)),
    (r"-kl-t40x48$", 2, dict(family="kload", tile="64x64")),
    (r"-kl-t40x200$", 2, dict(family="kload", tile="64x128")),
    (r"-kl-t200x40$", 2, dict(family="kload", tile="128x64")),
    (r"-epi-dma-", 2 * 20, dict(family="dma8", tile="128x128", splits=1)),
    (r"-epi-r4-", 2 * 18, dict(family="dma8", splits=2, reduce="reduce4")),
    (r"-epi-r1-", 2 * 18, dict(family="dma8", splits=2, reduce="reduce1", epi="elem")),
    (r"-epi-256-", 2 * 19, dict(family="dma8", tile="256x256")),
    (r"-epi-kl-", 2 * 18, dict(family="kload", splits=1)),
    (r"-epi-(dma|256)-(a05|a2|ba|b1|res|relu|pre|all|all-f32|f32|all-ldc8|gelu|gelu-f32|gbwd|"
     r"gbwd-b|c16)$", 2 * 31, dict(epi="vec8")),
    (r"-epi-(dma|256)-(all-ldc1|gbwd-ba|biasoff)$", 2 * 6, dict(epi="elem")),
    (r"-epi-(dma|256|kl)-ldc1$", 2 * 3, dict(epi="vec4+elem")),
    (r"-epi-r4-(a05|a2|b1|f32)$", 2 * 4, dict(epi="vec4")),
    (r"-epi-r4-ldc1$", 2, dict(epi="vec4+elem")),
    (r"-wb-(136x72|136x64|264x136)(-c16|-lda)?$", 18, dict(fused=True, reduce="reduce4")),
    (r"-wb-(136x72|264x136)(-c16|-lda)?$", 12, dict(family="dma8", tile="128x128")),
    (r"-wb-136x64", 8, dict(tile="128x64", family="dma4")),
    (r"-wb-(136x72|264x136)-w4$", 4, dict(fused=True, family="dma4", tile="128x128")),
    (r"-wb-136x(72|64)", 16, dict(splits=2, last=200, mrag=8)),
    (r"-wb-264x136", 8, dict(splits=7, last=200, mrag=8, nrag=8)),
    (r"-wb-k72$", 2, dict(fused=False, splits=1)),
    (r"-wb-m132$", 2, dict(fused=False, family="kload", splits=2)),
    (r"-wb-off$", 2, dict(fused=False, family="dma8", splits=2)),
    (r"-bg-520x72-", 4, dict(family="dma4", tile="64x128", splits=2, last=200)),
    (r"-bg-8x8-", 4, dict(family="dma4", tile="64x64", splits=1)),
    (r"^f32-", 12, dict(family="kload", ns=2)),
    (r"^f32-k70(-kr)?$", 2, dict(va=False, vtail=2, ktail=6, splits=1)),
    (r"^f32-k70-rr$", 1, dict(va=True, vb=True, ktail=6, mrag=8, nrag=72)),
    (r"^f32-k70-vec$", 1, dict(va=True, vb=True, vtail=2)),
    (r"^f32-k300$", 1, dict(splits=2, kper=160, last=140, reduce="reduce4")),
    (r"^f32-k300-n201$", 1, dict(splits=2, reduce="reduce1")),
    (r"^f32-t40x48$", 1, dict(tile="64x64", ktail=1)),
    (r"^f32-a05$", 1, dict(splits=2)),
    (r"^f32-wb$", 1, dict(fused=False, splits=2)),
]


def test_every_case_sits_on_its_edge():
    named = set()
    for pat, count, want in EDGES:
        hit = [c for c in R.CASES if re.search(pat, c.id)]
        assert len(hit) == count, (pat, len(hit))
        for c in hit:
            f = facts(c)
            got = {k: f[k] for k in want}
            assert got == want, (c.id, pat, got)
            named.add(c.id)
    assert named == set(R.BY_ID), sorted(set(R.BY_ID) - named)
    for c in R.CASES:
        M, N, K, _, _ = R.shapes(c)
        assert M <= 600 and N <= 600 and K <= 2200, c.id
        if not c.ak and R.ESIZE[c.dt] == 2 and facts(c)["family"] != "kload":
            assert M % 8 == 0, c.id


def test_integer_family_preconditions_of_the_whole_table():
    """Every value an integer-family run stores is exactly representable (|v| <= 256 in bf16,
    <= 2048 in fp16, half-integers from alpha = 0.5 within half of that), with fewer than 2^24
    terms; the seeds are fixed, so the largest |A B^T| stays what it is."""
    top = 0.0
    for c in R.CASES:
        if "int" not in c.families:
            continue
        h = R.host(c, "int")
        R.exact_preconditions(h)
        if c.kind == "gemm":
            top = max(top, h.r.acc.abs().max().item())
            h2 = R.host(c, "int")
            assert torch.equal(h.A, h2.A) and torch.equal(h.r.y, h2.r.y), c.id
    assert 40 <= top <= 128, top


# ------------------------------------------------------------------------------ sensitivity
def _whole_tensor_err(got, ref):
    """tests/test_kernels_gpu.py _close's figure."""
    return ((got - ref).abs().max() / ref.abs().max()).item()


def test_one_dropped_product_fails_both_comparisons_and_passes_the_old_bar():
    c = R.BY_ID["bf16-dma-k1736"]
    m, n = 3, 5
    h = R.host(c, "int")
    k = int((h.A[m] * h.B[n]).abs().argmax())
    assert h.A[m, k] * h.B[n, k] != 0
    got = h.r.y.clone()
    got[m, n] -= h.A[m, k] * h.B[n, k]
    with pytest.raises(AssertionError):
        R.assert_exact(got, h.r.y, "one product dropped")
    assert _whole_tensor_err(got, h.r.y) <= 2e-2          # TOL[bf16]
    R.assert_exact(h.r.y.clone(), h.r.y, "untouched")

    h = R.host(c, "gauss")
    prod = (h.A[m] * h.B[n]).abs()
    k = int(prod.argsort()[len(prod) // 2])               # a term of median size
    stored = h.r.y.to(BF16).double()                      # what a correct kernel stores
    assert R.assert_bounded("self", stored, h.r.y, h.r.y_terms, BF16, "rounded reference") <= 1.0
    got = (h.r.y - h.A[m, k] * h.B[n, k]).to(BF16).double()
    got = torch.where(torch.zeros_like(got, dtype=torch.bool).index_put_(
        (torch.tensor(m), torch.tensor(n)), torch.tensor(True)), got, stored)
    with pytest.raises(AssertionError):
        R.assert_bounded("self", got, h.r.y, h.r.y_terms, BF16, "one median product dropped")
    assert _whole_tensor_err(got, h.r.y) <= 1e-2


def test_skipped_split_or_k_tail_fails_the_exact_comparison():
    """A reduce that skips its last split, and a main loop that drops the 8-element K tail."""
    c = R.BY_ID["bf16-dma-k520-kk"]
    h = R.host(c, "int")
    kper = R.expected_path(c).plan.kper
    got = h.A[:, :kper] @ h.B[:, :kper].T
    with pytest.raises(AssertionError):
        R.assert_exact(got, h.r.y, "last split skipped")
    tail = h.A[:, :512] @ h.B[:, :512].T                  # one dropped 8-element K tail
    with pytest.raises(AssertionError):
        R.assert_exact(tail, h.r.y, "K tail dropped")
