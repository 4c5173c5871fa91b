"""fp64 CPU reference for the dense GEMM entry points of csrc/gemm_dense.hip (mmdx_gemm,
mmdx_gemm_res, mmdx_gemm_bias_grad, and mmdx_bias_grad's GEMM form): the epilogue in
EpiStore::apply()'s order with its sum of |terms|, the operand layouts the kernels read (both
orientations, padded leading dimensions, offset base pointers), the case table of
tests/test_gemm_reference_gpu.py with its knob runs, and expected_path(): a host mirror of
plan_dense + dense_path + the reduce / epilogue choices that names the kernel path each case
takes (tests/test_gemm_ref_cpu.py holds it against mmdx_gemm_describe for every case).

Generators and comparisons are conv_ref's (gen_integer, gen_gaussian, check_exact_preconditions,
assert_exact, bound_ratio, H_T, ACC)."""
import math
from types import SimpleNamespace

import torch

from conv_ref import (ACC, BF16, F16, F32, H_T, assert_exact, bound_ratio,  # noqa: F401
                      check_exact_preconditions, gen_gaussian, gen_integer)

DT_NAME = {BF16: "bf16", F16: "f16", F32: "f32"}
ESIZE = {BF16: 2, F16: 2, F32: 4}
BK = {BF16: 64, F16: 64, F32: 32}     # igemm.h KTile<T>::BK
GELU_LIP = 1.13                       # max |gelu'| (1.1290 at x = sqrt(2))
NAN = float("nan")


# -------------------------------------------------------------------------------- reference
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + \
        x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_grad_terms(x):
    """Sum of |terms| of common.h gelu_erf_grad: 0.5 + 0.5 erf(x / sqrt 2) + x pdf(x).  The
    three cancel in the left tail and at gelu's minimum (x = -0.7518, gelu' = 0), so the fp32
    evaluation's error is a few 2^-24 of THIS, however small gelu' itself is."""
    return 0.5 + 0.5 * torch.erf(x / math.sqrt(2.0)).abs() + \
        x.abs() * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def ref_gemm(A, B, alpha=1.0, bias=None, addend=None, act="none", beta=0.0, C0=None, res=None,
             pre_in=None):
    """C = act(alpha * A B^T + bias + addend) + beta * C0 + res for A [M, K], B [N, K] (fp64),
    in EpiStore::apply()'s order; act in none | relu | gelu | gelu_bwd.  gelu_bwd multiplies
    alpha * acc by gelu'(pre_in) first and then adds bias and addend (pre_in is an input).

    Returns acc = A B^T; z, the value in front of the activation (what the pre-activation copy
    receives); y = C; z_terms / y_terms, the sums of |terms| an fp32 evaluation of z / y adds up
    (for GELU the accumulation term scaled by GELU's Lipschitz constant); g = gelu'(pre_in) or
    None."""
    A, B = A.double(), B.double()
    acc = A @ B.T
    v = alpha * acc
    terms = abs(alpha) * (A.abs() @ B.abs().T)
    g = None
    if act == "gelu_bwd":
        g = gelu_grad(pre_in.double())
        v = v * g
        terms = terms * g.abs()
    if bias is not None:
        v = v + bias.double()
        terms = terms + bias.double().abs()
    if addend is not None:
        v = v + addend.double()
        terms = terms + addend.double().abs()
    z, z_terms = v, terms
    if act == "relu":
        v = v.clamp(min=0.0)
    elif act == "gelu":
        terms = GELU_LIP * terms
        v = gelu(v)
    if beta != 0.0:
        v = v + beta * C0.double()
        terms = terms + (beta * C0.double()).abs()
    if res is not None:
        v = v + res.double()
        terms = terms + res.double().abs()
    return SimpleNamespace(acc=acc, z=z, z_terms=z_terms, y=v, y_terms=terms, g=g)


def ref_wgrad_bias(dY, X):
    """mmdx_gemm_bias_grad: dW = dY^T X and db = column sums of dY for dY [K, M], X [K, N]
    (fp64), with their sums of |terms|."""
    dY, X = dY.double(), X.double()
    return SimpleNamespace(dW=dY.T @ X, dW_terms=dY.abs().T @ X.abs(), db=dY.sum(0),
                           db_terms=dY.abs().sum(0))


def triple_loop(A, B):
    """A B^T by the definition, one product at a time (tiny shapes only)."""
    M, K = A.shape
    N = B.shape[0]
    out = torch.zeros(M, N, dtype=torch.float64)
    for m in range(M):
        for n in range(N):
            s = 0.0
            for k in range(K):
                s += A[m, k].item() * B[n, k].item()
            out[m, n] = s
    return out


# ---------------------------------------------------------------------------------- layouts
def store(mat, kmajor, ld_pad, off, dt, fill=NAN):
    """The operand mat [R, K] (fp64) as the kernels read it: element (r, k) at base[r*ld + k]
    (kmajor) or base[k*ld + r], ld = the minimum + ld_pad, base = off elements into a 1-D buffer.
    Padding and the elements in front of base hold `fill` (NaN: a read of padding shows in an
    exact comparison).  Returns (buffer, ld)."""
    m = mat if kmajor else mat.T
    rows, cols = m.shape
    ld = cols + ld_pad
    buf = torch.full((off + rows * ld,), fill, dtype=dt)
    buf[off:].view(rows, ld)[:, :cols] = m.to(dt)
    return buf, ld


def matrix(shape, ld, off, dt, fill, mat=None, guard=64):
    """An [M, N] matrix of the output side (C, preact, addend, residual) in a 1-D buffer: row m
    at off + m * ld, everything else (the elements in front, padding columns, `guard` elements
    behind) = fill; mat None leaves the whole buffer at fill."""
    M, N = shape
    buf = torch.full((off + M * ld + guard,), fill, dtype=dt)
    if mat is not None:
        buf[off:off + M * ld].view(M, ld)[:, :N] = mat.to(dt)
    return buf


def view(buf, shape, ld, off):
    """The [M, ld] view of a matrix() buffer."""
    return buf[off:off + shape[0] * ld].view(shape[0], ld)


# ------------------------------------------------------------------------------- case table
def make_case(cid, dt, M, N, K, ak=1, bk=1, **kw):
    c = SimpleNamespace(
        id=cid, kind="gemm", dt=dt, M=M, N=N, K=K, ak=ak, bk=bk,
        lda_pad=0, ldb_pad=0, a_off=0, b_off=0,      # operand padding / base offset (elements)
        ldc_pad=0, c_dt=None, c_off=0,               # output: ldc = N + pad, dtype, base offset
        alpha=1.0, beta=0.0, bias=False, bias_off=0, addend=False, act="none", preact=False,
        res=False,
        knobs={},                                    # MMDX_* launch knobs of this run
        families=("int",),                           # int | gauss
        why="")
    c.__dict__.update(kw)
    if c.c_dt is None:
        c.c_dt = dt
    if c.act == "gelu_bwd":
        c.preact = True                              # an input there
    return c


OR = {"kk": (1, 1), "kr": (1, 0), "rr": (0, 0), "rk": (0, 1)}
K256 = {"MMDX_GEMM256_FWD_MIN": 1}
W4 = {"MMDX_GEMM_8W128": 0}
BOTH = ("int", "gauss")


def _build_cases():
    cs = []

    def add(cid, dt, M, N, K, o="kk", **kw):
        ak, bk = OR[o]
        cs.append(make_case(cid, dt, M, N, K, ak, bk, **kw))

    for dt in (BF16, F16):
        t = DT_NAME[dt]
        # ---- 16-bit LDS-DMA paths, 128 x 128 tiles (8 waves), ragged in M and N
        for o in OR:
            fam = BOTH if o in ("kk", "rr") else ("int",)
            add(f"{t}-dma-k72-{o}", dt, 136, 200, 72, o, families=fam,
                why="one K tile + an 8-element tail, ns2")
            add(f"{t}-dma-k328-{o}", dt, 136, 200, 328, o, why="no split, kper 384, ns3",
                families=BOTH if o == "kk" else ("int",))
            add(f"{t}-dma-k520-{o}", dt, 136, 200, 520, o, families=fam,
                why="2 splits, the second 3 tiles + 8")
        add(f"{t}-dma-k776", dt, 136, 200, 776, why="3 splits: the reduce's tail loop only")
        add(f"{t}-dma-k1160", dt, 136, 200, 1160, why="4 splits: one pass of the 4-wide loop")
        add(f"{t}-dma-k1600", dt, 136, 200, 1600, why="25 K tiles: 6 splits asked, 5 granted")
        add(f"{t}-dma-k1736", dt, 136, 200, 1736, families=BOTH, why="7 splits: 4 + 3")
        add(f"{t}-dma-n201", dt, 136, 201, 520, why="DMA main loop, N % 4 = 1: scalar reduce")
        add(f"{t}-dma-n203", dt, 136, 203, 520, families=BOTH,
            why="N % 4 = 3: apply4's partial columns in the partial store, scalar reduce")
        add(f"{t}-dma-n204-split", dt, 136, 204, 520,
            why="EpiPartial::apply8_fast's 4-column tail")
        add(f"{t}-dma-n204", dt, 136, 204, 72, ldc_pad=4,
            why="EpiStore::apply8_fast's 4-column tail (ldc 208)")
        add(f"{t}-dma-n203-ldc208", dt, 136, 203, 72, ldc_pad=5,
            why="apply8_fast's tail with 3 live columns: per element")
        add(f"{t}-dma-k520-novec", dt, 136, 200, 520, knobs={"MMDX_SPLITK_VEC": 0},
            why="MMDX_SPLITK_VEC=0: the scalar reduce at N % 4 == 0")
        # ---- 64-wide tiles: always the 4-wave kernel
        for M, N in ((40, 48), (40, 200), (200, 40)):
            add(f"{t}-t{M}x{N}-k72", dt, M, N, 72, families=BOTH,
                why="64-wide tile, ns2, K tail")
            add(f"{t}-t{M}x{N}-k328", dt, M, N, 328, families=BOTH,
                why="64-wide tile, no split, ns3")
            add(f"{t}-t{M}x{N}-k520", dt, M, N, 520, families=BOTH,
                why="64-wide tile, split, ns3")
        add(f"{t}-t64x64", dt, 64, 64, 72, why="M = N = 64 exactly: the last 64 x 64 shape")
        add(f"{t}-t65x65", dt, 65, 65, 72, why="M = N = 65: the first 128 x 128 shape")
        add(f"{t}-t40x48-rr", dt, 40, 48, 72, "rr", why="64 x 64 tile, R-major DMA")
        # ---- the 128 x 128 tile as 4 waves
        add(f"{t}-w4-k72", dt, 136, 200, 72, knobs=W4, families=BOTH, why="4-wave 128 x 128, ns2")
        add(f"{t}-w4-k328", dt, 136, 200, 328, knobs=W4, families=BOTH,
            why="4-wave 128 x 128, ns3")
        add(f"{t}-w4-k520", dt, 136, 200, 520, knobs=W4, families=BOTH,
            why="4-wave 128 x 128, split")
        add(f"{t}-w4-k520-rr", dt, 136, 200, 520, "rr", knobs=W4, why="4-wave, R-major")
        # ---- 256 x 256 forward kernel
        add(f"{t}-256-k136", dt, 300, 260, 136, knobs=K256, families=BOTH,
            why="256 x 256, ragged M and N, K tail 8")
        add(f"{t}-256-k128", dt, 300, 260, 128, knobs=K256, res=True, ldc_pad=4,
            why="the K >= 128 boundary; residual (ldc 264: the 16-B epilogue)")
        add(f"{t}-256-k120", dt, 300, 260, 120, knobs=K256,
            why="K < 128: must fall to the 128 x 128 kernel")
        add(f"{t}-256-n513", dt, 257, 513, 200, knobs=K256, why="one row / column past 256 / 512")
        add(f"{t}-256-gelu", dt, 300, 260, 136, knobs=K256, bias=True, act="gelu", preact=True,
            ldc_pad=4, families=("gauss",), why="256 x 256 with bias + GELU + preact")
        # ---- padded leading dimensions, NaN in every padding element
        for o in ("kk", "rr"):
            add(f"{t}-pad-k72-{o}", dt, 136, 200, 72, o, lda_pad=8, ldb_pad=8, ldc_pad=8,
                why="lda / ldb / ldc + 8: still DMA")
        add(f"{t}-pad-k520", dt, 136, 200, 520, lda_pad=8, ldb_pad=8, ldc_pad=8,
            why="padded, split")
        add(f"{t}-pad-256", dt, 300, 260, 136, lda_pad=8, ldb_pad=8, ldc_pad=12, knobs=K256,
            why="padded, 256 x 256")
        # ---- 16-bit kload paths
        add(f"{t}-kl-k75", dt, 136, 200, 75, families=BOTH, why="k-major K % 8 = 3, vec false")
        add(f"{t}-kl-k13", dt, 136, 200, 13, why="K < one vector past the first")
        add(f"{t}-kl-k76-vec", dt, 136, 200, 76, lda_pad=4, ldb_pad=4,
            why="aligned (ld 80): the vector path, one vector crossing klim")
        add(f"{t}-kl-k523", dt, 136, 200, 523, families=BOTH, why="split-K on kload")
        add(f"{t}-kl-k523-vec", dt, 136, 200, 523, lda_pad=5, ldb_pad=5,
            why="split-K on kload, vector loads (ld 528)")
        add(f"{t}-kl-k523-n201", dt, 136, 201, 523, why="split-K on kload, scalar reduce")
        add(f"{t}-kl-rr", dt, 130, 202, 72, "rr", why="R-major rows % 8 != 0, vec false")
        add(f"{t}-kl-rr-vec", dt, 130, 202, 72, "rr", lda_pad=6, ldb_pad=6,
            why="R-major rows % 8 != 0, vector loads up to the last whole vector")
        add(f"{t}-kl-lda1", dt, 136, 200, 72, lda_pad=1, why="lda = K + 1 alone decides")
        add(f"{t}-kl-aoff", dt, 136, 200, 72, a_off=1,
            why="A's base one element off 16 B at K % 8 == 0: vec == false alone decides")
        add(f"{t}-kl-boff-rr", dt, 136, 200, 72, "rr", b_off=3, why="B's base off, R-major")
        add(f"{t}-kl-t40x48", dt, 40, 48, 75, families=BOTH, why="kload 64 x 64")
        add(f"{t}-kl-t40x200", dt, 40, 200, 75, families=BOTH, why="kload 64 x 128")
        add(f"{t}-kl-t200x40", dt, 200, 40, 75, families=BOTH, why="kload 128 x 64")
        # ---- epilogues on five bases
        # (M, N, K, knobs, ldc - N: 264 lets the 256 x 256 kernel's N = 260 take 16-B stores)
        bases = {"dma": (136, 200, 72, {}, 0), "r4": (136, 200, 520, {}, 0),
                 "r1": (136, 201, 520, {}, 0), "256": (300, 260, 136, K256, 4),
                 "kl": (136, 200, 75, {}, 0)}
        for b, (M, N, K, kn, pad) in bases.items():
            def e(tag, ldc_pad=0, **kw):
                add(f"{t}-epi-{b}-{tag}", dt, M, N, K, knobs=kn,
                    ldc_pad=ldc_pad if ldc_pad == 1 else pad + ldc_pad, **kw)
            e("a05", alpha=0.5, why="alpha 0.5: half-integers")
            e("a2", alpha=2.0, why="alpha 2")
            e("ba", bias=True, addend=True, why="bias + addend")
            e("b1", beta=1.0, why="beta 1 on a preset C")
            e("res", res=True, why="residual")
            e("relu", act="relu", why="ReLU")
            e("pre", preact=True, why="pre-activation copy")
            allk = dict(alpha=2.0, bias=True, addend=True, act="relu", preact=True, beta=1.0,
                        res=True)
            e("all", why="every epilogue input at once", **allk)
            e("all-f32", c_dt=F32, why="... into an fp32 C", **allk)
            e("f32", c_dt=F32, why="fp32 C, plain")
            e("all-ldc8", ldc_pad=8, why="ldc = N + 8", **allk)
            e("all-ldc1", ldc_pad=1, why="ldc = N + 1: per element", **allk)
            e("ldc1", ldc_pad=1, why="ldc = N + 1, plain: apply4's row-wise choice")
            e("gelu", bias=True, act="gelu", preact=True, families=("gauss",), why="GELU")
            e("gelu-f32", bias=True, act="gelu", preact=True, c_dt=F32, families=("gauss",),
              why="GELU, fp32 C")
            e("gbwd", act="gelu_bwd", families=("gauss",), why="GELU backward, vector branch")
            e("gbwd-b", act="gelu_bwd", beta=1.0, families=("gauss",), why="... + beta C")
            e("gbwd-ba", act="gelu_bwd", bias=True, addend=True, families=("gauss",),
              why="GELU backward + bias + addend: per element")
        add(f"{t}-epi-dma-biasoff", dt, 136, 200, 72, bias=True, bias_off=1,
            why="bias at + 4 bytes: vec8_ok() must say no")
        add(f"{t}-epi-256-biasoff", dt, 300, 260, 136, knobs=K256, bias=True, bias_off=1,
            ldc_pad=4,
            why="the same on the 256 x 256 kernel")
        add(f"{t}-epi-dma-c16", dt, 136, 200, 72, c_dt=F32, c_off=4,
            why="fp32 C 16-B but not 32-B aligned under the 2 x 16-B stores")
        # ---- mmdx_gemm_bias_grad (A = dY^T [K][lda], B = X [K][ldb], both R-major)
        for M, N, K in ((136, 72, 520), (136, 64, 520), (264, 136, 1736)):
            s = f"{t}-wb-{M}x{N}"
            add(s, dt, M, N, K, "rr", kind="wb", c_dt=F32, families=BOTH,
                why="fused, ragged second row tile")
            add(s + "-c16", dt, M, N, K, "rr", kind="wb", why="fused, 16-bit dW")
            add(s + "-lda", dt, M, N, K, "rr", kind="wb", c_dt=F32, lda_pad=8,
                why="fused with lda = M + 8")
            add(s + "-w4", dt, M, N, K, "rr", kind="wb", c_dt=F32, knobs=W4, families=BOTH,
                why="fused on the 4-wave kernel")
        add(f"{t}-wb-k72", dt, 136, 72, 72, "rr", kind="wb", c_dt=F32, families=BOTH,
            why="unfused: no split")
        add(f"{t}-wb-m132", dt, 132, 72, 520, "rr", kind="wb", c_dt=F32, families=BOTH,
            why="unfused: M % 8")
        add(f"{t}-wb-off", dt, 136, 72, 520, "rr", kind="wb", c_dt=F32,
            knobs={"MMDX_WGRAD_BIAS_FUSED": 0}, families=BOTH, why="unfused by the knob")
        # ---- mmdx_bias_grad's GEMM form: db[N] = column sums of dy [M rows][N]
        for beta in (0.0, 1.0):
            for M, N in ((520, 72), (8, 8)):
                add(f"{t}-bg-{M}x{N}-b{int(beta)}", dt, M, N, 1, kind="bg", beta=beta,
                    knobs={"MMDX_BIAS_GRAD_GEMM": 1}, families=BOTH if M == 520 else ("int",),
                    why="1 x N x M GEMM against a ones row")

    # ---- fp32 compute (vector 4, BK 32, kload only)
    add("f32-k70", F32, 136, 200, 70, families=BOTH, why="K % 4 = 2 tail, ld 70: vec false")
    add("f32-k70-vec", F32, 136, 200, 70, lda_pad=2, ldb_pad=2, why="... with ld 72: vectors")
    add("f32-k300", F32, 136, 200, 300, families=BOTH, why="2 splits of 5 K tiles")
    add("f32-k300-n201", F32, 136, 201, 300, why="2 splits, scalar reduce")
    add("f32-t40x48", F32, 40, 48, 33, families=BOTH, why="64 x 64 tile, one element past a K tile")
    add("f32-k70-rr", F32, 136, 200, 70, "rr", families=BOTH, why="R-major")
    add("f32-k70-kr", F32, 136, 200, 70, "kr", why="mixed orientation")
    add("f32-all", F32, 136, 200, 70, alpha=2.0, bias=True, addend=True, act="relu",
        preact=True, beta=1.0, res=True, why="every epilogue input at once")
    add("f32-a05", F32, 136, 200, 300, alpha=0.5, why="alpha through the reduce")
    add("f32-gelu", F32, 136, 200, 70, bias=True, act="gelu", preact=True, families=("gauss",),
        why="GELU")
    add("f32-gbwd", F32, 136, 200, 70, act="gelu_bwd", families=("gauss",), why="GELU backward")
    add("f32-wb", F32, 136, 72, 300, "rr", kind="wb", families=BOTH, why="unfused: fp32")
    return cs


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case id"


def shapes(c):
    """(M, N, K, ak, bk) of the GEMM a case launches: bias-grad cases run 1 x N x rows against a
    ones row (k-major) with dy R-major."""
    if c.kind == "bg":
        return 1, c.N, c.M, 1, 0
    return c.M, c.N, c.K, c.ak, c.bk


def leading_dims(c):
    """(lda, ldb, ldc) in elements."""
    M, N, K, ak, bk = shapes(c)
    return (K if ak else M) + c.lda_pad, (K if bk else N) + c.ldb_pad, N + c.ldc_pad


def case_seed(c, family):
    """Deterministic per case and family."""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c.id)) % 100003 + \
        (0 if family == "int" else 500000)


# ----------------------------------------------------------------------- the dispatcher mirror
_KNOBS = {"MMDX_SPLITK_TARGET": 256, "MMDX_SPLITK_VEC": 1, "MMDX_GEMM256_FWD_MIN": 90,
          "MMDX_GEMM_8W128": 1, "MMDX_WGRAD_BIAS_FUSED": 1, "MMDX_BIAS_GRAD_GEMM": 0}
KNOB_NAMES = sorted(_KNOBS)


def _cdiv(a, b):
    return (a + b - 1) // b


def plan_dense(dt, M, N, K, kn):
    """gemm_dense.h plan_dense: tile, splits asked for (after the K-tile cap), splits granted,
    K extent per split."""
    bk = BK[dt]
    bm = 64 if M <= 64 else 128
    bn = 64 if N <= 64 else 128
    tiles = _cdiv(M, bm) * _cdiv(N, bn)
    ktiles = _cdiv(K, bk)
    s = 1
    if tiles < 256 and ktiles >= 8:
        s = max(1, min(_cdiv(kn["MMDX_SPLITK_TARGET"], tiles), ktiles // 4))
    kper = _cdiv(ktiles, s) * bk
    return SimpleNamespace(bm=bm, bn=bn, asked=s, splits=max(1, _cdiv(K, kper)), kper=kper,
                           tiles=tiles, ktiles=ktiles)


def dense_path(dt, p, M, N, K, lda, ak, a_low4, ldb, bk, b_low4, bias_sum, kn):
    """gemm_dense.h dense_path: (family, bm, bn, ns, va, vb)."""
    vec = 16 // ESIZE[dt]
    va = lda % vec == 0 and a_low4 % 16 == 0
    vb = ldb % vec == 0 and b_low4 % 16 == 0
    out = SimpleNamespace(family="kload", bm=p.bm, bn=p.bn, ns=2, va=va, vb=vb)
    if ESIZE[dt] != 2:
        return out
    abytes = (M if ak else K) * lda * 2
    bbytes = (N if bk else K) * ldb * 2
    oka = va and (K % 8 == 0 if ak else M % 8 == 0) and abytes < 1 << 31
    okb = vb and (K % 8 == 0 if bk else N % 8 == 0) and bbytes < 1 << 31
    if not (oka and okb):
        return out
    if p.bm == 128 and p.bn == 128 and ak and bk and not bias_sum:
        t256 = _cdiv(M, 256) * _cdiv(N, 256)
        lim = kn["MMDX_GEMM256_FWD_MIN"]
        if p.splits == 1 and lim > 0 and t256 >= lim and K >= 128:
            out.family, out.bm, out.bn = "dma8", 256, 256
            return out
    out.family = "dma8" if p.bm == 128 and p.bn == 128 and kn["MMDX_GEMM_8W128"] else "dma4"
    if p.tiles * p.splits <= 256 and p.kper >= 256:
        out.ns = 3
    return out


def _wb_fused(dt, p, M, N, K, lda, a_low4, ldb, b_low4, kn):
    """gemm_dense.hip wgrad_bias_fused."""
    return bool(kn["MMDX_WGRAD_BIAS_FUSED"] and dt != F32 and p.splits > 1 and p.bm == 128
                and M % 8 == 0 and N % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0
                and a_low4 % 16 == 0 and b_low4 % 16 == 0
                and K * lda * 2 < 1 << 31 and K * ldb * 2 < 1 << 31)


def _plain(c):
    return not (c.bias or c.addend or c.preact or c.res or c.act != "none")


def vec8_ok(c):
    """EpiStore<OutT, true>::vec8_ok() for the pointers the tests pass: C at c_off elements and
    the bias at bias_off floats past a 16-B aligned base, everything else aligned."""
    ldc = leading_dims(c)[2]
    if ldc % 8 or (c.c_off * ESIZE[c.c_dt]) % 16:
        return False
    if c.bias and (c.bias_off * 4) % 16:
        return False
    if c.act == "gelu_bwd":
        return not (c.res or c.bias or c.addend)
    return True


def _apply4_kind(c):
    """EpiStore::apply4: 4-wide stores for a plain epilogue where m * ldc + n is a multiple of
    4 (every row at ldc % 4 == 0, else every fourth), per element otherwise."""
    if not _plain(c):
        return "elem"
    return "vec4" if leading_dims(c)[2] % 4 == 0 else "vec4+elem"


def expected_path(c, knobs=None):
    """The path the dense dispatcher takes for case c under its knobs (or `knobs`):
      desc     mmdx_gemm_describe's string, [wb-fused/ | wb-unfused/]<family>/<bm>x<bn>/ns<stages>
               /s<splits>/k<kper>
      plan     plan_dense's result (asked / granted splits, kper, K tiles)
      partial  the split-K partial store: p8 (16-B pairs) | p4 | none
      reduce   none | reduce4 | reduce1
      epi      how the EpiStore writes C: vec8 (apply8_fast) | vec4 | vec4+elem | elem
      key      <dtype>:<family>/<tile>/ns<stages>/<one|split>|<partial>><reduce>|<epi>
    Operand base addresses are 16-B aligned plus a_off / b_off elements."""
    kn = dict(_KNOBS)
    kn.update(c.knobs if knobs is None else knobs)
    M, N, K, ak, bk = shapes(c)
    lda, ldb, _ = leading_dims(c)
    a4, b4 = (c.a_off * ESIZE[c.dt]) % 16, (c.b_off * ESIZE[c.dt]) % 16
    p = plan_dense(c.dt, M, N, K, kn)
    out = SimpleNamespace(plan=p, splits=p.splits, fused=False, prefix="")
    if c.kind == "wb":
        out.fused = _wb_fused(c.dt, p, M, N, K, lda, a4, ldb, b4, kn)
        out.prefix = "wb-fused/" if out.fused else "wb-unfused/"
    d = dense_path(c.dt, p, M, N, K, lda, ak, a4, ldb, bk, b4, out.fused, kn)
    out.path = d
    out.desc = f"{out.prefix}{d.family}/{d.bm}x{d.bn}/ns{d.ns}/s{p.splits}/k{p.kper}"
    if p.splits == 1:
        out.partial, out.reduce = "none", "none"
        out.epi = "vec8" if d.family != "kload" and vec8_ok(c) else _apply4_kind(c)
    else:
        out.partial = "p8" if d.family != "kload" and N % 4 == 0 else "p4"
        vec = out.fused or (kn["MMDX_SPLITK_VEC"] and N % 4 == 0 and M * N < 1 << 31)
        out.reduce = "reduce4" if vec else "reduce1"
        out.epi = _apply4_kind(c) if vec else "elem"
    out.key = (f"{DT_NAME[c.dt]}:{out.prefix}{d.family}/{d.bm}x{d.bn}/ns{d.ns}/"
               f"{'one' if p.splits == 1 else 'split'}|{out.partial}>{out.reduce}|{out.epi}")
    return out


def describe(lib, c, a_low4=None, b_low4=None):
    """mmdx_gemm_describe for case c (under the knobs the library currently holds)."""
    import ctypes
    M, N, K, ak, bk = shapes(c)
    lda, ldb, _ = leading_dims(c)
    a4 = (c.a_off * ESIZE[c.dt]) % 16 if a_low4 is None else a_low4
    b4 = (c.b_off * ESIZE[c.dt]) % 16 if b_low4 is None else b_low4
    buf = ctypes.create_string_buffer(96)
    code = {F32: 0, BF16: 1, F16: 2}[c.dt]
    rc = lib.mmdx_gemm_describe(code, M, N, K, lda, ak, a4, ldb, bk, b4, int(c.kind == "wb"),
                                buf, len(buf))
    assert rc == 0, lib.mmdx_last_error()
    return buf.value.decode()


# -------------------------------------------------------------------------------- host data
def host(c, family):
    """Operands, epilogue inputs and fp64 references of one case: values the compute dtype (and,
    for C0 / residual / preact input, the output dtype) holds exactly."""
    g = torch.Generator().manual_seed(case_seed(c, family))
    h = SimpleNamespace(c=c, family=family)
    M, N, K = c.M, c.N, c.K
    integer = family == "int"

    def gen(shape, dt, scale=1.0):
        return gen_integer(shape, g) if integer else gen_gaussian(shape, g, dt, scale)

    if c.kind == "bg":
        h.dy = gen((M, N), c.dt)
        h.db0 = gen((N,), F32)
        r = ref_wgrad_bias(h.dy, torch.zeros(M, 1))
        h.db = r.db + c.beta * h.db0
        h.db_terms = r.db_terms + (c.beta * h.db0).abs()
        h.n_terms = M + 1
        return h
    if c.kind == "wb":
        h.dY, h.X = gen((K, M), c.dt, 0.25), gen((K, N), c.dt, 0.25)
        h.r = ref_wgrad_bias(h.dY, h.X)
        h.n_terms = K
        return h
    h.A, h.B = gen((M, K), c.dt), gen((N, K), c.dt, 1.0 if integer else 0.125)
    h.bias = gen((N,), F32) if c.bias else None
    h.addend = gen((M, N), F32) if c.addend else None
    h.C0 = gen((M, N), c.c_dt) if c.beta != 0.0 else None
    h.res = gen((M, N), c.c_dt) if c.res else None
    h.pre_in = gen_gaussian((M, N), g, c.c_dt) if c.act == "gelu_bwd" else None
    h.r = ref_gemm(h.A, h.B, c.alpha, h.bias, h.addend, c.act, c.beta, h.C0, h.res, h.pre_in)
    h.n_terms = K + 4
    return h


def exact_preconditions(h):
    """From the reference alone, before any launch: operands in {-1, 0, 1}; every value that is
    stored (pre-activation copy, C, dW) a multiple of the case's step the stored dtype holds;
    fewer than 2^24 terms."""
    c = h.c
    ops = [t for t in (getattr(h, n, None) for n in
                       ("A", "B", "bias", "addend", "C0", "res", "dY", "X", "dy", "db0"))
           if t is not None]
    for t in ops:
        assert set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
    if c.kind == "bg":
        check_exact_preconditions(h.db, h.n_terms, F32, f"{c.id}: db")
    elif c.kind == "wb":
        check_exact_preconditions(h.r.dW, h.n_terms, c.c_dt, f"{c.id}: dW")
        check_exact_preconditions(h.r.db, h.n_terms, F32, f"{c.id}: db")
    else:
        step = 0.5 if c.alpha == 0.5 else 1.0
        check_exact_preconditions(h.r.z, h.n_terms, c.c_dt, f"{c.id}: preact", step)
        check_exact_preconditions(h.r.y, h.n_terms, c.c_dt, f"{c.id}: C", step)


def assert_bounded(kind, got, ref, abs_terms, dt_stored, what, extra=None, acc_scale=1.0):
    """|got - ref| <= h_T |ref| + ACC * sum |terms| (+ extra), element by element; prints
    'gemmref <kind> <error / bound>' first and returns the ratio."""
    bound = H_T[dt_stored] * ref.abs() + ACC * acc_scale * abs_terms
    if extra is not None:
        bound = bound + extra
    ratio = bound_ratio(got, ref, bound)
    print(f"gemmref {kind} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{what}: {kind} error / bound = {ratio:.3f}"
    return ratio
