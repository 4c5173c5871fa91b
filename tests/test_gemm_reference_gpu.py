"""The dense GEMM entry points of csrc/gemm_dense.hip (mmdx_gemm, mmdx_gemm_res,
mmdx_gemm_bias_grad, mmdx_bias_grad's GEMM form) against the fp64 reference of tests/gemm_ref.py,
element by element, at the smallest shapes that reach each path of the dispatcher: ragged
128 x 128 / 64-wide / 256 x 256 tiles, K tails of 8 elements and of less than a vector, 2 to 7
splits through both reduce kernels, padded and misaligned operands, every epilogue input, the
fused weight + bias gradient (tests/test_gemm_ref_cpu.py asserts which case reaches which path,
and that the mirror equals mmdx_gemm_describe; every launch here asks the library again with
the pointers it really passes).

Two operand families:
  * integer: A, B, bias, addend, C0 and the residual in {-1, 0, 1}, alpha in {0.5, 1, 2}.  Every
    product and partial sum is a small (half-)integer that an fp32 accumulator holds exactly in
    any K-tile order or split grouping, so C, the pre-activation copy, dW and db must EQUAL the
    reference.  The preconditions are asserted from the reference before any launch.  Outputs
    are preset to NaN (to a sentinel around a beta = 1 C); operand padding is NaN; padding
    columns, the elements in front of an offset base, guard elements behind every output, db's
    neighbours and the floats behind a workspace of exactly the queried size must be untouched,
    bit for bit, and every input unchanged.
  * Gaussian (one case per kernel path, every GELU / GELU-backward case): per element
    |got - ref| <= h_T |ref| + 2e-5 sum |terms|, the reference on operands already rounded to
    the compute dtype, h_T of the stored type.  GELU: the pre-activation copy has its own h_T;
    the output's accumulation term is scaled by GELU's Lipschitz constant 1.13 (nothing is
    added for the fp32 erf: 2e-5 of the terms is hundreds of its ulps).
    GELU backward adds an allowance for the device's fp32 erf / exp in gelu' = 0.5 + 0.5 erf +
    x pdf: the smaller of GELU_BWD_ULPS * 2^-24 |alpha acc gelu'| and GELU_BWD_TERM_ULPS *
    2^-24 |alpha acc| (0.5 + 0.5 |erf| + |x| pdf).  The three terms of gelu' cancel in the left
    tail and at gelu's minimum (x = -0.7518), where an error of a few 2^-24 of the terms is any
    multiple of gelu' itself: against |gelu'| the Gaussian cases need up to 38764 (f16-epi-dma-
    gbwd; 17026 f16-epi-kl-gbwd, 8644 f32-gbwd, 0 elsewhere), against the terms up to 2.70, and
    test_gelu_bwd_erf_allowance (integer operands: an exact accumulator, so the whole error is
    gelu' and one product rounding) measures 2.38 to 2.76.  Both constants are twice the
    largest seen; the minimum of the two is never wider than the first alone.
Every bounded check prints "gemmref <kind> <error / bound>" before it asserts.

Measured on an MI355X: every integer-family comparison is an equality in all 304 cases, and
the largest error / bound per kind is gemm 0.972, preact 0.978, gelu 0.972, gelu-bwd 0.988,
dW 0.006, db 0.001, bias-grad 0.0004 (the 16-bit ratios are the store's rounding: half an ulp
just above a power of two is h_T |ref|; GELU into an fp32 C reaches 0.002 to 0.005 with
16-bit operands and 0.012 in fp32, under the Lipschitz-scaled accumulation term alone).  The
kernels needed no fix.  The checks do bite; each of these libraries, which only do less work,
fails exactly the cases that run the broken code:
  * splitk_reduce4_kernel without its tail loop: every reduce4 case with 2, 3, 5 or 7 splits
    (dma-k520-*, -k776, -k1600, -k1736, -n204-split, t*-k520, w4-k520*, pad-k520, kl-k523,
    kl-k523-vec, epi-r4-*, every wb-* case that splits (dW and db), bg-520x72-*, f32-k300,
    f32-a05, f32-wb), in both families; dma-k1160 (4 splits) and the reduce1 cases pass.
  * kend rounded down to a multiple of 8 in igemm_kernel: every kload case with K % 8 != 0
    (kl-k75, -k13, -k76-vec, -k523*, kl-t*, epi-kl-*, every f32 case); kl-lda1, kl-aoff,
    kl-boff-rr and kl-rr* (K = 72) pass.
  * EpiStore::apply8_fast ignoring alpha: epi-dma-a05, -a2, -all, -all-f32, -all-ldc8 and the
    same five on the 256 x 256 kernel; the per-element and split cases pass.
  * the fused bias sum skipping the last K tile: every fused wb-* case (db only), in both
    families; the unfused ones pass.
"""
import pytest
import torch

import gemm_ref as R
import mmdx._lib as L
from gemm_ref import F32, NAN

pytestmark = pytest.mark.gpu

GELU_BWD_ULPS = 2 * 38763.65    # x 2^-24 |alpha acc gelu'|
GELU_BWD_TERM_ULPS = 2 * 2.76   # x 2^-24 |alpha acc| (0.5 + 0.5 |erf| + |x| pdf)
SENT = -7.0           # around a beta = 1 C, around db
WS_SENT = 3.0         # behind the workspace

INT_CASES = [c.id for c in R.CASES if "int" in c.families]
GAUSS_CASES = [c.id for c in R.CASES if "gauss" in c.families]
ACT = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "gelu": L.ACT_GELU, "gelu_bwd": L.ACT_GELU_BWD}


def _set_knobs(knobs, c):
    for name in R.KNOB_NAMES:
        knobs(name, c.knobs.get(name))


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _outside_same(after, before, shape, ld, off):
    """Everything of a matrix() buffer but its [M, N] block is bit for bit what it was."""
    a, b = after.cpu().clone(), before.clone()
    for t in (a, b):
        R.view(t, shape, ld, off)[:, :shape[1]] = 0
    return _same_bits(a, b)


class _Out:
    """A device matrix() buffer with the host copy of its preset."""

    def __init__(self, dev, shape, ld, off, dt, fill, mat=None):
        self.shape, self.ld, self.off = shape, ld, off
        self.before = R.matrix(shape, ld, off, dt, fill, mat)
        self.dev = self.before.to(dev)
        self.ptr = self.dev.data_ptr() + off * self.before.element_size()

    def block(self):
        return R.view(self.dev.cpu(), self.shape, self.ld, self.off)[:, :self.shape[1]].double()

    def check_outside(self, what):
        assert _outside_same(self.dev, self.before, self.shape, self.ld, self.off), \
            f"{what}: written outside its [M, N] block"

    def check_unchanged(self, what):
        assert _same_bits(self.dev, self.before), f"{what}: changed"


class _Ws:
    def __init__(self, dev, nbytes):
        self.n = nbytes
        self.dev = torch.full((nbytes // 4 + 64,), WS_SENT, device=dev)

    def check_guard(self, what, whole=False):
        tail = self.dev if whole else self.dev[self.n // 4:]
        assert (tail == WS_SENT).all(), f"{what}: written behind the workspace"


def _operand(dev, mat, kmajor, ld_pad, off, dt):
    buf, ld = R.store(mat, kmajor, ld_pad, off, dt)
    d = buf.to(dev)
    return buf, d, d.data_ptr() + off * buf.element_size(), ld


def _gemm(dev, c, h, ws_short=0):
    """Launches case c on the data h; checks everything that must stay untouched; returns
    (rc, C [M, N] fp64, preact [M, N] fp64 or None); all None after an error."""
    M, N, K = c.M, c.N, c.K
    _, _, ldc = R.leading_dims(c)
    lib = L.lib()
    a0, ad, ap, lda = _operand(dev, h.A, c.ak, c.lda_pad, c.a_off, c.dt)
    b0, bd, bp, ldb = _operand(dev, h.B, c.bk, c.ldb_pad, c.b_off, c.dt)
    what = c.id
    assert R.describe(lib, c, ap & 15, bp & 15) == R.expected_path(c).desc, \
        f"{what}: the library takes another path than the case table expects"
    C = _Out(dev, (M, N), ldc, c.c_off, c.c_dt, SENT if c.beta != 0.0 else NAN, h.C0)
    pre = None
    if c.act == "gelu_bwd":
        pre = _Out(dev, (M, N), ldc, 0, c.c_dt, NAN, h.pre_in)
    elif c.preact:
        pre = _Out(dev, (M, N), ldc, 0, c.c_dt, NAN)
    add = _Out(dev, (M, N), ldc, 0, F32, NAN, h.addend) if c.addend else None
    res = _Out(dev, (M, N), ldc, 0, c.c_dt, NAN, h.res) if c.res else None
    bias = bias0 = None
    if c.bias:
        bias0 = torch.full((c.bias_off + N,), NAN)
        bias0[c.bias_off:] = h.bias.float()
        bias = bias0.to(dev)
    n = lib.mmdx_gemm_workspace_size(L.dtype_code(c.dt), M, N, K)
    assert n == (R.expected_path(c).splits > 1) * R.expected_path(c).splits * 4 * M * N
    ws = _Ws(dev, n)
    args = [L.dtype_code(c.dt), M, N, K, ap, lda, c.ak, bp, ldb, c.bk, C.ptr, ldc,
            L.dtype_code(c.c_dt), bias.data_ptr() + 4 * c.bias_off if c.bias else None,
            add.ptr if add else None, ACT[c.act], c.alpha, c.beta, pre.ptr if pre else None]
    tail = [ws.dev.data_ptr(), n - ws_short, L.stream()]
    if c.res:
        rc = lib.mmdx_gemm_res(*args, res.ptr, *tail)
    else:
        rc = lib.mmdx_gemm(*args, *tail)
    torch.cuda.synchronize()
    ws.check_guard(what, whole=rc != 0)
    assert _same_bits(ad, a0) and _same_bits(bd, b0), f"{what}: an operand changed"
    for t, name in ((add, "addend"), (res, "residual")):
        if t:
            t.check_unchanged(f"{what}: {name}")
    if bias is not None:
        assert _same_bits(bias, bias0), f"{what}: bias changed"
    if rc != 0:
        C.check_unchanged(f"{what}: C after an error")
        if pre:
            pre.check_unchanged(f"{what}: preact after an error")
        return rc, None, None
    C.check_outside(f"{what}: C")
    pz = None
    if c.act == "gelu_bwd":
        pre.check_unchanged(f"{what}: the pre-activation input")
    elif pre:
        pre.check_outside(f"{what}: preact")
        pz = pre.block()
    return rc, C.block(), pz


def _wgrad_bias(dev, c, h, ws_short=0):
    """mmdx_gemm_bias_grad on case c: (rc, dW, db)."""
    M, N, K = c.M, c.N, c.K
    lib = L.lib()
    a0, ad, ap, lda = _operand(dev, h.dY.T, 0, c.lda_pad, 0, c.dt)
    b0, bd, bp, ldb = _operand(dev, h.X.T, 0, c.ldb_pad, 0, c.dt)
    e = R.expected_path(c)
    assert R.describe(lib, c, ap & 15, bp & 15) == e.desc, f"{c.id}: path"
    ldc = N + c.ldc_pad
    dW = _Out(dev, (M, N), ldc, 0, c.c_dt, NAN)
    db0 = torch.full((8 + M + 8,), SENT)
    db0[8:8 + M] = NAN
    db = db0.to(dev)
    n = lib.mmdx_gemm_bias_grad_workspace_size(L.dtype_code(c.dt), M, N, K)
    ws = _Ws(dev, n)
    rc = lib.mmdx_gemm_bias_grad(L.dtype_code(c.dt), M, N, K, ap, lda, bp, ldb, dW.ptr, ldc,
                                 L.dtype_code(c.c_dt), db.data_ptr() + 32, ws.dev.data_ptr(),
                                 n - ws_short, L.stream())
    torch.cuda.synchronize()
    ws.check_guard(c.id, whole=rc != 0)
    assert _same_bits(ad, a0) and _same_bits(bd, b0), f"{c.id}: an operand changed"
    if rc != 0:
        dW.check_unchanged(f"{c.id}: dW after an error")
        assert _same_bits(db, db0), f"{c.id}: db after an error"
        return rc, None, None
    dW.check_outside(f"{c.id}: dW")
    got = db.cpu()
    assert (got[:8] == SENT).all() and (got[8 + M:] == SENT).all(), f"{c.id}: db's neighbours"
    return rc, dW.block(), got[8:8 + M].double()


def _bias_grad(dev, c, h):
    """mmdx_bias_grad on dy [M rows][N] under MMDX_BIAS_GRAD_GEMM=1: db [N] fp64."""
    M, N = c.M, c.N
    lib = L.lib()
    dy0 = h.dy.to(c.dt).contiguous()
    dy = dy0.to(dev)
    db0 = torch.full((8 + N + 8,), SENT)
    db0[8:8 + N] = h.db0.float() if c.beta != 0.0 else NAN
    db = db0.to(dev)
    n = lib.mmdx_bias_grad_workspace_size(M, N)
    ws = _Ws(dev, n)
    L.call("mmdx_bias_grad", L.dtype_code(c.dt), dy.data_ptr(), M, N, db.data_ptr() + 32, c.beta,
           ws.dev.data_ptr(), n, L.stream())
    torch.cuda.synchronize()
    ws.check_guard(c.id)
    # the GEMM form keeps its ones row (M elements of the compute dtype) at the front of the
    # workspace; the column-sum kernels it would otherwise fall back to silently put fp32
    # partial sums there
    assert (ws.dev.view(c.dt)[:M] == 1).all(), f"{c.id}: the GEMM form did not run"
    assert _same_bits(dy, dy0), f"{c.id}: dy changed"
    got = db.cpu()
    assert (got[:8] == SENT).all() and (got[8 + N:] == SENT).all(), f"{c.id}: db's neighbours"
    return got[8:8 + N].double()


# ============================================================================ integer family
@pytest.mark.parametrize("cid", INT_CASES)
def test_gemm_exact(dev, knobs, cid):
    """Integer operands: C, the pre-activation copy, dW and db equal the fp64 reference."""
    c = R.BY_ID[cid]
    h = R.host(c, "int")
    R.exact_preconditions(h)
    _set_knobs(knobs, c)
    if c.kind == "bg":
        R.assert_exact(_bias_grad(dev, c, h), h.db, f"{cid}: db")
    elif c.kind == "wb":
        rc, dW, db = _wgrad_bias(dev, c, h)
        assert rc == 0, L.lib().mmdx_last_error()
        R.assert_exact(dW, h.r.dW, f"{cid}: dW")
        R.assert_exact(db, h.r.db, f"{cid}: db")
    else:
        rc, C, pre = _gemm(dev, c, h)
        assert rc == 0, L.lib().mmdx_last_error()
        R.assert_exact(C, h.r.y, f"{cid}: C")
        if pre is not None:
            R.assert_exact(pre, h.r.z, f"{cid}: preact")


# =========================================================================== Gaussian family
@pytest.mark.parametrize("cid", GAUSS_CASES)
def test_gemm_gaussian(dev, knobs, cid):
    """Gaussian operands: fp32 accumulation and one rounding per stored value."""
    c = R.BY_ID[cid]
    h = R.host(c, "gauss")
    _set_knobs(knobs, c)
    if c.kind == "bg":
        R.assert_bounded("bg", _bias_grad(dev, c, h), h.db, h.db_terms, F32, cid)
        return
    if c.kind == "wb":
        rc, dW, db = _wgrad_bias(dev, c, h)
        assert rc == 0, L.lib().mmdx_last_error()
        R.assert_bounded("dW", dW, h.r.dW, h.r.dW_terms, c.c_dt, cid)
        R.assert_bounded("db", db, h.r.db, h.r.db_terms, F32, cid)
        return
    rc, C, pre = _gemm(dev, c, h)
    assert rc == 0, L.lib().mmdx_last_error()
    extra = None
    if c.act == "gelu_bwd":
        unit = 2.0 ** -24 * (c.alpha * h.r.acc).abs()
        lit, trm = unit * h.r.g.abs(), unit * R.gelu_grad_terms(h.pre_in.double())
        over = ((C - h.r.y).abs() - R.H_T[c.c_dt] * h.r.y.abs() - R.ACC * h.r.y_terms).clamp(min=0)
        live = (over > 0) & (lit > 0)
        need = [(over[live] / u[live]).max().item() if live.any() else 0.0 for u in (lit, trm)]
        print(f"gemmref gelu-bwd-needs {need[0]:.2f} {need[1]:.2f} {cid}")
        extra = torch.minimum(GELU_BWD_ULPS * lit, GELU_BWD_TERM_ULPS * trm)
    kind = {"none": "gemm", "relu": "gemm", "gelu": "gelu", "gelu_bwd": "gelu-bwd"}[c.act]
    R.assert_bounded(kind, C, h.r.y, h.r.y_terms, c.c_dt, cid, extra)
    if pre is not None:
        R.assert_bounded("preact", pre, h.r.z, h.r.z_terms, c.c_dt, cid)


@pytest.mark.parametrize("dt", [R.BF16, R.F16, F32], ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("shape", [(136, 200, 72), (136, 200, 520), (136, 201, 520)],
                         ids=["vec8", "reduce4", "reduce1"])
def test_gelu_bwd_erf_allowance(dev, knobs, dt, shape):
    """The device's fp32 gelu' against fp64: integer A and B make alpha * acc exact, the output
    is fp32, so |got - ref| / (2^-24 |acc| (0.5 + 0.5 |erf| + |x| pdf)) is the error of gelu'
    (plus one product rounding) in units of 2^-24 of the sum of its |terms|.  Prints the largest
    multiple and pins GELU_BWD_TERM_ULPS: it stays within that constant.  GELU_BWD_ULPS, the
    multiple of |gelu'| itself, is measured by test_gemm_gaussian's "gelu-bwd-needs" lines."""
    M, N, K = shape
    c = R.make_case(f"ulps-{R.DT_NAME[dt]}-{K}-{N}", dt, M, N, K, act="gelu_bwd", c_dt=F32)
    _set_knobs(knobs, c)
    h = R.host(c, "int")
    rc, C, _ = _gemm(dev, c, h)
    assert rc == 0, L.lib().mmdx_last_error()
    unit = 2.0 ** -24 * h.r.acc.abs() * R.gelu_grad_terms(h.pre_in.double())
    live = unit > 0
    assert (C[~live] == 0).all()
    mult = ((C - h.r.y).abs()[live] / unit[live]).max().item()
    print(f"gemmref gelu-bwd-ulps {mult:.2f} {c.id}")
    assert mult <= GELU_BWD_TERM_ULPS, f"{c.id}: gelu' error {mult:.2f} x 2^-24 |acc| sum |terms|"


# =============================================================================== error paths
@pytest.mark.parametrize("dt", [R.BF16, F32], ids=lambda d: R.DT_NAME[d])
def test_unfused_wgrad_rejects_padded_lda(dev, knobs, dt):
    """lda > M is allowed on the fused path only: the unfused one (no split here) returns an
    error, launches nothing and leaves dW, db and the workspace at their presets."""
    c = R.make_case(f"err-lda-{R.DT_NAME[dt]}", dt, 136, 72, 72, 0, 0, kind="wb", c_dt=F32,
                lda_pad=8)
    _set_knobs(knobs, c)
    assert R.expected_path(c).desc.startswith("wb-unfused/")
    rc, _, _ = _wgrad_bias(dev, c, R.host(c, "int"))
    assert rc != 0 and b"lda == M" in L.lib().mmdx_last_error()


@pytest.mark.parametrize("cid", ["bf16-dma-k520-kk", "bf16-kl-k523", "f32-k300", "bf16-wb-136x72"])
def test_workspace_one_byte_short(dev, knobs, cid):
    """A workspace one byte short: an error, nothing launched, outputs at their presets."""
    c = R.BY_ID[cid]
    _set_knobs(knobs, c)
    h = R.host(c, "int")
    if c.kind == "wb":
        rc, _, _ = _wgrad_bias(dev, c, h, ws_short=1)
    else:
        rc, _, _ = _gemm(dev, c, h, ws_short=1)
    assert rc != 0 and b"workspace" in L.lib().mmdx_last_error()
