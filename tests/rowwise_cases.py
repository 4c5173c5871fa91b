"""The case tables, host inputs and error bounds of tests/test_rowwise_reference_gpu.py.  They
live here so that tests/test_rowwise_ref_cpu.py walks exactly the cases the GPU suite runs and
shows, without a GPU, that each is well posed for an fp32 evaluation under the same bounds.

Bounds (TOL is test_kernels_gpu's table; the reference sees the same dtype-rounded inputs as the
kernels, which compute in fp32 and round once on store):
  * tensors stored in dtype T, per element: |out - ref| <= h_T |ref| + TOL[fp32] max|ref|, h_T
    one rounding (2^-8 bf16, 2^-11 fp16, 2^-24 fp32);
  * fp32 per-row vectors (mean, rstd): TOL[fp32] max|ref|;
  * row-summed fp32 outputs, per element: TOL[fp32] sum|term| + |preload| 2^-23 (a bound on
    sum|term|, not on the result: the atomic kernels have no fixed order)."""
import functools
from types import SimpleNamespace

import torch

import rowwise_ref as R
from test_kernels_gpu import TOL

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, F16, F32)
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
TOL32 = TOL[F32]
H_T = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
# eps = 1e-3, not the models' 1e-12 / 1e-6: at unit scale those are below fp32 rounding, so a
# kernel that dropped eps would pass; 1e-3 moves rstd by about 5e-4 of itself at unit variance
# (tests/test_bn_reference_gpu.py makes the same choice).
EPS = 1e-3
# The all-zero row of every normalisation case has rstd = eps^-1/2 = 31.6; its dy is scaled by
# 2^-5 so that its dx stays at the scale of the other rows' and does not widen max|ref|.
ZERO_ROW_DY = 2.0 ** -5
SENTINEL = -7.0
# The tables the scatter kernels add onto are preloaded at this scale, not at the scale of the
# sums: every atomicAdd rounds at the magnitude of what the element holds by then, n roundings
# for n colliding terms, and the bound grants the preload two (|preload| 2^-23).  A preload well
# below sum|term| keeps the later ones inside TOL[fp32] sum|term|; one that is dropped or
# doubled still misses the bound by a factor of thousands.
TABLE_PRELOAD = 2.0 ** -6


def tensor_bound(ref, h):
    return h * ref.abs() + TOL32 * ref.abs().max()


def vector_bound(ref):
    return (TOL32 * ref.abs().max()).expand_as(ref)


def sum_bound(sum_abs, preload):
    """0 where every term is zero: there the output is exactly the preload."""
    return torch.where(sum_abs == 0, torch.zeros_like(sum_abs),
                       TOL32 * sum_abs + preload.abs() * 2.0 ** -23)


def ratio(out, ref, bound, what):
    """max error / bound; where the bound is 0 (every term is zero) the output must be exact."""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(out).all(), f"{what}: not finite"
    err = (out - ref).abs()
    exact = bound == 0
    assert (err[exact] == 0).all(), f"{what}: must be exact where every term is zero"
    return (err[~exact] / bound[~exact]).max().item() if (~exact).any() else 0.0


def rounded(t, dt):
    """The values of t on dtype dt's grid, as fp64."""
    return t.to(dt).double()


def _id(dt, *shape):
    return "x".join(str(s) for s in shape) + "-" + NAME[dt]


# =============================================================================== LayerNorm
# D, 16-bit: one live lane | slot 0 exactly full | MV = 2 with one live lane in slot 1, ragged
# last 32-column block of the finalize | 768 | MV = 3, one live lane | MV = 4 | the maximum
# (64 KiB of LDS in the backward).  fp32: the same edges at its 4-element vectors.
LN_D = {BF16: [8, 512, 520, 768, 1032, 1544, 2048], F16: [8, 512, 520, 768, 1032, 1544, 2048],
        F32: [4, 256, 260, 768, 1024]}
# rows: less than one 4-wave block | 5 | one past a 16-row block (rpw 4) | one past a 32-row
# block (rpw 8) | 37
LN_ROWS = [1, 3, 5, 17, 33, 37]
LN_ROWS_WIDE = [5, 33]          # D >= 1032
LN_CASES = [(dt, rows, D) for dt in DTYPES for D in LN_D[dt] if D % R.vec_width(dt) == 0
            for rows in (LN_ROWS_WIDE if D >= 1032 else LN_ROWS)]
LN_IDS = [_id(dt, rows, D) for dt, rows, D in LN_CASES]


def ln_many_rows():
    """[(rows, D)] of the many-partials cases, from the finalize's constants: more than
    LN_FIN_LANES partial blocks at either rpw (rows = 1029 at D = 64), and at D = 32 the
    fewest rows, plus 5, with more than LN_FIN_LANES * LN_FIN_UNROLL blocks at rpw = 4."""
    a = R.LN_FIN_LANES * R.LN_WAVES * max(R.LN_RPW) + 5
    b = R.LN_FIN_LANES * R.LN_FIN_UNROLL * R.LN_WAVES * R.LN_RPW_MIN + 1 + 5
    return [(a, 64), (b, 32)]


LN_MANY = [(dt, rows, D) for dt in DTYPES for rows, D in ln_many_rows()]
LN_MANY_IDS = [_id(dt, rows, D) for dt, rows, D in LN_MANY]
# (dtype, D): over the register limit for the type; no multiple of the vector width
LN_REJECT = [(BF16, 2056), (F16, 2056), (F32, 1028), (BF16, 12)]


def _gamma(D, g):
    gam = torch.rand(D, generator=g) + 0.5
    gam[::7] *= -1.0
    return gam


@functools.lru_cache(maxsize=None)
def ln_case(dt, rows, D, zero_only=False):
    """Host inputs of one LayerNorm case: tensors on dt's grid (fp64), vectors fp32 as the
    kernels read them.  Row `zero` is all zeros in x, residual and xsum (none when rows == 1,
    unless zero_only: then the single row is the zero row).  Shared; never modified."""
    g = torch.Generator().manual_seed(7000 + 13 * rows + D)
    d = SimpleNamespace(dt=dt, rows=rows, D=D, zero=rows // 2 if rows > 1 else None)
    if zero_only:
        d.zero = 0
    off = torch.linspace(-1.5, 1.5, D)
    d.x = rounded(torch.randn(rows, D, generator=g) * 2 + off + torch.randn(rows, 1, generator=g),
                  dt)
    d.res = rounded(torch.randn(rows, D, generator=g), dt)
    # the backward's input: a stored sum on the grid
    d.xsum = rounded(torch.randn(rows, D, generator=g) * 2 + off
                     + torch.randn(rows, 1, generator=g), dt)
    dy = torch.randn(rows, D, generator=g)
    d.addin = rounded(torch.randn(rows, D, generator=g), dt)
    if d.zero is not None:
        d.x[d.zero] = 0.0
        d.res[d.zero] = 0.0
        d.xsum[d.zero] = 0.0
        dy[d.zero] *= ZERO_ROW_DY
    d.dy = rounded(dy, dt)
    d.gam = _gamma(D, g)
    d.bet = torch.randn(D, generator=g) * 0.3
    d.acc = [torch.randn(D, generator=g) * 3 for _ in range(2)]   # dgamma / dbeta preloads
    return d


@functools.lru_cache(maxsize=None)
def ln_bwd_ref(dt, rows, D, addin=False, zero_only=False):
    """The reference backward of one case at the fp32 statistics the kernel is handed
    (mean32, rstd32: the fp64 statistics of xsum rounded to fp32)."""
    d = ln_case(dt, rows, D, zero_only)
    f = R.layernorm_forward(d.xsum, None, d.gam, d.bet, EPS)
    m32, r32 = f.mean.float(), f.rstd.float()
    ref = R.layernorm_backward(d.xsum, d.dy, d.gam, EPS, d.addin if addin else None, m32, r32)
    ref.mean32, ref.rstd32 = m32, r32
    return ref


# =============================================================================== RMSNorm
RMS_D = {BF16: [8, 512, 520, 2048], F16: [8, 512, 520, 2048], F32: [4, 512, 260, 1024]}
# rows around the 8-rows-per-wave and the 32-rows-per-block splits
RMS_ROWS = [1, 7, 9, 31, 33, 37]
RMS_CASES = [(dt, rows, D) for dt in DTYPES for D in RMS_D[dt] for rows in RMS_ROWS]
RMS_IDS = [_id(dt, rows, D) for dt, rows, D in RMS_CASES]
RMS_MANY = [(dt, 1029, 64) for dt in DTYPES]
RMS_MANY_IDS = [_id(*c) for c in RMS_MANY]


@functools.lru_cache(maxsize=None)
def rms_case(dt, rows, D, zero_only=False):
    g = torch.Generator().manual_seed(8000 + 13 * rows + D)
    d = SimpleNamespace(dt=dt, rows=rows, D=D, zero=rows // 2 if rows > 1 else None)
    if zero_only:
        d.zero = 0
    x = torch.randn(rows, D, generator=g) * 2 + torch.linspace(-1.5, 1.5, D)
    dy = torch.randn(rows, D, generator=g)
    if d.zero is not None:
        x[d.zero] = 0.0
        dy[d.zero] *= ZERO_ROW_DY
    d.x, d.dy = rounded(x, dt), rounded(dy, dt)
    d.dx0 = rounded(torch.randn(rows, D, generator=g), dt)     # the residual gradient in dx
    d.w = _gamma(D, g)
    d.dw0 = torch.randn(D, generator=g) * 3
    return d


# =============================================================================== embeddings
EMB_VOCAB = 11
# (B, L, D): one element | the scalar type-gradient kernel (D % VEC != 0) | D / VEC = 9: the
# vector kernel's second block has one live column vector | BERT's width | the maximum
EMB_SHAPES = [(1, 1, 1), (2, 5, 70), (2, 5, 72), (3, 37, 768), (2, 9, 1024)]
EMB_CASES = [(dt, s) for dt in DTYPES for s in EMB_SHAPES]
EMB_IDS = [_id(dt, *s) for dt, s in EMB_CASES]
EMB_REJECT_D = R.EMB_MAXD + 1


@functools.lru_cache(maxsize=None)
def emb_case(dt, shape):
    """ids hold vocab - 1 (first token), a repeat of it, and `pad` (the last token's id); tt is
    mixed 0 / 1.  The position table has B * L + 2 rows, the tables are fp32."""
    B, L, D = shape
    g = torch.Generator().manual_seed(9000 + B * L + D)
    d = SimpleNamespace(dt=dt, B=B, L=L, D=D, rows=B * L, vocab=EMB_VOCAB, max_pos=B * L + 2)
    d.ids = torch.randint(0, EMB_VOCAB, (B, L), generator=g)
    d.ids[0, 0] = EMB_VOCAB - 1
    if L > 1:
        d.ids[0, 1] = EMB_VOCAB - 1
        d.ids[-1, -1] = 0
    d.pad = int(d.ids[-1, -1])
    d.tt = (torch.rand(B, L, generator=g) > 0.5).long()
    if L > 1:
        d.tt[0, 0], d.tt[0, 1] = 0, 1
    d.word = torch.randn(EMB_VOCAB, D, generator=g)
    d.pos = torch.randn(d.max_pos, D, generator=g) * 0.5
    d.type = torch.randn(2, D, generator=g) * 0.5
    d.gam = _gamma(D, g)
    d.bet = torch.randn(D, generator=g) * 0.3
    d.dsum = rounded(torch.randn(B * L, D, generator=g), dt)
    d.pre = [torch.randn(n, D, generator=g) * TABLE_PRELOAD for n in (EMB_VOCAB, d.max_pos, 2)]
    return d


# =============================================================================== pooling, gather
POOL_VOCAB = 7
POOL_SHAPES = [(1, 1, 1), (3, 7, 70), (5, 37, 300)]
POOL_MASKS = ["mixed", "zero"]
POOL_CASES = [(dt, s, m) for dt in DTYPES for s in POOL_SHAPES for m in POOL_MASKS]
POOL_IDS = [_id(dt, *s) + "-" + m for dt, s, m in POOL_CASES]
SCATTER_HEAVY = (4, 200, 70)                          # table rows, ids, D
GATHER_LONG = (R.GRID_CAP + 1, 256, BF16)             # n, D: the grid-stride loop's second trip


@functools.lru_cache(maxsize=None)
def pool_case(dt, shape, masks):
    """mask, per sample b: b % 3 == 0 interior holes, 1 fully masked, 2 full ("mixed"), or every
    sample fully masked ("zero").  ids are drawn from a 7-row table, so ids under a zero mask
    name rows that other tokens use."""
    B, L, D = shape
    g = torch.Generator().manual_seed(10000 + B * L + D)
    d = SimpleNamespace(dt=dt, B=B, L=L, D=D, vocab=POOL_VOCAB)
    mask = torch.ones(B, L, dtype=torch.int64)
    if masks == "zero":
        mask[:] = 0
    else:
        for b in range(B):
            if b % 3 == 0 and L > 2:
                mask[b, 1:-1] = (torch.rand(L - 2, generator=g) > 0.5).long()
                mask[b, 1] = 0
            elif b % 3 == 1:
                mask[b] = 0
    d.mask = mask
    d.ids = torch.randint(0, POOL_VOCAB, (B, L), generator=g)
    d.h = rounded(torch.randn(B, L, D, generator=g) + 0.5, dt)
    d.dout = rounded(torch.randn(B, D, generator=g), dt)
    d.table = torch.randn(POOL_VOCAB, D, generator=g)
    d.dtok = rounded(torch.randn(B * L, D, generator=g), dt)    # scatter's input
    d.pre = torch.randn(POOL_VOCAB, D, generator=g) * TABLE_PRELOAD
    return d


# =============================================================================== ViT pieces
PATCH_SHAPES = [(1, 1, 8, 8, 8), (2, 3, 32, 48, 16), (1, 3, 16, 16, 8)]       # N, C, H, W, p
PATCH_REJECT = [(1, 2, 8, 8, 4), (1, 1, 12, 8, 8)]          # p = 4 | H no multiple of p
# N, S, D; the last is above the grid cap (N * S * D > 8192 * 256)
TOKEN_SHAPES = [(1, 2, 1), (3, 5, 70), (2, 197, 768), (14, 197, 768)]
ADD_N = [1, 255, 257, R.GRID_CAP * 256 + 3]
assert 14 * 197 * 768 > R.GRID_CAP * 256 and 13 * 197 * 768 <= R.GRID_CAP * 256


def dyadic(shape, g, frac_bits, limit):
    """Random multiples of 2^-frac_bits inside (-limit, limit)."""
    v = torch.round(torch.randn(shape, generator=g) * 2.0 ** frac_bits) / 2.0 ** frac_bits
    return v.clamp(-limit + 2.0 ** -frac_bits, limit - 2.0 ** -frac_bits)
