"""fp64 CPU reference for the implicit-GEMM convolutions of csrc/conv.hip / csrc/igemm.h (torch
only): forward, data gradient and weight gradient of a full descriptor, their sums of |terms|,
the NHWC / packed layouts the kernels read and write, the two operand families of
tests/test_conv_reference_gpu.py (integer and Gaussian) with their comparisons, the forward
epilogue's BatchNorm slabs, and expected_path(): a host mirror of conv.hip's path functions
(conv_fwd_path, conv_dgrad_path, conv_wgrad_path) that names the kernel path each case takes.
tests/test_conv_ref_cpu.py holds it against mmdx_conv_describe, which prints what the launches
themselves consult, for the case table, the threshold shapes and the ResNet trunks.

A descriptor is the tuple cfg = (N, C, H, W, K, R, S, sh, sw, ph, pw): C is the channel count the
kernels see (a multiple of the vector width); c_master <= C is the master weight's / image's."""
from types import SimpleNamespace

import torch
import torch.nn.functional as tF

import bn_ref

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
H_T = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}   # one round to nearest on store
ACC = 2e-5                                  # fp32 accumulation in any order, times sum |terms|
EXACT_BF16 = 256.0                          # integers up to here are bf16 values
EXACT_F16 = 2048.0                          # ... and fp16 values
EXACT_F32 = 2.0 ** 24                       # integers below here are fp32 values


def vec(dt):
    """Elements of one 16-byte vector: the channel granularity of the kernels."""
    return 8 if dt == BF16 else 4


def pad_channels(c, dt):
    """c rounded up to the vector width."""
    v = vec(dt)
    return (c + v - 1) // v * v


def out_size(cfg):
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    return (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1


# ---------------------------------------------------------------------------- the case table
# id -> (cfg, c_master or None).  The smallest shapes that reach each edge of the dispatcher; what
# each one reaches is asserted by tests/test_conv_ref_cpu.py through expected_path().
CASES_BF16 = {
    # one ragged tile (M 35); nearly every pixel touches the border
    1: ((1, 64, 5, 7, 64, 3, 3, 1, 1, 1, 1), None),
    # ragged second N tile (72); K % 64 != 0: dgrad takes DgradK<false>; M 162
    2: ((2, 64, 9, 9, 72, 3, 3, 1, 1, 1, 1), None),
    # pointwise, two K tiles, three 64-column tiles
    3: ((3, 128, 7, 7, 192, 1, 1, 1, 1, 0, 0), None),
    # four merged phases of unequal size (8x7, 8x6, 7x7, 7x6 pixels per image)
    4: ((2, 64, 15, 13, 128, 3, 3, 2, 2, 1, 1), None),
    # three phases no tap reaches: zeros at beta 0, untouched at beta 1
    5: ((2, 64, 14, 14, 128, 1, 1, 2, 2, 0, 0), None),
    # last input row and column unreachable: dx there is 0
    6: ((1, 64, 8, 8, 64, 3, 3, 2, 2, 0, 0), None),
    # C no power of two: KLoad fallback, ragged K tail (216)
    7: ((2, 24, 9, 9, 64, 3, 3, 1, 1, 1, 1), None),
    # power-of-two C: the self-decoding DMA gather, ragged K tail (144)
    8: ((2, 16, 9, 9, 64, 3, 3, 1, 1, 1, 1), None),
    # 25 taps, under the 32-tap limit
    9: ((2, 8, 12, 12, 64, 5, 5, 1, 1, 2, 2), None),
    # 49 taps: the 64-tap gather; per-phase dgrad (taps > 32); the image has 3 real channels
    10: ((2, 8, 32, 32, 64, 7, 7, 2, 2, 3, 3), 3),
    # 390 tiles of 128x128: the 8-wave kernel in fwd and dgrad; ragged M (24948 = 194 * 128 + 116)
    11: ((33, 256, 27, 28, 256, 1, 1, 1, 1, 0, 0), None),
    # the same tile, non-pointwise forward
    12: ((33, 64, 27, 28, 256, 3, 3, 1, 1, 1, 1), None),
    # with MMDX_CONV_N64_WIDE=1: 256x64 tiles, the second with 41 live rows (M 297)
    13: ((3, 64, 9, 11, 64, 3, 3, 1, 1, 1, 1), None),
    # wgrad 64x64; two splits, the last short and ending mid-tile (2205 pixels)
    14: ((5, 64, 21, 21, 64, 1, 1, 1, 1, 0, 0), None),
    # wgrad 128x128, DmaRq (DmaR with MMDX_WGRAD_RQ=0)
    15: ((5, 64, 21, 21, 128, 3, 3, 1, 1, 1, 1), None),
    # wgrad 64x128
    16: ((5, 64, 21, 21, 64, 3, 3, 1, 1, 1, 1), None),
    # wgrad 128x64
    17: ((5, 64, 21, 21, 128, 1, 1, 1, 1, 0, 0), None),
    # nine splits: the reduction's 8-wide loop plus its tail
    18: ((5, 64, 43, 43, 64, 1, 1, 1, 1, 0, 0), None),
    # at least 128 splits: wgrad_reduce_z (wgrad only)
    19: ((32, 64, 64, 64, 64, 1, 1, 1, 1, 0, 0), None),
    # only the centre tap is valid
    20: ((2, 64, 1, 1, 64, 3, 3, 1, 1, 1, 1), None),
    # R != S, sh != sw, ph != pw: an r/s or h/w swap shows
    21: ((2, 64, 9, 12, 64, 3, 1, 2, 1, 1, 0), None),
    # deepest K (4608)
    22: ((2, 512, 7, 7, 512, 3, 3, 1, 1, 1, 1), None),
    # Added after reading conv_gemm_epi / conv_dgrad_phases_merged: three launches no case above
    # reaches.  23 = case 7 with K 72: the KLoad kernel's 128x128 tile (N > 64), ragged in N
    23: ((2, 24, 9, 9, 72, 3, 3, 1, 1, 1, 1), None),
    # the merged-phase dgrad's 128x128 tile needs >= 384 such tiles over all phases: 392 here,
    # every phase ragged in M (13 x (32x31, 32x30, 31x31, 31x30) pixels)
    24: ((13, 128, 63, 61, 64, 3, 3, 2, 2, 1, 1), None),
    # case 12 with C and K swapped: the 8-wave tile in a non-pointwise (DgradK) dgrad
    25: ((33, 256, 27, 28, 64, 3, 3, 1, 1, 1, 1), None),
}
# fp32: vector 4, BK 32, no DMA path
CASES_F32 = {
    # smallest channel counts
    "f1": ((2, 4, 9, 9, 12, 3, 3, 1, 1, 1, 1), None),
    # strided with K % 32 = 4: the dispatcher's phase rule needs K % BK == 0, so this one runs the
    # strided dgrad through the non-FAST DgradK (its stride division), not per-phase launches
    "f2": ((2, 32, 9, 9, 36, 3, 3, 2, 2, 1, 1), None),
    # asymmetric; K % 32 == 0: two per-phase launches (sh 2, sw 1)
    "f3": ((2, 32, 9, 12, 64, 3, 1, 2, 1, 1, 0), None),
    # RLoad split-K
    "f4": ((5, 32, 21, 21, 64, 1, 1, 1, 1, 0, 0), None),
    # added: f2 with K a multiple of 32, so that the fp32 per-phase launches also run with four
    # phases of unequal size (f2 as the issue states it never reaches them, see above)
    "f5": ((2, 32, 9, 9, 64, 3, 3, 2, 2, 1, 1), None),
    # added: the fp32 128x128 tiles (N > 64) of fwd and wgrad, ragged (72 of 128 columns) ...
    "f6": ((2, 32, 9, 9, 72, 3, 3, 1, 1, 1, 1), None),
    # ... and of the per-phase dgrad (C 72)
    "f7": ((2, 72, 9, 9, 64, 3, 3, 2, 2, 1, 1), None),
}
WGRAD_ONLY = {19}
GAUSSIAN = [2, 4, 7, 11, 21, "f2"]
# (case, knobs): runs of a case under launch-heuristic knobs besides the defaults
KNOB_RUNS = [(13, {"MMDX_CONV_N64_WIDE": 1}), (15, {"MMDX_WGRAD_RQ": 0})]


def case(cid):
    """(cfg, c_master, dtype) of a case id."""
    cfg, cm = (CASES_F32 if isinstance(cid, str) else CASES_BF16)[cid]
    return cfg, cm or cfg[1], F32 if isinstance(cid, str) else BF16


# -------------------------------------------------------------------------------- reference
def ref_fwd(x, w, cfg):
    """y[n,k,p,q] = sum_{c,r,s} x[n,c,p*sh-ph+r,q*sw-pw+s] w[k,c,r,s], NCHW / KCRS fp64."""
    sh, sw, ph, pw = cfg[7:]
    return tF.conv2d(x.double(), w.double(), stride=(sh, sw), padding=(ph, pw))


def ref_dgrad(dy, w, cfg):
    """dx = d sum(dy * y) / dx, [N, C, H, W] with C = the weight's channel count."""
    N, _, H, W = cfg[:4]
    sh, sw, ph, pw = cfg[7:]
    return torch.nn.grad.conv2d_input((N, w.shape[1], H, W), w.double(), dy.double(),
                                      stride=(sh, sw), padding=(ph, pw))


def ref_wgrad(x, dy, cfg):
    """dw = d sum(dy * y) / dw, [K, C, R, S] with C = x's channel count."""
    K, R, S, sh, sw, ph, pw = cfg[4:]
    return torch.nn.grad.conv2d_weight(x.double(), (K, x.shape[1], R, S), dy.double(),
                                       stride=(sh, sw), padding=(ph, pw))


def ref_abs_fwd(x, w, cfg):
    """sum of |terms| of ref_fwd: the conv of |x| and |w|."""
    return ref_fwd(x.abs(), w.abs(), cfg)


def ref_abs_dgrad(dy, w, cfg):
    return ref_dgrad(dy.abs(), w.abs(), cfg)


def ref_abs_wgrad(x, dy, cfg):
    return ref_wgrad(x.abs(), dy.abs(), cfg)


def reached(cfg):
    """[H, W] booleans: the input pixels at least one (tap, output pixel) pair reads — where dx
    has any term at all."""
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    P, Q = out_size(cfg)
    one = (1, 1, H, W, 1) + tuple(cfg[5:])
    return ref_dgrad(torch.ones(1, 1, P, Q), torch.ones(1, 1, R, S), one)[0, 0] > 0


# ---------------------------------------------------------------------------------- layouts
def to_nhwc(t, C, dt):
    """NCHW fp64 -> [N, H, W, C] of dtype dt, channels beyond t's zero (the padded lanes)."""
    N, c, H, W = t.shape
    out = torch.zeros(N, H, W, C, dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out.to(dt)


def from_nhwc(t):
    """Device or host [N, H, W, C] -> host NCHW fp64."""
    return t.detach().double().cpu().permute(0, 3, 1, 2)


def pad_c(t, C):
    """NCHW / KCRS fp64 with dimension 1 zero-padded to C channels."""
    out = torch.zeros(t.shape[0], C, *t.shape[2:], dtype=torch.float64)
    out[:, :t.shape[1]] = t
    return out


def pack_krsc(w, C, dt):
    """The master [K, c_master, R, S] as mmdx_conv_pack_weight writes it: [K][R][S][C]."""
    return pad_c(w.double(), C).permute(0, 2, 3, 1).contiguous().to(dt)


def pack_crsk(w, C, dt):
    """[C][R][S][K], the dgrad's weight operand."""
    return pad_c(w.double(), C).permute(1, 2, 3, 0).contiguous().to(dt)


def slab_stats(y, stat_rows):
    """(mean, M2) of each stat_rows-row slab of the forward output y (NCHW fp64; rows are the
    pixels (n, p, q)), the last slab ragged: fp32 [K][slabs][2] as the epilogue writes them."""
    K = y.shape[1]
    return bn_ref.slab_stats(y.permute(0, 2, 3, 1).reshape(-1, K), stat_rows)


# ------------------------------------------------------------------------------- generators
def gen_integer(shape, g):
    """Values in {-1, 0, 1}, zero with probability 1/2 (fp64)."""
    r = torch.randint(0, 4, shape, generator=g)
    return ((r == 2).double() - (r == 3).double())


def gen_gaussian(shape, g, dt, scale=1.0):
    """N(0, scale^2) on the grid of the compute dtype (fp64)."""
    return (torch.randn(shape, generator=g) * scale).to(dt).double()


def operands(cid, family):
    """x [N, c_master, H, W], w [K, c_master, R, S], dy [N, K, P, Q] of a case, fp64 values the
    compute dtype holds exactly."""
    cfg, cm, dt = case(cid)
    N, C, H, W, K, R, S = cfg[:7]
    P, Q = out_size(cfg)
    seed = (cid if isinstance(cid, int) else 100 + int(cid[1:])) + (0 if family == "int" else 1000)
    g = torch.Generator().manual_seed(seed)
    if family == "int":
        return (gen_integer((N, cm, H, W), g), gen_integer((K, cm, R, S), g),
                gen_integer((N, K, P, Q), g), g)
    return (gen_gaussian((N, cm, H, W), g, dt), gen_gaussian((K, cm, R, S), g, dt, 0.1),
            gen_gaussian((N, K, P, Q), g, dt), g)


# ------------------------------------------------------------------------------ comparisons
def check_exact_preconditions(ref, n_terms, dt_stored, what, step=1.0):
    """What makes an exact comparison legitimate, from the reference alone: every value an
    integer; storable in the output dtype (|v| <= 256 in bf16, <= 2048 in fp16, < 2^24 in fp32);
    and the sum of |terms| (at most n_terms: every |term| is 0 or 1) below 2^24, so that an fp32
    accumulator holds every partial sum in any order.  step (a power of two, 1 by default): the
    values are multiples of step instead, storable up to step times those limits (half-integers
    within 128 in bf16)."""
    assert torch.equal(ref, (ref / step).round() * step), \
        f"{what}: the reference is not integer-valued" + ("" if step == 1.0 else f" / {step}")
    top = {BF16: EXACT_BF16, F16: EXACT_F16}.get(dt_stored, EXACT_F32 - 1) * step
    assert ref.abs().max().item() <= top, f"{what}: max |ref| {ref.abs().max().item()} > {top}"
    assert n_terms < EXACT_F32, f"{what}: {n_terms} terms can exceed 2^24"


def assert_exact(got, ref, what):
    """got (any dtype / device) equals ref (fp64) element for element."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), got[tuple(i)].item(), ref[tuple(i)].item()) for i in idx[:8]]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; "
                         f"(index, got, ref): {first}")


def bound_ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 (no term at all) got must equal ref."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), "non-finite output"
    err = (got - ref).abs()
    zero = bound == 0
    assert (err[zero] == 0).all(), "must be exact where every term is zero"
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0


def assert_bounded(kind, got, ref, abs_terms, dt_stored, what, extra=None):
    """|got - ref| <= h_T |ref| + 2e-5 sum |terms| (+ extra), element by element; prints
    'convref <kind> <error / bound>' first and returns the ratio."""
    bound = H_T[dt_stored] * ref.abs() + ACC * abs_terms
    if extra is not None:
        bound = bound + extra
    ratio = bound_ratio(got, ref, bound)
    print(f"convref {kind} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{what}: {kind} error / bound = {ratio:.3f}"
    return ratio


# ----------------------------------------------------------------------- the dispatcher mirror
BK = {BF16: 64, F32: 32}          # igemm.h KTile<T>::BK
NARROW_BELOW = 384                # conv.hip kNarrowBelow
WGRAD_TARGET = 256                # common.h: MMDX_WGRAD_TARGET's default
_KNOBS = {"MMDX_CONV_N64_WIDE": -1, "MMDX_CONV_8W128": 1, "MMDX_WGRAD_RQ": 1,
          "MMDX_WGRAD_TARGET": WGRAD_TARGET, "MMDX_STEM_DIRECT": 1}


def _cdiv(a, b):
    return (a + b - 1) // b


def is_pointwise(cfg):
    return tuple(cfg[5:]) == (1, 1, 1, 1, 0, 0)


def dma_geom_ok(cfg, dgrad, max_taps=32, rows=0):
    """conv.hip dma_geom_ok: 32-bit byte offsets, the tap-mask width, rows the float reciprocal
    decodes, and stride 1 for the plain dgrad."""
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    P, Q = out_size(cfg)
    if N * H * W * C * 2 >= 1 << 31 or N * P * Q * K * 2 >= 1 << 31 or R * S > max_taps:
        return False
    if rows >= (1 << 22) - 256:
        return False
    return not dgrad or (sh == 1 and sw == 1)


def _stem_direct_geom(cfg):
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    P, Q = out_size(cfg)
    return (C == 8 and S == 4 and R in (7, 8) and sh == 2 and sw == 1 and ph == 0 and pw == 0
            and K == 64 and Q % 16 == 0 and Q <= 256 and P % 2 == 0 and 2 * (P - 1) + R <= H
            and Q + 3 <= W)


def _stages(blocks, ktiles):
    """conv.hip use_three_stages."""
    return 3 if blocks <= 256 and ktiles >= 4 else 2


def _gemm_path(operand, M, N, K, dma, kn, lane_tap=False):
    """conv.hip kmajor_tile: loader, tile and stages of a k-major conv GEMM [M, N, K]."""
    if not dma:
        return f"{operand}/kload/{'128x64' if N <= 64 else '128x128'}"
    dname = "dma-lanetap" if lane_tap else "dma"
    tiles128 = _cdiv(M, 128) * _cdiv(N, 128)
    wide = kn["MMDX_CONV_N64_WIDE"]
    wide = _cdiv(M, 256) >= 1024 if wide < 0 else wide != 0
    if N <= 64 and wide:
        return f"{operand}/{dname}/256x64"
    if N <= 64 or tiles128 < NARROW_BELOW:
        ns = _stages(_cdiv(M, 128) * _cdiv(N, 64), _cdiv(K, 64))
        return f"{operand}/{dname}/128x64/ns{ns}"
    return f"{operand}/{dname}/128x128-8w" if kn["MMDX_CONV_8W128"] else \
        f"{operand}/{dname}/128x128/ns{_stages(tiles128, _cdiv(K, 64))}"


def phases(cfg):
    """conv.hip phase_geom for every (a, b) = (h mod sh, w mod sw): dicts with the phase's grid
    Hp x Wp, its tap counts and GEMM sizes M, K (K == 0: no tap reaches the phase)."""
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    out = []
    for a in range(sh):
        for b in range(sw):
            Hp = _cdiv(H - a, sh) if H > a else 0
            Wp = _cdiv(W - b, sw) if W > b else 0
            if Hp == 0 or Wp == 0:
                continue
            r0, s0 = (a + ph) % sh, (b + pw) % sw
            ntr = (R - 1 - r0) // sh + 1 if r0 < R else 0
            nts = (S - 1 - s0) // sw + 1 if s0 < S else 0
            out.append(dict(a=a, b=b, Hp=Hp, Wp=Wp, M=N * Hp * Wp, K=ntr * nts * K))
    return out


def plan_wgrad(cfg, dt, target=WGRAD_TARGET):
    """conv.hip plan_wgrad: tile, split count, pixels per split (the pixel-pair stem: about 256
    splits of whole 2-row pixel tiles)."""
    N, C, H, W, K, R, S = cfg[:7]
    P, Q = out_size(cfg)
    M, Nn, Kl = K, R * S * C, N * P * Q
    bm = 64 if M <= 64 else 128
    bn = 64 if Nn <= 64 else 128
    if dt == BF16 and _stem_direct_geom(cfg) and R == 7:
        ptiles = Kl // (2 * Q)
        tps = _cdiv(ptiles, 256)
        return SimpleNamespace(bm=bm, bn=bn, splits=_cdiv(ptiles, tps), kper=tps * 2 * Q)
    tiles = _cdiv(M, bm) * _cdiv(Nn, bn)
    ktiles = _cdiv(Kl, BK[dt])
    s = max(1, min(_cdiv(target, tiles), ktiles // 16))
    kper = _cdiv(ktiles, s) * BK[dt]
    return SimpleNamespace(bm=bm, bn=bn, splits=_cdiv(Kl, kper), kper=kper)


def dgrad_stat_blocks(cfg, dt):
    """mmdx_conv_dgrad_stat_blocks: 128-row slots of the fused BN-backward statistics, 0 where
    the fusion does not apply."""
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    if dt != BF16 or K % 64 or C % 8:
        return 0
    if sh == 1 and sw == 1:
        return _cdiv(N * H * W, 128) if dma_geom_ok(cfg, True, 32, N * H * W) else 0
    if not dma_geom_ok(cfg, False, 32, N * _cdiv(H, sh) * _cdiv(W, sw)):   # not phases-merged
        return 0
    ph_ = phases(cfg)
    return 0 if any(p["K"] == 0 for p in ph_) else sum(_cdiv(p["M"], 128) for p in ph_)


def expected_path(cfg, dt, knobs=None, beta=0.0):
    """The kernel path conv.hip's dispatcher takes for this descriptor: names for fwd (also
    mmdx_conv_fwd_bn_eval's, but for the direct stem), dgrad (at this beta) and wgrad, and the
    weight-gradient plan; desc(pass) is mmdx_conv_describe's string.

    fwd / stride-1 dgrad: <operand>/<loader>/<tile>[/ns<stages>], operand point | fast | generic
    (PointFwdK / PointDgradK, Im2colK / DgradK <true>, <false>), loader dma | dma-lanetap (the
    power-of-two self-decoding gather) | kload.  Strided dgrad with K % BK == 0:
    phases-merged/dma/<tile> or phases-each/kload/<tile>.  wgrad: <bm>x<bn>/<operand>/ns<stages>/
    <reduction>, operand DmaRq | DmaR | DmaR-point | RLoad, reduction reduce | reduce-z.  The
    pixel-pair stem's direct kernels (MMDX_STEM_DIRECT): stem-direct, stem-direct/<reduction>."""
    kn = dict(_KNOBS)
    kn.update(knobs or {})
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    P, Q = out_size(cfg)
    bk, bf = BK[dt], dt == BF16
    out = SimpleNamespace()

    # conv_fwd_path
    M, Kg = N * P * Q, R * S * C
    if bf and kn["MMDX_STEM_DIRECT"] and _stem_direct_geom(cfg):
        out.fwd = "stem-direct"
    elif C % bk == 0 and is_pointwise(cfg):
        out.fwd = _gemm_path("point", M, K, Kg, bf and dma_geom_ok(cfg, False, 32, M), kn)
    elif C % bk == 0:
        out.fwd = _gemm_path("fast", M, K, Kg, bf and dma_geom_ok(cfg, False, 32, M), kn)
    else:
        pow2 = C >= 8 and C & (C - 1) == 0 and R * S <= 64
        out.fwd = _gemm_path("generic", M, K, Kg, bf and pow2 and dma_geom_ok(cfg, False, 64, M),
                             kn, lane_tap=True)

    # conv_dgrad_path: a phase no tap reaches is launched (to write zeros) at beta 0 only
    out.phases = phases(cfg) if (sh > 1 or sw > 1) else []
    if (sh > 1 or sw > 1) and K % bk == 0:
        rows = N * _cdiv(H, sh) * _cdiv(W, sw)
        tiles128 = sum(_cdiv(p["M"], 128) * _cdiv(C, 128) for p in out.phases
                       if p["K"] or beta == 0)
        if bf and dma_geom_ok(cfg, False, 32, rows):
            tile = "128x64" if C <= 64 or tiles128 < NARROW_BELOW else "128x128"
            out.dgrad = f"phases-merged/dma/{tile}"
        else:
            out.dgrad = f"phases-each/kload/{'128x64' if C <= 64 else '128x128'}"
    else:
        M, Kg = N * H * W, R * S * K
        if K % bk == 0 and is_pointwise(cfg):
            out.dgrad = _gemm_path("point", M, C, Kg, bf and dma_geom_ok(cfg, True, 32, M), kn)
        elif K % bk == 0:
            out.dgrad = _gemm_path("fast", M, C, Kg, bf and dma_geom_ok(cfg, True, 32, M), kn)
        else:
            out.dgrad = _gemm_path("generic", M, C, Kg, False, kn)

    # conv_wgrad_path
    p = plan_wgrad(cfg, dt, kn["MMDX_WGRAD_TARGET"])
    out.plan = p
    Kl, total = N * P * Q, K * R * S * C
    red = "reduce" if total % 4 or p.splits < 128 else "reduce-z"
    out.desc = lambda pas: (out.fwd, out.dgrad, f"{out.wgrad}/s{p.splits}/k{p.kper}")[pas]
    if (bf and _stem_direct_geom(cfg) and kn["MMDX_STEM_DIRECT"] and R == 7
            and p.kper % (2 * Q) == 0 and Kl % (2 * Q) == 0 and 2 * Q <= 256
            and W * (2 + R) <= 3 * 512):
        out.wgrad = f"stem-direct/{red}"
        return out
    if bf and dma_geom_ok(cfg, False, 1 << 30) and Kl < 1 << 23:
        op = "DmaR-point" if is_pointwise(cfg) else "DmaRq" if kn["MMDX_WGRAD_RQ"] else "DmaR"
        blocks = _cdiv(K, p.bm) * _cdiv(R * S * C, p.bn) * p.splits
        op += f"/ns{_stages(blocks, _cdiv(p.kper, 64))}"
    else:
        op = "RLoad"
    out.wgrad = f"{p.bm}x{p.bn}/{op}/{red}"
    return out


def describe(lib, cfg, dt, pas, beta=0.0):
    """mmdx_conv_describe for this descriptor (under the knobs the library currently holds);
    pas 0 fwd, 1 dgrad, 2 wgrad."""
    import ctypes
    from mmdx import _lib as L
    N, C, H, W, K, R, S, sh, sw, ph, pw = cfg
    d = L.ConvDesc(N, H, W, C, K, R, S, sh, sw, ph, pw, *out_size(cfg))
    buf = ctypes.create_string_buffer(96)
    rc = lib.mmdx_conv_describe(L.dtype_code(dt), pas, d, beta, buf, len(buf))
    assert rc == 0, lib.mmdx_last_error().decode()
    return buf.value.decode()
