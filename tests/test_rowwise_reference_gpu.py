"""The row-wise normalisation kernels and the memory-bound token kernels against the fp64
reference of tests/rowwise_ref.py, called through their C entry points with raw pointers at the
smallest shapes that reach each code path.  The case tables, the host inputs and the derived
bounds are in tests/rowwise_cases.py (tests/test_rowwise_ref_cpu.py shows on the CPU that every
case is well posed for fp32 under the same bounds).  Every check prints
"rowref <kind> <error / bound> <case>" before it asserts; every output buffer is preloaded with
NaN where it must be fully overwritten and with a sentinel (or the table's preload) where part
of it must stay as it was.

Covered entry points:
  norm.hip (LayerNorm part): mmdx_layernorm_fwd, mmdx_layernorm_bwd (both MMDX_LN_BWD_RPW
    values, beta_acc 0 / 1 / 0.5, dgamma or dbeta NULL), mmdx_layernorm_bwd_residual,
    mmdx_layernorm_workspace_size;
  t5.hip (RMSNorm part): mmdx_rmsnorm_fwd, mmdx_rmsnorm_bwd, mmdx_rmsnorm_workspace_size;
  text.hip: mmdx_embed_ln_fwd, mmdx_embed_bwd (the word, position and both token-type kernels),
    mmdx_masked_mean_fwd / _bwd, mmdx_embed_mean_fwd / _bwd, mmdx_embed_gather, mmdx_embed_scatter;
  vit.hip: mmdx_patchify, mmdx_vit_tokens_fwd / _bwd, mmdx_rows_copy, mmdx_add.
Deliberately not covered: mmdx_layernorm_fwd_dropout and mmdx_layernorm_bwd_dropout
(tests/test_ln_dropout_gpu.py holds them bit-equal to the unfused path checked here) and
everything in lstm.hip.

Bit-for-bit checks: pure data movement (gather to fp32, rows_copy, vit_tokens_bwd, patchify to
fp32) equals the reference; patchify and gather into 16-bit equal the reference rounded once.
mmdx_vit_tokens_fwd adds a dtype-T embedding to an fp32 position row in fp32; its inputs are on
a dyadic grid on which that fp32 sum is exact, so its one rounding is the reference's.  mmdx_add
adds two dtype-T values in fp32: that sum is exact or far from a rounding boundary of T for the
16-bit types and is the correctly rounded fp32 sum for fp32, so it equals the fp64 sum rounded
once to T for all three."""
import collections

import pytest
import torch

import mmdx._lib as L
import rowwise_cases as K
import rowwise_ref as R
from rowwise_cases import BF16, F32, EPS, SENTINEL

pytestmark = pytest.mark.gpu

PAD = 4                     # rows allocated past `rows`: they keep the sentinel
NAN = float("nan")
RAN = collections.defaultdict(set)         # test function -> the table cases it ran
REJECTED = collections.defaultdict(list)   # entry point -> the arguments it refused


# =============================================================================== helpers
def _check(kind, out, ref, bound, what):
    r = K.ratio(out, ref, bound, f"{what}: {kind}")
    print(f"rowref {kind} {r:.4f} {what}")
    assert r <= 1.0, f"{what}: {kind} error / bound = {r:.3f}"


def _tensor(out, ref, dt, kind, what):
    """A tensor stored in dtype dt, elementwise."""
    _check(kind, out, ref, K.tensor_bound(ref, K.H_T[dt]), what)


def _vector(out, ref, kind, what):
    """An fp32 per-row vector."""
    _check(kind, out, ref, K.vector_bound(ref), what)


def _sum(out, grad, sum_abs, preload, kind, what):
    """A row-summed fp32 output onto `preload` (fp64 of the fp32 values the buffer held)."""
    _check(kind, out, grad + preload, K.sum_bound(sum_abs, preload), what)


def _equal(out, want, kind, what):
    """Bit for bit (want: a host tensor of out's dtype)."""
    same = out.dtype == want.dtype and torch.equal(out.cpu(), want)
    print(f"rowref {kind} {0.0 if same else float('inf'):.4f} {what}")
    assert same, f"{what}: {kind} differs from the reference in " \
                 f"{(out.cpu() != want).sum().item()} elements"


def _buf(dev, dt, rows, D, fill=NAN, pad=PAD):
    """[rows + pad, D]: `fill` in the rows a kernel writes, the sentinel in the rest."""
    t = torch.full((rows + pad, D), SENTINEL, dtype=dt, device=dev)
    t[:rows] = fill
    return t


def _vecbuf(dev, n, fill=NAN, pad=PAD):
    t = torch.full((n + pad,), SENTINEL, device=dev)
    t[:n] = fill
    return t


def _untouched(t, n, what):
    assert (t[n:] == SENTINEL).all(), f"{what}: written past the end"


def _rejects(name, match, args, outs, what):
    """A call that must return non-zero (L.call raises) and leave the sentinel-filled outs."""
    with pytest.raises(RuntimeError, match=match):
        L.call(name, *args)
    torch.cuda.synchronize()
    for t in outs:
        assert (t == SENTINEL).all(), f"{name} {what}: wrote an output before refusing"
    REJECTED[name].append(what)
    print(f"rowref rejected {name} {what}")


def _ln_ws(rows, D, dev):
    n = L.lib().mmdx_layernorm_workspace_size(rows, D)
    assert n == R.layernorm_workspace_size(rows, D) > 0
    return torch.full((n // 4,), NAN, device=dev), n


def _rms_ws(rows, D, dev):
    n = L.lib().mmdx_rmsnorm_workspace_size(rows, D)
    assert n == R.rmsnorm_workspace_size(rows, D) > 0
    return torch.full((n // 4,), NAN, device=dev), n


# =============================================================================== LayerNorm
def _ln_fwd(dev, d, what):
    dt, rows, D, dc = d.dt, d.rows, d.D, L.dtype_code(d.dt)
    x, res = d.x.to(dev, dt), d.res.to(dev, dt)
    gam, bet = d.gam.to(dev), d.bet.to(dev)
    for use_res in (0, 1):
        ref = R.layernorm_forward(d.x, d.res if use_res else None, d.gam, d.bet, EPS)
        for use_sum in (0, 1):
            w = f"{what} res={use_res} sum_out={use_sum}"
            y = _buf(dev, dt, rows, D)
            xs = _buf(dev, dt, rows, D) if use_sum else None
            mean, rstd = _vecbuf(dev, rows), _vecbuf(dev, rows)
            L.call("mmdx_layernorm_fwd", dc, x.data_ptr(), res.data_ptr() if use_res else None,
                   rows, D, gam.data_ptr(), bet.data_ptr(), EPS, y.data_ptr(), L.ptr(xs),
                   mean.data_ptr(), rstd.data_ptr(), L.stream())
            torch.cuda.synchronize()
            _tensor(y[:rows], ref.y, dt, "y", w)
            _vector(mean[:rows], ref.mean, "mean", w)
            _vector(rstd[:rows], ref.rstd, "rstd", w)
            for t in (y, mean, rstd):
                _untouched(t, rows, w)
            if use_sum:
                _tensor(xs[:rows], ref.xsum, dt, "xsum", w)
                _untouched(xs, rows, w)
            if d.zero is not None:   # exact sums: y == beta on dt's grid, mean == 0
                assert torch.equal(y[d.zero].cpu(), d.bet.to(dt)), f"{w}: zero row"
                assert mean[d.zero].item() == 0.0, f"{w}: zero row"


@pytest.mark.parametrize("case", K.LN_CASES, ids=K.LN_IDS)
def test_layernorm_fwd(dev, case):
    """mmdx_layernorm_fwd: with and without residual and sum_out, save_mean / save_rstd, the
    all-zero row, the rows past `rows` untouched."""
    RAN["test_layernorm_fwd"].add(case)
    _ln_fwd(dev, K.ln_case(*case), f"ln fwd {K._id(*case)}")
    if case[1] == 1:    # one row: the zero row is a run of its own
        _ln_fwd(dev, K.ln_case(*case, zero_only=True), f"ln fwd zero row {K._id(*case)}")


def _ln_bwd_call(dev, d, ref, beta_acc, ws, ws_n, what, want_dg=True, want_db=True, addin=None):
    """One mmdx_layernorm_bwd (or _bwd_residual with addin) launch and its checks."""
    dt, rows, D, dc = d.dt, d.rows, d.D, L.dtype_code(d.dt)
    xs, dy, gam = d.xsum.to(dev, dt), d.dy.to(dev, dt), d.gam.to(dev)
    mean, rstd = ref.mean32.to(dev), ref.rstd32.to(dev)
    dx = _buf(dev, dt, rows, D)
    dg, db = _vecbuf(dev, D), _vecbuf(dev, D)
    if beta_acc != 0.0:
        dg[:D], db[:D] = d.acc[0].to(dev), d.acc[1].to(dev)
    ws.fill_(NAN)
    tail = (dx.data_ptr(), dg.data_ptr() if want_dg else None, db.data_ptr() if want_db else None,
            beta_acc, ws.data_ptr(), ws_n, L.stream())
    head = (dc, xs.data_ptr(), dy.data_ptr(), rows, D, gam.data_ptr(), mean.data_ptr(),
            rstd.data_ptr())
    if addin is None:
        L.call("mmdx_layernorm_bwd", *head, *tail)
    else:
        a = addin.to(dev, dt)
        L.call("mmdx_layernorm_bwd_residual", *head, a.data_ptr(), *tail)
    torch.cuda.synchronize()
    _tensor(dx[:rows], ref.dx, dt, "dx" if addin is None else "dx+addin", what)
    _untouched(dx, rows, what)
    pre = [a.double() * beta_acc for a in d.acc]
    if want_dg:
        _sum(dg[:D], ref.dgamma, ref.sum_abs_gx, pre[0], "dgamma", what)
    else:
        assert torch.isnan(dg[:D]).all(), f"{what}: dgamma == NULL was written"
    if want_db:
        _sum(db[:D], ref.dbeta, ref.sum_abs_g, pre[1], "dbeta", what)
    else:
        assert torch.isnan(db[:D]).all(), f"{what}: dbeta == NULL was written"
    _untouched(dg, D, what)
    _untouched(db, D, what)


def _ln_bwd(dev, knobs, case, zero_only, what):
    d = K.ln_case(*case, zero_only=zero_only)
    ref = K.ln_bwd_ref(*case, False, zero_only)
    ref_add = K.ln_bwd_ref(*case, True, zero_only)
    ws, ws_n = _ln_ws(d.rows, d.D, dev)
    for rpw in R.LN_RPW:
        knobs("MMDX_LN_BWD_RPW", rpw)
        for beta_acc in (0.0, 1.0, 0.5):
            _ln_bwd_call(dev, d, ref, beta_acc, ws, ws_n, f"{what} rpw={rpw} beta_acc={beta_acc}")
        _ln_bwd_call(dev, d, ref_add, 1.0, ws, ws_n, f"{what} rpw={rpw} residual",
                     addin=d.addin)
    knobs("MMDX_LN_BWD_RPW", None)
    _ln_bwd_call(dev, d, ref, 0.0, ws, ws_n, f"{what} dgamma=NULL", want_dg=False)
    _ln_bwd_call(dev, d, ref, 0.0, ws, ws_n, f"{what} dbeta=NULL", want_db=False)


@pytest.mark.parametrize("case", K.LN_CASES, ids=K.LN_IDS)
def test_layernorm_bwd(dev, knobs, case):
    """mmdx_layernorm_bwd and mmdx_layernorm_bwd_residual: dx, dgamma and dbeta under both
    MMDX_LN_BWD_RPW values, accumulation onto preloaded dgamma / dbeta, either of them NULL."""
    RAN["test_layernorm_bwd"].add(case)
    _ln_bwd(dev, knobs, case, False, f"ln bwd {K._id(*case)}")
    if case[1] == 1:
        _ln_bwd(dev, knobs, case, True, f"ln bwd zero row {K._id(*case)}")


@pytest.mark.parametrize("case", K.LN_MANY, ids=K.LN_MANY_IDS)
def test_layernorm_bwd_many_partials(dev, knobs, case):
    """More partial blocks than the finalize has lanes (its strided loop runs more than once per
    lane), and more than LN_FIN_LANES * LN_FIN_UNROLL of them at rpw = 4 (the unrolled body and
    its tail both run)."""
    RAN["test_layernorm_bwd_many_partials"].add(case)
    dt, rows, D = case
    blocks = {rpw: R.ln_partial_blocks(rows, rpw) for rpw in R.LN_RPW}
    if (rows, D) == K.ln_many_rows()[0]:
        assert min(blocks.values()) > R.LN_FIN_LANES
    else:
        assert blocks[R.LN_RPW_MIN] > R.LN_FIN_LANES * R.LN_FIN_UNROLL
        assert blocks[R.LN_RPW_MIN] % R.LN_FIN_UNROLL != 0
    d, ref = K.ln_case(*case), K.ln_bwd_ref(*case)
    ws, ws_n = _ln_ws(rows, D, dev)
    for rpw in R.LN_RPW:
        knobs("MMDX_LN_BWD_RPW", rpw)
        for beta_acc in (0.0, 1.0):
            _ln_bwd_call(dev, d, ref, beta_acc, ws, ws_n,
                         f"ln bwd {K._id(*case)} partials={blocks[rpw]} beta_acc={beta_acc}")


def test_layernorm_rejections(dev):
    """D over the register limit, D no multiple of the vector width, a workspace one byte short:
    a non-zero return, no output written."""
    rows = 5
    for dt, D in K.LN_REJECT:
        dc = L.dtype_code(dt)
        x = torch.zeros(rows, D, dtype=dt, device=dev)
        f = torch.zeros(max(rows, D), device=dev)
        y, xs = _buf(dev, dt, rows, D, SENTINEL), _buf(dev, dt, rows, D, SENTINEL)
        v = [_vecbuf(dev, max(rows, D), SENTINEL) for _ in range(2)]
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        what = f"{K.NAME[dt]} D={D}"
        _rejects("mmdx_layernorm_fwd", "layernorm: D=",
                 (dc, x.data_ptr(), None, rows, D, f.data_ptr(), f.data_ptr(), EPS, y.data_ptr(),
                  xs.data_ptr(), v[0].data_ptr(), v[1].data_ptr(), L.stream()), [y, xs] + v, what)
        _rejects("mmdx_layernorm_bwd", "layernorm bwd: D=",
                 (dc, x.data_ptr(), x.data_ptr(), rows, D, f.data_ptr(), f.data_ptr(),
                  f.data_ptr(), y.data_ptr(), v[0].data_ptr(), v[1].data_ptr(), 0.0,
                  ws.data_ptr(), ws.numel(), L.stream()), [y] + v, what)
        _rejects("mmdx_layernorm_bwd_residual", "layernorm bwd: D=",
                 (dc, x.data_ptr(), x.data_ptr(), rows, D, f.data_ptr(), f.data_ptr(),
                  f.data_ptr(), x.data_ptr(), y.data_ptr(), v[0].data_ptr(), v[1].data_ptr(),
                  0.0, ws.data_ptr(), ws.numel(), L.stream()), [y] + v, what)
    for dt, D in [(BF16, 768), (F32, 260)]:
        x = torch.zeros(rows, D, dtype=dt, device=dev)
        f = torch.zeros(max(rows, D), device=dev)
        y = _buf(dev, dt, rows, D, SENTINEL)
        v = [_vecbuf(dev, D, SENTINEL) for _ in range(2)]
        ws, ws_n = _ln_ws(rows, D, dev)
        _rejects("mmdx_layernorm_bwd", "workspace too small",
                 (L.dtype_code(dt), x.data_ptr(), x.data_ptr(), rows, D, f.data_ptr(),
                  f.data_ptr(), f.data_ptr(), y.data_ptr(), v[0].data_ptr(), v[1].data_ptr(), 0.0,
                  ws.data_ptr(), ws_n - 1, L.stream()), [y] + v,
                 f"{K.NAME[dt]} D={D} workspace {ws_n - 1} of {ws_n} bytes")


# =============================================================================== RMSNorm
def _rms(dev, d, what):
    dt, rows, D, dc = d.dt, d.rows, d.D, L.dtype_code(d.dt)
    x, dy, w = d.x.to(dev, dt), d.dy.to(dev, dt), d.w.to(dev)
    fwd = R.rmsnorm_forward(d.x, d.w, EPS)
    for use_rstd in (1, 0):
        y = _buf(dev, dt, rows, D)
        rstd = _vecbuf(dev, rows) if use_rstd else None
        L.call("mmdx_rmsnorm_fwd", dc, x.data_ptr(), rows, D, w.data_ptr(), EPS, y.data_ptr(),
               L.ptr(rstd), L.stream())
        torch.cuda.synchronize()
        _tensor(y[:rows], fwd.y, dt, "y", f"{what} srstd={use_rstd}")
        _untouched(y, rows, what)
        if use_rstd:
            _vector(rstd[:rows], fwd.rstd, "rstd", what)
            _untouched(rstd, rows, what)
        if d.zero is not None:
            assert not y[d.zero].any(), f"{what}: zero row"
    rstd32 = fwd.rstd.float().to(dev)
    ws, ws_n = _rms_ws(rows, D, dev)
    for beta in (0.0, 1.0):
        for beta_acc in (0.0, 1.0):
            w2 = f"{what} beta={beta} beta_acc={beta_acc}"
            ref = R.rmsnorm_backward(d.x, d.dy, d.w, EPS, d.dx0, beta, d.dw0, beta_acc)
            dx = _buf(dev, dt, rows, D, NAN if beta == 0.0 else 0.0)
            if beta != 0.0:
                dx[:rows] = d.dx0.to(dev, dt)
            dw = _vecbuf(dev, D)
            if beta_acc != 0.0:
                dw[:D] = d.dw0.to(dev)
            ws.fill_(NAN)
            L.call("mmdx_rmsnorm_bwd", dc, x.data_ptr(), dy.data_ptr(), rows, D, w.data_ptr(),
                   rstd32.data_ptr(), dx.data_ptr(), beta, dw.data_ptr(), beta_acc,
                   ws.data_ptr(), ws_n, L.stream())
            torch.cuda.synchronize()
            _tensor(dx[:rows], ref.dx, dt, "dx", w2)
            pre = d.dw0.double() * beta_acc
            _sum(dw[:D], ref.dw - pre, ref.sum_abs_w, pre, "dw", w2)
            _untouched(dx, rows, w2)
            _untouched(dw, D, w2)


@pytest.mark.parametrize("case", K.RMS_CASES + K.RMS_MANY, ids=K.RMS_IDS + K.RMS_MANY_IDS)
def test_rmsnorm(dev, case):
    """mmdx_rmsnorm_fwd (with and without save_rstd) and mmdx_rmsnorm_bwd: beta onto a preloaded
    dx (one rounding of grad + beta * dx0), beta_acc onto a preloaded dw; rows around the 8-row
    wave and the 32-row block splits; 1029 rows: 33 partial blocks."""
    RAN["test_rmsnorm"].add(case)
    _rms(dev, K.rms_case(*case), f"rms {K._id(*case)}")
    if case[1] == 1:
        _rms(dev, K.rms_case(*case, zero_only=True), f"rms zero row {K._id(*case)}")


def test_rmsnorm_rejections(dev):
    rows = 5
    for dt, D in K.LN_REJECT:       # the same limits as LayerNorm's
        dc = L.dtype_code(dt)
        x = torch.zeros(rows, D, dtype=dt, device=dev)
        f = torch.zeros(max(rows, D), device=dev)
        y = _buf(dev, dt, rows, D, SENTINEL)
        v = [_vecbuf(dev, max(rows, D), SENTINEL) for _ in range(2)]
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        what = f"{K.NAME[dt]} D={D}"
        _rejects("mmdx_rmsnorm_fwd", "rmsnorm: D=",
                 (dc, x.data_ptr(), rows, D, f.data_ptr(), EPS, y.data_ptr(), v[0].data_ptr(),
                  L.stream()), [y] + v, what)
        _rejects("mmdx_rmsnorm_bwd", "rmsnorm bwd: D=",
                 (dc, x.data_ptr(), x.data_ptr(), rows, D, f.data_ptr(), f.data_ptr(),
                  y.data_ptr(), 0.0, v[0].data_ptr(), 0.0, ws.data_ptr(), ws.numel(),
                  L.stream()), [y] + v, what)
    dt, D = BF16, 512
    x = torch.zeros(rows, D, dtype=dt, device=dev)
    f = torch.zeros(max(rows, D), device=dev)
    y, dw = _buf(dev, dt, rows, D, SENTINEL), _vecbuf(dev, D, SENTINEL)
    ws, ws_n = _rms_ws(rows, D, dev)
    _rejects("mmdx_rmsnorm_bwd", "workspace too small",
             (L.dtype_code(dt), x.data_ptr(), x.data_ptr(), rows, D, f.data_ptr(), f.data_ptr(),
              y.data_ptr(), 0.0, dw.data_ptr(), 0.0, ws.data_ptr(), ws_n - 1, L.stream()),
             [y, dw], f"bf16 D={D} workspace {ws_n - 1} of {ws_n} bytes")


# =============================================================================== embeddings
@pytest.mark.parametrize("case", K.EMB_CASES, ids=K.EMB_IDS)
def test_embed_ln_fwd(dev, case):
    """mmdx_embed_ln_fwd: tt mixed 0 / 1 and NULL, xsum present and NULL; repeated ids, the
    table's last row, position rows by row % L with B > 1."""
    RAN["test_embed_ln_fwd"].add(case)
    d = K.emb_case(*case)
    dt, rows, D, dc = d.dt, d.rows, d.D, L.dtype_code(d.dt)
    ids, tt = d.ids.to(dev), d.tt.to(dev)
    word, pos, typ, gam, bet = (t.to(dev) for t in (d.word, d.pos, d.type, d.gam, d.bet))
    for use_tt in (1, 0):
        ref = R.embed_ln_forward(d.ids, d.tt if use_tt else None, d.word, d.pos, d.type, d.gam,
                                 d.bet, EPS)
        for use_sum in (1, 0):
            what = f"embed fwd {K._id(*case[:1], *case[1])} tt={use_tt} xsum={use_sum}"
            y = _buf(dev, dt, rows, D)
            xs = _buf(dev, dt, rows, D) if use_sum else None
            mean, rstd = _vecbuf(dev, rows), _vecbuf(dev, rows)
            L.call("mmdx_embed_ln_fwd", dc, ids.data_ptr(), tt.data_ptr() if use_tt else None,
                   d.B, d.L, D, word.data_ptr(), pos.data_ptr(), typ.data_ptr(), gam.data_ptr(),
                   bet.data_ptr(), EPS, y.data_ptr(), L.ptr(xs), mean.data_ptr(),
                   rstd.data_ptr(), L.stream())
            torch.cuda.synchronize()
            _tensor(y[:rows], ref.y, dt, "y", what)
            _vector(mean[:rows], ref.mean, "mean", what)
            _vector(rstd[:rows], ref.rstd, "rstd", what)
            for t in (y, mean, rstd):
                _untouched(t, rows, what)
            if use_sum:
                _tensor(xs[:rows], ref.xsum, dt, "xsum", what)
                _untouched(xs, rows, what)


def test_embed_ln_fwd_rejects_wide_rows(dev):
    B, Lq, D = 1, 2, K.EMB_REJECT_D
    ids = torch.zeros(B, Lq, dtype=torch.int64, device=dev)
    f = torch.zeros(2 * D, device=dev)
    y, xs = _buf(dev, BF16, B * Lq, D, SENTINEL), _buf(dev, BF16, B * Lq, D, SENTINEL)
    v = [_vecbuf(dev, B * Lq, SENTINEL) for _ in range(2)]
    _rejects("mmdx_embed_ln_fwd", "embed_ln: D=",
             (L.BF16, ids.data_ptr(), None, B, Lq, D, f.data_ptr(), f.data_ptr(), f.data_ptr(),
              f.data_ptr(), f.data_ptr(), EPS, y.data_ptr(), xs.data_ptr(), v[0].data_ptr(),
              v[1].data_ptr(), L.stream()), [y, xs] + v, f"D={D}")


def _embed_bwd(dev, d, tt, pad, what, null=None, misalign=False):
    dt, D, dc = d.dt, d.D, L.dtype_code(d.dt)
    ref = R.embed_backward(d.ids, tt, d.dsum, pad, d.vocab, d.max_pos)
    ids = d.ids.to(dev)
    ttd = None if tt is None else tt.to(dev)
    if misalign:    # one element past a 16-byte boundary: the scalar type-gradient kernel
        flat = torch.zeros(d.rows * D + 8, dtype=dt, device=dev)
        dsum = flat[1:1 + d.rows * D]
        dsum.copy_(d.dsum.to(dev, dt).flatten())
        assert flat.data_ptr() % 16 == 0 and dsum.data_ptr() % 16 != 0
    else:
        dsum = d.dsum.to(dev, dt)
        assert dsum.data_ptr() % 16 == 0
    tabs = [p.to(dev) for p in d.pre]
    ptrs = [None if i == null else t.data_ptr() for i, t in enumerate(tabs)]
    L.call("mmdx_embed_bwd", dc, ids.data_ptr(), L.ptr(ttd), d.B, d.L, D, dsum.data_ptr(), *ptrs,
           pad, L.stream())
    torch.cuda.synchronize()
    grads = [(ref.dword, ref.abs_word, "dword"), (ref.dpos, ref.abs_pos, "dpos"),
             (ref.dtype, ref.abs_type, "dtype")]
    for i, (grad, sum_abs, kind) in enumerate(grads):
        if i == null:
            assert torch.equal(tabs[i].cpu(), d.pre[i]), f"{what}: {kind} == NULL"
        else:
            _sum(tabs[i], grad, sum_abs, d.pre[i].double(), kind, what)
    if pad >= 0 and null != 0:      # the pad row keeps its preload exactly
        assert torch.equal(tabs[0][pad].cpu(), d.pre[0][pad]), f"{what}: pad row"


@pytest.mark.parametrize("case", K.EMB_CASES, ids=K.EMB_IDS)
def test_embed_bwd(dev, case):
    """mmdx_embed_bwd onto preloaded tables: pad_id among the ids and -1, tt mixed and NULL, each
    table NULL in turn; the vector type-gradient kernel (D = 72, 768, 1024), the scalar one by
    D % VEC != 0 (D = 1, 70) and by a dsum one element off a 16-byte boundary."""
    RAN["test_embed_bwd"].add(case)
    d = K.emb_case(*case)
    name = K._id(case[0], *case[1])
    assert d.rows % 32 != 0
    for use_tt in (1, 0):
        for pad in (d.pad, -1):
            _embed_bwd(dev, d, d.tt if use_tt else None, pad,
                       f"embed bwd {name} tt={use_tt} pad={pad}")
    # tt values other than 1 go to row 0 (backward only: the forward indexes the table by tt)
    _embed_bwd(dev, d, d.tt * 2, d.pad, f"embed bwd {name} tt in (0, 2)")
    for null in (0, 1, 2):
        _embed_bwd(dev, d, d.tt, d.pad, f"embed bwd {name} null={null}", null=null)
    if d.D % R.vec_width(d.dt) == 0:
        _embed_bwd(dev, d, d.tt, d.pad, f"embed bwd {name} misaligned dsum", misalign=True)


# =============================================================================== pooling, gather
@pytest.mark.parametrize("case", K.POOL_CASES, ids=K.POOL_IDS)
def test_masked_mean_embed_mean_gather_scatter(dev, case):
    RAN["test_masked_mean_embed_mean_gather_scatter"].add(case)
    d = K.pool_case(*case)
    dt, B, Lq, D, dc = d.dt, d.B, d.L, d.D, L.dtype_code(d.dt)
    what = f"pool {K.POOL_IDS[K.POOL_CASES.index(case)]}"
    ids, mask = d.ids.to(dev), d.mask.to(dev)
    # (every device input has a name: a temporary's memory may be handed to the next one)
    h, dout, dtok = d.h.to(dev, dt), d.dout.to(dev, dt), d.dtok.to(dev, dt)
    empty = (d.mask.sum(1) == 0).to(dev)
    st = L.stream()

    out = _buf(dev, dt, B, D)
    L.call("mmdx_masked_mean_fwd", dc, h.data_ptr(), mask.data_ptr(), B, Lq, D, out.data_ptr(), st)
    torch.cuda.synchronize()
    _tensor(out[:B], R.masked_mean(d.h, d.mask), dt, "masked_mean", what)
    assert not out[:B][empty].any(), f"{what}: a fully masked sample pools to exactly 0"
    _untouched(out, B, what)

    dh = _buf(dev, dt, B * Lq, D)
    L.call("mmdx_masked_mean_bwd", dc, dout.data_ptr(), mask.data_ptr(), B, Lq, D, dh.data_ptr(),
           st)
    torch.cuda.synchronize()
    _tensor(dh[:B * Lq].view(B, Lq, D), R.masked_mean_backward(d.dout, d.mask, Lq), dt,
            "masked_mean_bwd", what)
    assert not dh[:B * Lq].view(B, Lq, D)[empty].any(), f"{what}: fully masked: dh exactly 0"
    _untouched(dh, B * Lq, what)

    table = d.table.to(dev)
    out = _buf(dev, dt, B, D)
    L.call("mmdx_embed_mean_fwd", dc, ids.data_ptr(), mask.data_ptr(), B, Lq, D,
           table.data_ptr(), out.data_ptr(), st)
    torch.cuda.synchronize()
    _tensor(out[:B], R.embed_mean(d.ids, d.mask, d.table), dt, "embed_mean", what)
    assert not out[:B][empty].any(), f"{what}: a fully masked sample pools to exactly 0"
    _untouched(out, B, what)

    pre = d.pre.double()
    dtab = d.pre.to(dev)
    L.call("mmdx_embed_mean_bwd", dc, ids.data_ptr(), mask.data_ptr(), B, Lq, D,
           dout.data_ptr(), dtab.data_ptr(), st)
    torch.cuda.synchronize()
    ref = R.embed_mean_backward(d.ids, d.mask, d.dout, d.vocab)
    _sum(dtab, ref.dtable, ref.sum_abs, pre, "embed_mean_bwd", what)   # (exact under zero masks)

    n = B * Lq
    flat = d.ids.flatten()
    got = _buf(dev, dt, n, D)
    L.call("mmdx_embed_gather", dc, ids.data_ptr(), n, D, table.data_ptr(), got.data_ptr(), st)
    torch.cuda.synchronize()
    _equal(got[:n], R.gather(flat, d.table).to(dt), "gather", what)
    _untouched(got, n, what)

    dtab = d.pre.to(dev)
    L.call("mmdx_embed_scatter", dc, ids.data_ptr(), n, D, dtok.data_ptr(), dtab.data_ptr(), st)
    torch.cuda.synchronize()
    ref = R.scatter(flat, d.dtok, d.vocab)
    _sum(dtab, ref.dtable, ref.sum_abs, pre, "scatter", what)


@pytest.mark.parametrize("dt", K.DTYPES, ids=[K.NAME[dt] for dt in K.DTYPES])
def test_scatter_heavily_repeated_ids(dev, dt):
    """200 rows onto a 4-row table, one of whose rows no id names: about 67 colliding atomics
    per element, and a row that keeps its preload exactly."""
    V, n, D = K.SCATTER_HEAVY
    g = torch.Generator().manual_seed(11000)
    ids = torch.randint(0, V - 1, (n,), generator=g)
    dout = K.rounded(torch.randn(n, D, generator=g), dt)
    pre = torch.randn(V, D, generator=g) * K.TABLE_PRELOAD
    dtab, ids_d, dout_d = pre.to(dev), ids.to(dev), dout.to(dev, dt)
    L.call("mmdx_embed_scatter", L.dtype_code(dt), ids_d.data_ptr(), n, D, dout_d.data_ptr(),
           dtab.data_ptr(), L.stream())
    torch.cuda.synchronize()
    ref = R.scatter(ids, dout, V)
    assert (ref.sum_abs[V - 1] == 0).all()
    _sum(dtab, ref.dtable, ref.sum_abs, pre.double(), "scatter", f"heavy {K.NAME[dt]}")


def test_gather_second_grid_stride_trip(dev):
    """n * D just above 8192 blocks x 256 threads: the grid-stride loop's second trip."""
    n, D, dt = K.GATHER_LONG
    assert (n - 1) * D == R.GRID_CAP * 256 < n * D
    g = torch.Generator().manual_seed(12000)
    V = 50
    ids = torch.randint(0, V, (n,), generator=g)
    ids[-1] = V - 1
    table = torch.randn(V, D, generator=g)
    got = _buf(dev, dt, n, D)
    ids_d, table_d = ids.to(dev), table.to(dev)
    L.call("mmdx_embed_gather", L.dtype_code(dt), ids_d.data_ptr(), n, D, table_d.data_ptr(),
           got.data_ptr(), L.stream())
    torch.cuda.synchronize()
    _equal(got[:n], R.gather(ids, table).to(dt), "gather", f"long n={n} D={D}")
    _untouched(got, n, "long gather")
    got32 = _buf(dev, F32, 37, D)
    L.call("mmdx_embed_gather", L.F32, ids_d.data_ptr(), 37, D, table_d.data_ptr(),
           got32.data_ptr(), L.stream())
    torch.cuda.synchronize()
    _equal(got32[:37], table[ids[:37]], "gather", "fp32: data movement")


# =============================================================================== ViT pieces
@pytest.mark.parametrize("dt", K.DTYPES, ids=[K.NAME[dt] for dt in K.DTYPES])
def test_patchify(dev, dt):
    ran = 0
    for N, C, H, W, p in K.PATCH_SHAPES:
        g = torch.Generator().manual_seed(13000 + H + W)
        x = torch.randn(N, C, H, W, generator=g)
        rows, Kp = N * (H // p) * (W // p), C * p * p
        out, x_d = _buf(dev, dt, rows, Kp), x.to(dev)
        L.call("mmdx_patchify", L.dtype_code(dt), x_d.data_ptr(), N, C, H, W, p,
               out.data_ptr(), L.stream())
        torch.cuda.synchronize()
        _equal(out[:rows], R.patchify(x, p).to(dt), "patchify",
               f"{K.NAME[dt]} {(N, C, H, W, p)}")
        _untouched(out, rows, "patchify")
        ran += 1
    assert ran == len(K.PATCH_SHAPES)
    for N, C, H, W, p in K.PATCH_REJECT:
        x = torch.zeros(N, C, H, W, device=dev)
        out = torch.full((N * H * W * C + 64,), SENTINEL, dtype=dt, device=dev)
        _rejects("mmdx_patchify", "patchify: bad shape",
                 (L.dtype_code(dt), x.data_ptr(), N, C, H, W, p, out.data_ptr(), L.stream()),
                 [out], f"{K.NAME[dt]} {(N, C, H, W, p)}")


@pytest.mark.parametrize("dt", K.DTYPES, ids=[K.NAME[dt] for dt in K.DTYPES])
def test_vit_tokens(dev, dt):
    """mmdx_vit_tokens_fwd / _bwd; the last shape is above the grid cap.  Inputs on a dyadic
    grid: embeddings multiples of 2^-6 below 4, class token and positions multiples of 2^-12
    below 2, so emb + pos is exact in fp32 and the kernel's one rounding is the reference's."""
    ran = 0
    for N, S, D in K.TOKEN_SHAPES:
        g = torch.Generator().manual_seed(14000 + N + S)
        emb = K.dyadic((N, S - 1, D), g, 6, 4.0)
        cls, pos = K.dyadic((D,), g, 12, 2.0), K.dyadic((S, D), g, 12, 2.0)
        assert torch.equal(emb.to(dt).float(), emb)
        dtok = torch.randn(N, S, D, generator=g).to(dt)
        what = f"{K.NAME[dt]} {(N, S, D)}"
        tok = _buf(dev, dt, N * S, D)
        emb_d, cls_d, pos_d, dtok_d = emb.to(dev, dt), cls.to(dev), pos.to(dev), dtok.to(dev)
        L.call("mmdx_vit_tokens_fwd", L.dtype_code(dt), emb_d.data_ptr(), cls_d.data_ptr(),
               pos_d.data_ptr(), N, S, D, tok.data_ptr(), L.stream())
        torch.cuda.synchronize()
        _equal(tok[:N * S].view(N, S, D), R.vit_tokens_fwd(emb, cls, pos).to(dt), "vit_tokens_fwd",
               what)
        _untouched(tok, N * S, what)
        demb = _buf(dev, dt, N * (S - 1), D)
        L.call("mmdx_vit_tokens_bwd", L.dtype_code(dt), dtok_d.data_ptr(), N, S, D,
               demb.data_ptr(), L.stream())
        torch.cuda.synchronize()
        _equal(demb[:N * (S - 1)].view(N, S - 1, D), R.vit_tokens_bwd(dtok).to(dt),
               "vit_tokens_bwd", what)
        _untouched(demb, N * (S - 1), what)
        ran += 1
    assert ran == len(K.TOKEN_SHAPES)


@pytest.mark.parametrize("dt", K.DTYPES, ids=[K.NAME[dt] for dt in K.DTYPES])
def test_rows_copy(dev, dt):
    """src_ld and dst_ld both larger than D and different; the gap columns of dst keep the
    sentinel; src_ld < D (and dst_ld < D) refused."""
    rows, D, src_ld, dst_ld = 37, 70, 75, 83
    g = torch.Generator().manual_seed(15000)
    src = torch.randn(rows * src_ld, generator=g).to(dt)
    dst = torch.full((rows * dst_ld + 5,), SENTINEL, dtype=dt)
    out, src_d = dst.to(dev), src.to(dev)
    L.call("mmdx_rows_copy", L.dtype_code(dt), src_d.data_ptr(), src_ld, out.data_ptr(),
           dst_ld, rows, D, L.stream())
    torch.cuda.synchronize()
    want = R.rows_copy(src, src_ld, dst, dst_ld, rows, D)
    assert (want == SENTINEL).sum() >= rows * (dst_ld - D)
    _equal(out, want, "rows_copy", f"{K.NAME[dt]} {rows}x{D} ld {src_ld}->{dst_ld}")
    for s_ld, d_ld in [(D - 1, dst_ld), (src_ld, D - 1)]:
        out = dst.to(dev)
        _rejects("mmdx_rows_copy", "rows_copy: bad shape",
                 (L.dtype_code(dt), src_d.data_ptr(), s_ld, out.data_ptr(), d_ld, rows, D,
                  L.stream()), [out], f"{K.NAME[dt]} D={D} src_ld={s_ld} dst_ld={d_ld}")


@pytest.mark.parametrize("dt", K.DTYPES, ids=[K.NAME[dt] for dt in K.DTYPES])
def test_add(dev, dt):
    """out = x + y rounded once to T (see the file's docstring), n around one block and above
    the grid cap."""
    ran = 0
    for n in K.ADD_N:
        g = torch.Generator().manual_seed(16000 + n % 1000)
        x, y = torch.randn(n, generator=g).to(dt), (torch.randn(n, generator=g) * 3).to(dt)
        out, x_d, y_d = _buf(dev, dt, n, 1), x.to(dev), y.to(dev)
        L.call("mmdx_add", L.dtype_code(dt), n, x_d.data_ptr(), y_d.data_ptr(),
               out.data_ptr(), L.stream())
        torch.cuda.synchronize()
        _equal(out[:n, 0], R.add(x, y).to(dt), "add", f"{K.NAME[dt]} n={n}")
        _untouched(out, n, "add")
        ran += 1
    assert ran == len(K.ADD_N)
    out = torch.full((4,), SENTINEL, dtype=dt, device=dev)
    _rejects("mmdx_add", "add: empty", (L.dtype_code(dt), 0, out.data_ptr(), out.data_ptr(),
                                        out.data_ptr(), L.stream()), [out], f"{K.NAME[dt]} n=0")


# =============================================================================== accounting
TABLES = {"test_layernorm_fwd": K.LN_CASES, "test_layernorm_bwd": K.LN_CASES,
          "test_layernorm_bwd_many_partials": K.LN_MANY, "test_rmsnorm": K.RMS_CASES + K.RMS_MANY,
          "test_embed_ln_fwd": K.EMB_CASES, "test_embed_bwd": K.EMB_CASES,
          "test_masked_mean_embed_mean_gather_scatter": K.POOL_CASES}


def test_every_table_case_ran(dev, request):
    """No case is skipped at run time: each parametrised test ran every case of its table (the
    dtype and vector-width filter is applied where the tables are built).  Checked for the
    tests that were selected whole; prints what the library refused, per entry point."""
    selected = collections.Counter(i.originalname for i in request.session.items
                                   if i.module is request.module)
    for name, table in TABLES.items():
        if selected[name] == len(table):
            assert len(RAN[name]) == len(table), f"{name}: ran {len(RAN[name])} of {len(table)}"
    for name in sorted(REJECTED):
        print(f"rowref rejected-by {name}: " + "; ".join(REJECTED[name]))
