"""CPU: tests/rowwise_ref.py (the fp64 reference of tests/test_rowwise_reference_gpu.py) against
torch.nn.functional and autograd in double, its host mirrors against hand-worked values, and
the conditioning of every case of the GPU suite: a plain fp32 torch evaluation of the same
formulas, with another summation order than the kernels', must stay within half of the GPU
suite's bounds, so a kernel that misses a bound cannot blame its inputs.

The fp32 evaluation is not rounded to the 16-bit types (that rounding alone uses up h_T |ref|);
its tensors are held to the bound of an fp32 store, h = 2^-24, for every compute dtype — the
tighter choice."""
import pytest
import torch
import torch.nn.functional as tF

import rowwise_cases as K
import rowwise_ref as R

F64 = torch.float64
EPS = 1e-5


def _same(a, b, what):
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert a.shape == b.shape, what
    assert err <= 1e-12 * max(1.0, b.abs().max().item()), f"{what}: {err}"


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed)) * scale


# =============================================================================== the reference
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("rows,D", [(1, 4), (9, 12), (5, 260)])
def test_layernorm_matches_torch(rows, D, use_res):
    x, res, dy = _rand(rows, D, seed=1, scale=2) + 0.5, _rand(rows, D, seed=2), _rand(rows, D, seed=3)
    gam, bet, addin = _rand(D, seed=4) + 1, _rand(D, seed=5), _rand(rows, D, seed=6)
    f = R.layernorm_forward(x, res if use_res else None, gam, bet, EPS)
    xs = (x + res if use_res else x).clone().requires_grad_(True)
    g, b = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    y = tF.layer_norm(xs, (D,), g, b, EPS)
    y.backward(dy)
    _same(f.xsum, xs.detach(), "xsum")
    _same(f.y, y.detach(), "y")
    _same(f.mean, xs.detach().mean(-1), "mean")
    _same(f.rstd, 1 / torch.sqrt(xs.detach().var(-1, unbiased=False) + EPS), "rstd")
    bw = R.layernorm_backward(f.xsum, dy, gam, EPS)
    _same(bw.dx, xs.grad, "dx")
    _same(bw.dgamma, g.grad, "dgamma")
    _same(bw.dbeta, b.grad, "dbeta")
    _same(bw.mean, f.mean, "backward mean")
    _same(bw.rstd, f.rstd, "backward rstd")
    xhat = (f.xsum - f.mean[:, None]) * f.rstd[:, None]
    _same(bw.sum_abs_gx, (dy * xhat).abs().sum(0), "sum |dy xhat|")
    _same(bw.sum_abs_g, dy.abs().sum(0), "sum |dy|")
    _same(R.layernorm_backward(f.xsum, dy, gam, EPS, addin).dx, xs.grad + addin, "dx + addin")
    # the statistics a kernel is handed replace the values: the exact ones change nothing,
    # coarse ones give the closed form evaluated at them
    same = R.layernorm_backward(f.xsum, dy, gam, EPS, None, f.mean, f.rstd)
    _same(same.dx, xs.grad, "dx at the exact statistics")
    _same(same.dgamma, g.grad, "dgamma at the exact statistics")
    m, r = f.mean.bfloat16().double(), f.rstd.bfloat16().double()
    coarse = R.layernorm_backward(f.xsum, dy, gam, EPS, None, m, r)
    _same(coarse.dgamma, (dy * (f.xsum - m[:, None]) * r[:, None]).sum(0), "dgamma, coarse")
    _same(coarse.mean, m, "mean, coarse")


def test_layernorm_zero_row():
    """An all-zero row: y == beta and rstd == eps^-1/2 exactly, for any D."""
    gam, bet = _rand(7, seed=1), _rand(7, seed=2)
    f = R.layernorm_forward(torch.zeros(2, 7, dtype=F64), None, gam, bet, 1e-3)
    assert torch.equal(f.y, bet.expand(2, 7)) and torch.equal(f.mean, torch.zeros(2, dtype=F64))
    _same(f.rstd, torch.full((2,), 1e-3 ** -0.5, dtype=F64), "rstd")


@pytest.mark.parametrize("rows,D", [(1, 4), (9, 12)])
def test_rmsnorm_matches_autograd(rows, D):
    x, dy, w = _rand(rows, D, seed=1, scale=2), _rand(rows, D, seed=2), _rand(D, seed=3) + 1
    dx0, dw0 = _rand(rows, D, seed=4), _rand(D, seed=5)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    if hasattr(tF, "rms_norm"):
        y = tF.rms_norm(xr, (D,), wr, EPS)
    else:
        y = wr * (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + EPS))
    y.backward(dy)
    f = R.rmsnorm_forward(x, w, EPS)
    _same(f.y, y.detach(), "y")
    _same(f.rstd, torch.rsqrt(x.pow(2).mean(-1) + EPS), "rstd")
    b = R.rmsnorm_backward(x, dy, w, EPS)
    _same(b.dx, xr.grad, "dx")
    _same(b.dw, wr.grad, "dw")
    _same(b.sum_abs_w, (dy * x * f.rstd[:, None]).abs().sum(0), "sum |dy x rstd|")
    b = R.rmsnorm_backward(x, dy, w, EPS, dx0, 1.0, dw0, 0.5)
    _same(b.dx, xr.grad + dx0, "dx + beta dx0")
    _same(b.dw, wr.grad + 0.5 * dw0, "dw + beta_acc dw0")


@pytest.mark.parametrize("use_tt", [False, True])
def test_embeddings_match_torch_embedding(use_tt):
    B, L, D, V, P = 3, 5, 6, 9, 8
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[0, 0], ids[1, 2], ids[2, 4] = V - 1, V - 1, 2
    tt = torch.randint(0, 3, (B, L), generator=g) if use_tt else None   # 2: "everything else"
    word, pos, typ = _rand(V, D, seed=1), _rand(P, D, seed=2), _rand(2, D, seed=3)
    gam, bet, dsum = _rand(D, seed=4) + 1, _rand(D, seed=5), _rand(B * L, D, seed=6)
    trow = (tt == 1).long() if use_tt else torch.zeros(B, L, dtype=torch.long)
    for pad in (2, -1):
        w, p, t = (x.clone().requires_grad_(True) for x in (word, pos, typ))
        wrows = tF.embedding(ids, w, padding_idx=pad if pad >= 0 else None)
        s = wrows + tF.embedding(torch.arange(L).expand(B, L), p) + tF.embedding(trow, t)
        y = tF.layer_norm(s, (D,), gam, bet, EPS)
        s.backward(dsum.view(B, L, D))
        f = R.embed_ln_forward(ids, tt, word, pos, typ, gam, bet, EPS)
        _same(f.xsum, s.detach().view(B * L, D), "xsum")
        _same(f.y, y.detach().view(B * L, D), "y")
        _same(f.mean, s.detach().view(B * L, D).mean(-1), "mean")
        b = R.embed_backward(ids, tt, dsum, pad, V, P)
        _same(b.dword, w.grad, "dword")
        _same(b.dpos, p.grad, "dpos")
        _same(b.dtype, t.grad, "dtype")
        if pad >= 0:
            assert (b.dword[pad] == 0).all() and (b.abs_word[pad] == 0).all()
        assert (b.dpos[L:] == 0).all()
        a = R.embed_backward(ids, tt, dsum.abs(), pad, V, P)
        _same(b.abs_word, a.dword, "abs_word")
        _same(b.abs_pos, a.dpos, "abs_pos")
        _same(b.abs_type, a.dtype, "abs_type")
    if not use_tt:
        assert (b.dtype[1] == 0).all() and (b.abs_type[1] == 0).all()


def test_masked_mean_and_embed_mean():
    B, L, D, V = 4, 6, 5, 7
    g = torch.Generator().manual_seed(4)
    h, dout, table = _rand(B, L, D, seed=1), _rand(B, D, seed=2), _rand(V, D, seed=3)
    ids = torch.randint(0, V, (B, L), generator=g)
    mask = torch.tensor([[1, 0, 1, 1, 0, 1], [0] * 6, [1] * 6, [1, 0, 0, 0, 0, 0]])
    want = torch.zeros(B, D, dtype=F64)
    for b in range(B):                       # hand-written: the mean of the kept tokens
        keep = [l for l in range(L) if mask[b, l]]
        if keep:
            want[b] = sum(h[b, l] for l in keep) / len(keep)
    _same(R.masked_mean(h, mask), want, "masked_mean")
    hr = h.clone().requires_grad_(True)
    cnt = mask.sum(1, keepdim=True).clamp(min=1)
    ((hr * mask[..., None]).sum(1) / cnt).backward(dout)
    dh = R.masked_mean_backward(dout, mask, L)
    _same(dh, hr.grad, "masked_mean backward")
    assert (dh[1] == 0).all() and (R.masked_mean(h, mask)[1] == 0).all()

    tr = table.clone().requires_grad_(True)
    out = (tF.embedding(ids, tr) * mask[..., None]).sum(1) / cnt
    out.backward(dout)
    _same(R.embed_mean(ids, mask, table), out.detach(), "embed_mean")
    eb = R.embed_mean_backward(ids, mask, dout, V)
    _same(eb.dtable, tr.grad, "embed_mean backward")
    _same(eb.sum_abs, R.embed_mean_backward(ids, mask, dout.abs(), V).dtable, "sum_abs")


def test_gather_scatter():
    V, D, n = 4, 3, 50
    ids = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(5))
    table, dout = _rand(V, D, seed=1), _rand(n, D, seed=2)
    _same(R.gather(ids, table), table.index_select(0, ids), "gather")
    s = R.scatter(ids, dout, V)
    _same(s.dtable, torch.zeros(V, D, dtype=F64).index_add_(0, ids, dout), "scatter")
    _same(s.sum_abs, torch.zeros(V, D, dtype=F64).index_add_(0, ids, dout.abs()), "sum_abs")


@pytest.mark.parametrize("N,C,H,W,p", K.PATCH_SHAPES)
def test_patchify_matches_unfold(N, C, H, W, p):
    x = _rand(N, C, H, W, seed=H)
    want = tF.unfold(x, p, stride=p).transpose(1, 2).reshape(-1, C * p * p)
    got = R.patchify(x, p)
    assert torch.equal(got, want)
    # as the patch-embedding GEMM uses it: patches @ W.flatten(1).T == conv2d(x, W, stride = p)
    wt = _rand(5, C, p, p, seed=1)
    conv = tF.conv2d(x, wt, stride=p).permute(0, 2, 3, 1).reshape(-1, 5)
    _same(got @ wt.flatten(1).T, conv, "patch embedding")


def test_vit_tokens_rows_copy_add():
    N, S, D = 2, 4, 3
    emb, cls, pos, dtok = _rand(N, S - 1, D, seed=1), _rand(D, seed=2), _rand(S, D, seed=3), \
        _rand(N, S, D, seed=4)
    tok = R.vit_tokens_fwd(emb, cls, pos)
    for n in range(N):
        _same(tok[n, 0], cls + pos[0], "class token")
        for q in range(S - 1):
            _same(tok[n, 1 + q], emb[n, q] + pos[1 + q], "patch token")
    assert torch.equal(R.vit_tokens_bwd(dtok), dtok[:, 1:])
    src, dst = torch.arange(20.0), torch.full((30,), -7.0)
    out = R.rows_copy(src, 6, dst, 9, 3, 4)
    for r in range(3):
        assert torch.equal(out[r * 9:r * 9 + 4], src[r * 6:r * 6 + 4])
        assert (out[r * 9 + 4:(r + 1) * 9] == -7.0).all()
    assert (out[27:] == -7.0).all() and (dst == -7.0).all()
    assert torch.equal(R.add(emb, emb), 2 * emb)


def test_host_mirrors():
    assert R.layernorm_workspace_size(1, 8) == 1 * 2 * 8 * 4
    assert R.layernorm_workspace_size(16, 768) == 1 * 2 * 768 * 4
    assert R.layernorm_workspace_size(17, 768) == 2 * 2 * 768 * 4
    assert R.rmsnorm_workspace_size(32, 512) == 512 * 4
    assert R.rmsnorm_workspace_size(33, 512) == 2 * 512 * 4
    assert R.ln_partial_blocks(33, 8) == 2 and R.ln_partial_blocks(33, 4) == 3
    assert R.ln_max_d(torch.bfloat16) == 2048 and R.ln_max_d(torch.float32) == 1024
    (a, da), (b, db) = K.ln_many_rows()
    assert (a, da, b, db) == (1029, 64, 4102, 32)
    # more than one strided trip per lane at either rpw; more than one unrolled body at rpw 4
    assert min(R.ln_partial_blocks(a, r) for r in R.LN_RPW) > R.LN_FIN_LANES
    assert R.ln_partial_blocks(b, 4) == R.LN_FIN_LANES * R.LN_FIN_UNROLL + 1
    assert R.ln_partial_blocks(b - 6, 4) == R.LN_FIN_LANES * R.LN_FIN_UNROLL


def test_case_tables():
    """The tables hold what the suite's docstrings promise."""
    assert len(K.LN_CASES) == 2 * (4 * 6 + 3 * 2) + 5 * 6
    assert all(D % R.vec_width(dt) == 0 and D <= R.ln_max_d(dt) for dt, _, D in K.LN_CASES)
    assert len(K.RMS_CASES) == 3 * 4 * 6 and len(K.EMB_CASES) == 3 * 5
    assert len(K.POOL_CASES) == 3 * 3 * 2
    for dt, rows, D in K.LN_CASES:
        d = K.ln_case(dt, rows, D)
        for t in (d.x, d.res, d.xsum, d.dy, d.addin):
            assert torch.equal(t, K.rounded(t, dt))
        if rows > 1:
            assert not d.x[d.zero].any() and not d.xsum[d.zero].any() and not d.res[d.zero].any()
    for dt, shape, masks in K.POOL_CASES:
        d = K.pool_case(dt, shape, masks)
        cnt = d.mask.sum(1)
        if masks == "zero":
            assert (cnt == 0).all()
        elif d.B >= 3:
            assert cnt[1] == 0 and cnt[2] == d.L and 0 < cnt[0] < d.L and d.mask[0, 1] == 0
    for dt, shape in K.EMB_CASES:
        d = K.emb_case(dt, shape)
        assert (d.ids == d.vocab - 1).sum() >= min(2, d.L) and (d.ids == d.pad).any()
        assert d.max_pos >= d.B * d.L


# =============================================================================== conditioning
H32 = 2.0 ** -24
COND = 0.5


def _cond(kind, out, ref, bound, what):
    r = K.ratio(out, ref, bound, what)
    assert r <= COND, f"{what}: fp32 evaluation of {kind} at {r:.3f} of the bound"


def _f32_ln(xs, gam, bet, eps):
    var, mean = torch.var_mean(xs, -1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    return mean[:, 0], rstd[:, 0], (xs - mean) * rstd * gam + bet


def _f32_ln_bwd(xs, dy, gam, mean, rstd):
    xhat = (xs - mean[:, None]) * rstd[:, None]
    g = dy * gam
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).flip(0).sum(0), dy.flip(0).sum(0)       # (the rows in reverse order)


def _ln_conditioning(d, what, zero_only=False):
    for use_res in (False, True):
        ref = R.layernorm_forward(d.x, d.res if use_res else None, d.gam, d.bet, K.EPS)
        xs = d.x.float() + d.res.float() if use_res else d.x.float()
        mean, rstd, y = _f32_ln(xs, d.gam, d.bet, K.EPS)
        _cond("y", y, ref.y, K.tensor_bound(ref.y, H32), what)
        _cond("mean", mean, ref.mean, K.vector_bound(ref.mean), what)
        _cond("rstd", rstd, ref.rstd, K.vector_bound(ref.rstd), what)
    ref = K.ln_bwd_ref(d.dt, d.rows, d.D, True, zero_only)
    dx, dg, db = _f32_ln_bwd(d.xsum.float(), d.dy.float(), d.gam, ref.mean32, ref.rstd32)
    _cond("dx", dx + d.addin.float(), ref.dx, K.tensor_bound(ref.dx, H32), what)
    zero = torch.zeros(d.D, dtype=F64)
    _cond("dgamma", dg, ref.dgamma, K.sum_bound(ref.sum_abs_gx, zero), what)
    _cond("dbeta", db, ref.dbeta, K.sum_bound(ref.sum_abs_g, zero), what)


@pytest.mark.parametrize("case", K.LN_CASES + K.LN_MANY, ids=K.LN_IDS + K.LN_MANY_IDS)
def test_layernorm_cases_are_well_posed_for_fp32(case):
    _ln_conditioning(K.ln_case(*case), f"layernorm {case}")
    if case[1] == 1:
        _ln_conditioning(K.ln_case(*case, zero_only=True), f"layernorm zero row {case}", True)


def _rms_conditioning(d, what):
    ref = R.rmsnorm_forward(d.x, d.w, K.EPS)
    x, dy = d.x.float(), d.dy.float()
    rstd = torch.rsqrt(x.pow(2).flip(1).sum(-1) / d.D + K.EPS)
    _cond("y", d.w * x * rstd[:, None], ref.y, K.tensor_bound(ref.y, H32), what)
    _cond("rstd", rstd, ref.rstd, K.vector_bound(ref.rstd), what)
    ref = R.rmsnorm_backward(d.x, d.dy, d.w, K.EPS, d.dx0, 1.0, d.dw0, 1.0)
    r = ref.rstd.float()[:, None]
    g = dy * d.w
    dx = r * (g - x * r * r * (g * x).mean(-1, keepdim=True)) + d.dx0.float()
    _cond("dx", dx, ref.dx, K.tensor_bound(ref.dx, H32), what)
    dw = (dy * x * r).flip(0).sum(0) + d.dw0
    _cond("dw", dw, ref.dw, K.sum_bound(ref.sum_abs_w, d.dw0.double()), what)


@pytest.mark.parametrize("case", K.RMS_CASES + K.RMS_MANY, ids=K.RMS_IDS + K.RMS_MANY_IDS)
def test_rmsnorm_cases_are_well_posed_for_fp32(case):
    _rms_conditioning(K.rms_case(*case), f"rmsnorm {case}")
    if case[1] == 1:
        _rms_conditioning(K.rms_case(*case, zero_only=True), f"rmsnorm zero row {case}")


@pytest.mark.parametrize("case", K.EMB_CASES, ids=K.EMB_IDS)
def test_embedding_cases_are_well_posed_for_fp32(case):
    d = K.emb_case(*case)
    what = f"embedding {case}"
    for tt in (d.tt, None):
        ref = R.embed_ln_forward(d.ids, tt, d.word, d.pos, d.type, d.gam, d.bet, K.EPS)
        trow = torch.zeros_like(d.ids) if tt is None else tt
        xs = (d.type[trow] + d.pos[:d.L][None] + d.word[d.ids]).view(d.rows, d.D)
        mean, rstd, y = _f32_ln(xs, d.gam, d.bet, K.EPS)
        _cond("xsum", xs, ref.xsum, K.tensor_bound(ref.xsum, H32), what)
        _cond("y", y, ref.y, K.tensor_bound(ref.y, H32), what)
        _cond("mean", mean, ref.mean, K.vector_bound(ref.mean), what)
        _cond("rstd", rstd, ref.rstd, K.vector_bound(ref.rstd), what)
        ref = R.embed_backward(d.ids, tt, d.dsum, d.pad, d.vocab, d.max_pos)
        ds = d.dsum.float().view(d.B, d.L, d.D)
        keep = (d.ids != d.pad).float()[..., None]
        dword = d.pre[0].clone().index_add_(0, d.ids.flatten().flip(0),
                                            (ds * keep).view(d.rows, d.D).flip(0))
        dpos = d.pre[1].clone()
        dpos[:d.L] += ds.flip(0).sum(0)
        dtyp = d.pre[2].clone().index_add_(0, trow.flatten().flip(0), ds.view(d.rows, d.D).flip(0))
        pre = [p.double() for p in d.pre]
        _cond("dword", dword, ref.dword + pre[0], K.sum_bound(ref.abs_word, pre[0]), what)
        _cond("dpos", dpos, ref.dpos + pre[1], K.sum_bound(ref.abs_pos, pre[1]), what)
        _cond("dtype", dtyp, ref.dtype + pre[2], K.sum_bound(ref.abs_type, pre[2]), what)


@pytest.mark.parametrize("case", K.POOL_CASES, ids=K.POOL_IDS)
def test_pooling_cases_are_well_posed_for_fp32(case):
    d = K.pool_case(*case)
    what = f"pooling {case}"
    m = d.mask.float()
    inv = 1.0 / m.sum(1, keepdim=True).clamp(min=1e-6)
    ref = R.masked_mean(d.h, d.mask)
    _cond("masked_mean", (d.h.float() * m[..., None]).flip(1).sum(1) * inv, ref,
          K.tensor_bound(ref, H32), what)
    ref = R.masked_mean_backward(d.dout, d.mask, d.L)
    _cond("masked_mean bwd", d.dout.float()[:, None] * (m * inv)[..., None], ref,
          K.tensor_bound(ref, H32), what)
    ref = R.embed_mean(d.ids, d.mask, d.table)
    _cond("embed_mean", (d.table[d.ids] * m[..., None]).flip(1).sum(1) * inv, ref,
          K.tensor_bound(ref, H32), what)
    ref = R.embed_mean_backward(d.ids, d.mask, d.dout, d.vocab)
    terms = (d.dout.float()[:, None] * (m * inv)[..., None]).view(-1, d.D)
    pre = d.pre.double()
    _cond("embed_mean bwd", d.pre.clone().index_add_(0, d.ids.flatten().flip(0), terms.flip(0)),
          ref.dtable + pre, K.sum_bound(ref.sum_abs, pre), what)
    ref = R.scatter(d.ids.flatten(), d.dtok, d.vocab)
    _cond("scatter", d.pre.clone().index_add_(0, d.ids.flatten().flip(0), d.dtok.float().flip(0)),
          ref.dtable + pre, K.sum_bound(ref.sum_abs, pre), what)
