"""fp64 CPU reference for the row-wise normalisation kernels (LayerNorm of csrc/norm.hip, RMSNorm
of csrc/t5.hip) and the memory-bound token kernels of csrc/text.hip and csrc/vit.hip, written
from the definitions (torch only).  Inputs are the tensors the kernel sees, already rounded to
the compute dtype; everything here is computed in double.  Every backward is torch.autograd
through the fp64 forward of this file, so a forward and its backward are not two copies of one
hand-derived formula.  The host-side mirrors at the end repeat the kernels' launch constants."""
from types import SimpleNamespace

import torch

F64 = torch.float64

# ------------------------------------------------------------------------------ host mirrors
LN_RPW_MIN = 4       # csrc/norm.hip: the fewest rows per wave of ln_bwd_kernel (MMDX_LN_BWD_RPW)
LN_RPW = (4, 8)      # the two values of MMDX_LN_BWD_RPW; 8 is the default
LN_WAVES = 4         # waves (rows in flight) per 256-thread block, forward and backward
LN_FIN_LANES = 32    # csrc/norm.hip: lanes that stride the partial blocks in the finalize
LN_FIN_UNROLL = 8    # ... and the unroll factor of that strided loop
LN_MAXV = 4          # 16-byte vectors per lane: D <= 64 * LN_MAXV * VEC
RMS_BWD_ROWS = 32    # csrc/t5.hip: rows per block of rms_bwd_kernel (4 waves x 8 rows)
EMB_MAXD = 1024      # csrc/text.hip: 64 lanes x EMB_MAXE elements
GRID_CAP = 8192      # common.h grid_for / vit.hip vgrid: at most this many 256-thread blocks


def vec_width(dtype):
    """Elements of a 16-byte vector."""
    return 4 if dtype == torch.float32 else 8


def ln_max_d(dtype):
    return 64 * LN_MAXV * vec_width(dtype)


def ln_partial_blocks(rows, rpw):
    """Blocks of ln_bwd_kernel = partial (dgamma, dbeta) rows the finalize sums."""
    return (rows + LN_WAVES * rpw - 1) // (LN_WAVES * rpw)


def layernorm_workspace_size(rows, D):
    """mmdx_layernorm_workspace_size: [blocks at LN_RPW_MIN][2][D] fp32."""
    return ln_partial_blocks(rows, LN_RPW_MIN) * 2 * D * 4


def rmsnorm_workspace_size(rows, D):
    """mmdx_rmsnorm_workspace_size: [blocks][D] fp32."""
    return (rows + RMS_BWD_ROWS - 1) // RMS_BWD_ROWS * D * 4


# ------------------------------------------------------------------------------ LayerNorm
def _ln(xs, gamma, beta, eps, save_mean=None, save_rstd=None):
    mean = xs.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + eps)
    if save_mean is not None:   # the values change, the derivative still flows through the row
        mean = mean + (save_mean.double()[..., None] - mean).detach()
        rstd = rstd * (save_rstd.double()[..., None] / rstd).detach()
    xhat = (xs - mean) * rstd
    return mean[..., 0], rstd[..., 0], xhat, xhat * gamma + beta


def layernorm_forward(x, residual, gamma, beta, eps):
    """y = LayerNorm(x + residual) over the last axis with the biased variance.  Returns xsum
    (= x + residual, the tensor the backward reads), mean, rstd (per row) and y."""
    xs = x.double() if residual is None else x.double() + residual.double()
    mean, rstd, _, y = _ln(xs, gamma.double(), beta.double(), eps)
    return SimpleNamespace(xsum=xs, mean=mean, rstd=rstd, y=y)


def layernorm_backward(xsum, dy, gamma, eps, addin=None, save_mean=None, save_rstd=None):
    """torch.autograd of sum(dy * LayerNorm(xsum)) in double.  Returns dx (+ addin, a residual
    branch's gradient), dgamma, dbeta, mean and rstd and, per channel, sum_abs_gx =
    sum_r |dy * xhat| and sum_abs_g = sum_r |dy|.

    save_mean / save_rstd (optional): the fp32-rounded row statistics the kernel is handed.
    They replace the VALUES of mean and rstd in the graph, as in bn_ref.bn_backward, so the
    reference is evaluated at the kernel's own inputs: xhat = (x - save_mean) * save_rstd is
    ill-conditioned in save_mean wherever x is close to it, and a one-row dgamma is that
    single product."""
    xs = xsum.double().clone().requires_grad_(True)
    gam = gamma.double().clone().requires_grad_(True)
    bet = torch.zeros_like(gam, requires_grad=True)
    mean, rstd, xhat, y = _ln(xs, gam, bet, eps, save_mean, save_rstd)
    y.backward(dy.double())
    dx = xs.grad if addin is None else xs.grad + addin.double()
    lead = tuple(range(dy.dim() - 1))
    return SimpleNamespace(dx=dx, dgamma=gam.grad, dbeta=bet.grad, mean=mean.detach(),
                           rstd=rstd.detach(),
                           sum_abs_gx=(dy.double() * xhat.detach()).abs().sum(lead),
                           sum_abs_g=dy.double().abs().sum(lead))


# ------------------------------------------------------------------------------ RMSNorm
def _rms(x, w, eps):
    rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    return rstd, w * (x * rstd)


def rmsnorm_forward(x, w, eps):
    """T5LayerNorm: y = w * x * rsqrt(mean(x^2) + eps); no mean, no bias.  Returns rstd, y."""
    rstd, y = _rms(x.double(), w.double(), eps)
    return SimpleNamespace(rstd=rstd[..., 0], y=y)


def rmsnorm_backward(x, dy, w, eps, dx0=None, beta=0.0, dw0=None, beta_acc=0.0):
    """torch.autograd of sum(dy * rmsnorm(x)) in double; dx = grad + beta * dx0 (beta = 1 adds
    onto a residual gradient already in the buffer), dw = grad + beta_acc * dw0.  Also rstd and
    sum_abs_w = sum_r |dy * x * rstd| per channel."""
    xr = x.double().clone().requires_grad_(True)
    wr = w.double().clone().requires_grad_(True)
    rstd, y = _rms(xr, wr, eps)
    y.backward(dy.double())
    dx, dw = xr.grad, wr.grad
    if beta != 0.0:
        dx = dx + beta * dx0.double()
    if beta_acc != 0.0:
        dw = dw + beta_acc * dw0.double()
    return SimpleNamespace(dx=dx, dw=dw, rstd=rstd.detach()[..., 0],
                           sum_abs_w=(dy.double() * xr.detach() * rstd.detach()).abs().sum(0))


# ------------------------------------------------------------------------------ BERT embeddings
def _type_rows(ids, tt):
    """Row of the 2-row token-type table each token uses.  The kernels send tt == 1 to row 1 and
    everything else — any other value, and tt == NULL (None) — to row 0."""
    return torch.zeros_like(ids) if tt is None else (tt == 1).long()


def _embed_sum(ids, tt, word, pos, type_tab, keep=None):
    B, L = ids.shape
    w = word[ids]
    if keep is not None:
        w = w * keep[..., None]
    return w + pos[torch.arange(L)][None] + type_tab[_type_rows(ids, tt)]


def embed_ln_forward(ids, tt, word, pos, type, gamma, beta, eps):
    """BertEmbeddings: xsum[b, l] = word[ids[b, l]] + pos[l] + type[tt[b, l] == 1] and
    y = LayerNorm(xsum).  ids, tt: [B, L] int64 (tt None: row 0, as the kernel treats a NULL
    tt; see _type_rows for values other than 0 and 1).  Returns xsum, mean, rstd, y with rows
    flattened to [B * L]."""
    B, L = ids.shape
    xs = _embed_sum(ids, tt, word.double(), pos.double(), type.double()).view(B * L, -1)
    mean, rstd, _, y = _ln(xs, gamma.double(), beta.double(), eps)
    return SimpleNamespace(xsum=xs, mean=mean, rstd=rstd, y=y)


def embed_backward(ids, tt, dsum, pad_id, vocab, max_pos=None):
    """The table gradients of sum(dsum * xsum) by autograd through _embed_sum: dword [vocab, D]
    (the row pad_id takes no gradient, nn.Embedding's padding_idx; pad_id = -1 names no row),
    dpos [max_pos, D] (rows >= L stay 0), dtype [2, D] (tt == 1 -> row 1, all else -> row 0).
    abs_word / abs_pos / abs_type: the same sums over |dsum|."""
    B, L = ids.shape
    D = dsum.shape[-1]
    max_pos = L if max_pos is None else max_pos
    keep = (ids != pad_id).double()
    out = []
    for g in (dsum.double().view(B, L, D), dsum.double().abs().view(B, L, D)):
        tabs = [torch.zeros(n, D, dtype=F64, requires_grad=True) for n in (vocab, max_pos, 2)]
        _embed_sum(ids, tt, *tabs, keep=keep).backward(g)
        out += [t.grad for t in tabs]
    return SimpleNamespace(dword=out[0], dpos=out[1], dtype=out[2], abs_word=out[3],
                           abs_pos=out[4], abs_type=out[5])


# ------------------------------------------------------------------------------ pooling, gather
COUNT_FLOOR = 1e-6   # the kernels divide by fmaxf(count, 1e-6f)


def _mean_weights(mask):
    m = mask.double()
    return m / torch.clamp(m.sum(-1, keepdim=True), min=COUNT_FLOOR)


def masked_mean(h, mask):
    """out[b] = sum_l mask[b, l] h[b, l] / max(sum_l mask[b, l], 1e-6).  h [B, L, D]."""
    return (h.double() * _mean_weights(mask)[..., None]).sum(1)


def masked_mean_backward(dout, mask, L):
    """dh [B, L, D] of sum(dout * masked_mean(h, mask)), by autograd."""
    B, D = dout.shape
    h = torch.zeros(B, L, D, dtype=F64, requires_grad=True)
    masked_mean(h, mask).backward(dout.double())
    return h.grad


def embed_mean(ids, mask, table):
    """masked_mean of the gathered rows table[ids]: [B, D]."""
    return masked_mean(table.double()[ids], mask)


def embed_mean_backward(ids, mask, dout, vocab):
    """dtable [vocab, D] of sum(dout * embed_mean(ids, mask, table)) by autograd, and sum_abs,
    the same sum over |dout| (the weights are non-negative)."""
    out = []
    for g in (dout.double(), dout.double().abs()):
        tab = torch.zeros(vocab, dout.shape[-1], dtype=F64, requires_grad=True)
        embed_mean(ids, mask, tab).backward(g)
        out.append(tab.grad)
    return SimpleNamespace(dtable=out[0], sum_abs=out[1])


def gather(ids, table):
    """out[i] = table[ids[i]]."""
    return table.double()[ids]


def scatter(ids, dout, vocab):
    """dtable [vocab, D] = the autograd of gather: dout's rows summed by id; and sum_abs."""
    out = []
    for g in (dout.double(), dout.double().abs()):
        tab = torch.zeros(vocab, dout.shape[-1], dtype=F64, requires_grad=True)
        gather(ids, tab).backward(g)
        out.append(tab.grad)
    return SimpleNamespace(dtable=out[0], sum_abs=out[1])


# ------------------------------------------------------------------------------ ViT pieces
def patchify(x, p):
    """x NCHW [N, C, H, W] -> [N * (H/p) * (W/p), C * p * p]: the p x p patches in row-major
    patch order, each flattened in (c, ky, kx) order (a Conv2d weight's [C][p][p])."""
    N, C, H, W = x.shape
    v = x.double().view(N, C, H // p, p, W // p, p)       # n c py ky px kx
    return v.permute(0, 2, 4, 1, 3, 5).reshape(N * (H // p) * (W // p), C * p * p)


def vit_tokens_fwd(emb, cls, pos):
    """tokens[n][0] = cls + pos[0]; tokens[n][1 + q] = emb[n][q] + pos[1 + q].
    emb [N, S - 1, D], cls [D], pos [S, D] -> [N, S, D]."""
    N, _, D = emb.shape
    return torch.cat([cls.double().expand(N, 1, D), emb.double()], dim=1) + pos.double()


def vit_tokens_bwd(dtok):
    """demb [N, S - 1, D] of sum(dtok * tokens), by autograd through vit_tokens_fwd."""
    N, S, D = dtok.shape
    emb = torch.zeros(N, S - 1, D, dtype=F64, requires_grad=True)
    vit_tokens_fwd(emb, torch.zeros(D, dtype=F64), torch.zeros(S, D, dtype=F64)).backward(
        dtok.double())
    return emb.grad


def rows_copy(src, src_ld, dst, dst_ld, rows, D):
    """dst[r * dst_ld + d] = src[r * src_ld + d] for d < D on flat buffers; the rest of dst is
    returned as it was."""
    out = dst.clone()
    r, d = torch.meshgrid(torch.arange(rows), torch.arange(D), indexing="ij")
    out[(r * dst_ld + d).flatten()] = src[(r * src_ld + d).flatten()]
    return out


def add(x, y):
    return x.double() + y.double()
