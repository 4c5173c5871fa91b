"""fp64 CPU reference for the BatchNorm entry points of csrc/norm.hip, written from the
definitions (torch only): the forward, the backward as torch.autograd through that forward,
and the host-side mirrors of the data layouts the kernels read and write (statistics slabs,
1-bit ReLU masks, pool argmax bytes, bn_layout's slab count).  Inputs are the tensors the
kernel sees, already rounded to the compute dtype; everything here is computed in double."""
from types import SimpleNamespace

import torch

BN_NT = 256      # csrc/norm.hip: threads per reduce block
FIN_WIDE = 512   # csrc/norm.hip fin_wide(): above this many slabs the wide finalize runs
FIN_REGS = 4096  # 256 threads x FIN_PER: above this many slabs the wide finalize re-reads memory


# ------------------------------------------------------------------------------ layout
def _layout(rows, C, vec):
    """csrc/norm.hip bn_layout(rows, C, vec): (row threads per block, rows per block, row
    slabs).  A reduce thread visits rows_per_block / row threads rows of its slab."""
    cv = C // vec
    ct = min(cv, 64)
    rt = BN_NT // ct
    cgroups = (cv + ct - 1) // ct
    target = max(1, 2048 // cgroups)
    rpb = max((rows + target - 1) // target, rt)
    rpb = (rpb + rt - 1) // rt * rt
    return rt, rpb, (rows + rpb - 1) // rpb


def _rblocks(rows, C, vec):
    """Row slabs of csrc/norm.hip bn_layout(rows, C, vec)."""
    return _layout(rows, C, vec)[2]


def workspace_size(rows, C):
    """mmdx_bn_workspace_size: the larger layout's (mean, M2) slabs plus 5 C coefficients, over
    the vector widths C is a multiple of (4: fp32, 8: bf16); 0 if there is none."""
    nb = max([_rblocks(rows, C, vec) for vec in (4, 8) if C > 0 and C % vec == 0], default=0)
    return nb * C * 8 + 5 * C * 4 if nb else 0


def _wide_rows(C):
    """The fewest rows (plus a ragged tail) whose slab count exceeds fin_wide() in both the
    bf16 and the fp32 layout."""
    import mmdx._lib as L
    rt8 = BN_NT // min(C // 8, 64)
    rows = (FIN_WIDE + 1) * rt8 + 5
    assert _rblocks(rows, C, 8) > FIN_WIDE and _rblocks(rows, C, 4) > FIN_WIDE
    # the mirror above against the library: its workspace holds max(slabs) * C pairs + 5 C
    nb = max(_rblocks(rows, C, 4), _rblocks(rows, C, 8))
    assert L.lib().mmdx_bn_workspace_size(rows, C) == nb * C * 8 + 5 * C * 4
    return rows


# ------------------------------------------------------------------------------ forward
def _vec(t, C, fill):
    return torch.full((C,), fill, dtype=torch.float64) if t is None else t.double()


def bn_forward(x, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1,
               eps=1e-5, residual=None, relu=False, train=True):
    """BatchNorm2d over [rows, C] (+ residual)(+ ReLU).  Train: batch mean and biased variance
    normalise, running_var takes the unbiased one; eval: the running statistics normalise.
    Returns mean, var, rstd, running_mean, running_var (updated in train mode), scale, shift,
    pre (the value the ReLU sees) and y, all fp64."""
    x = x.double()
    rows, C = x.shape
    g, b = _vec(gamma, C, 1.0), _vec(beta, C, 0.0)
    rm = None if running_mean is None else running_mean.double()
    rv = None if running_var is None else running_var.double()
    if train:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        if rm is not None:
            unbiased = var * rows / (rows - 1) if rows > 1 else var
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * unbiased
    else:
        mean, var = rm, rv
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = (x - mean) * rstd * g + b
    if residual is not None:
        pre = pre + residual.double()
    y = torch.clamp(pre, min=0.0) if relu else pre
    scale = g * rstd
    return SimpleNamespace(mean=mean, var=var, rstd=rstd, running_mean=rm, running_var=rv,
                           scale=scale, shift=b - mean * scale, pre=pre, y=y)


# ------------------------------------------------------------------------------ backward
def bn_backward(x, dy, gamma=None, pos=None, train=True, eps=1e-5, running_mean=None,
                running_var=None, save_mean=None, save_rstd=None):
    """torch.autograd of sum(dy * out) through out = gate(bn(x) + residual) in double, where
    gate keeps the elements of the boolean tensor `pos` (None: no ReLU) — the ReLU decision is
    an input, so each kernel mode is checked against the decision it is documented to use.
    Train mode differentiates through the batch statistics; eval mode holds the running
    statistics constant.  save_mean / save_rstd (train mode, optional): the rounded batch
    statistics the kernel is handed — they replace the VALUES of the batch mean and rstd in
    the graph (the derivative still flows through the batch statistics), so the reference is
    evaluated at the kernel's own inputs: xhat = (x - save_mean) * save_rstd is ill-conditioned
    in save_mean wherever x is close to it.  Returns dx, d_residual, dgamma, dbeta and, per
    channel, sum_abs_g = sum_r |g| and sum_abs_gx = sum_r |g * xhat| (g = the gated dy)."""
    rows, C = x.shape
    xr = x.double().clone().requires_grad_(True)
    res = torch.zeros(rows, C, dtype=torch.float64, requires_grad=True)
    gam = _vec(gamma, C, 1.0).clone().requires_grad_(True)
    bet = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    if train:
        mean = xr.mean(0)
        rstd = 1.0 / torch.sqrt(((xr - mean) ** 2).mean(0) + eps)
        if save_mean is not None:
            mean = mean + (save_mean.double() - mean).detach()
            rstd = rstd * (save_rstd.double() / rstd).detach()
    else:
        mean, rstd = running_mean.double(), 1.0 / torch.sqrt(running_var.double() + eps)
    xhat = (xr - mean) * rstd
    out = xhat * gam + bet + res
    if pos is not None:
        out = torch.where(pos, out, torch.zeros_like(out))
    out.backward(dy.double())
    g = res.grad
    return SimpleNamespace(dx=xr.grad, d_residual=g, dgamma=gam.grad, dbeta=bet.grad,
                           sum_abs_g=g.abs().sum(0),
                           sum_abs_gx=(g * xhat.detach()).abs().sum(0))


# ------------------------------------------------------------------------------ slabs
def slab_stats(x, stat_rows):
    """(mean, M2) of each consecutive stat_rows-row slab of x [rows, C] (the last one short), as
    the conv epilogues and bn_stats_kernel hand them to the finalize: fp32 [C][blocks][2]."""
    x = x.double()
    rows, C = x.shape
    full = (rows - 1) // stat_rows          # slabs of exactly stat_rows rows; then the last one
    parts = []
    for s in (x[:full * stat_rows].view(full, stat_rows, C), x[None, full * stat_rows:]):
        m = s.mean(1, keepdim=True)
        parts.append(torch.stack([m[:, 0], ((s - m) ** 2).sum(1)], dim=-1))   # [slabs][C][2]
    return torch.cat(parts).permute(1, 0, 2).float().contiguous()


def merge_slabs(part, stat_rows, rows):
    """The two-level decomposition in fp64: mean = sum n_b mean_b / rows and
    M2 = sum (M2_b + n_b (mean_b - mean)^2) over slabs of n_b rows."""
    part = part.double()
    nblk = part.shape[1]
    n = torch.full((nblk,), float(stat_rows), dtype=torch.float64)
    n[-1] = rows - (nblk - 1) * stat_rows
    mean = (part[..., 0] * n).sum(1) / rows
    m2 = (part[..., 1] + n * (part[..., 0] - mean[:, None]) ** 2).sum(1)
    return mean, m2


def split_totals(sum_g, sum_gx, nblk, generator):
    """The backward totals (sum g, sum g*xhat) of each channel as nblk fp32 pieces
    [C][nblk][2] that add up to them (random positive shares, so no piece exceeds the total)."""
    tot = torch.stack([sum_g.double(), sum_gx.double()], dim=-1)          # [C][2]
    w = torch.rand(tot.shape[0], nblk, 2, generator=generator, dtype=torch.float64) + 0.1
    return (w / w.sum(1, keepdim=True) * tot[:, None, :]).float().contiguous()


# ------------------------------------------------------------------------------ ReLU bit mask
def pack_mask(pos, vec):
    """[rows, C] booleans -> one byte per 16-byte vector (vec elements), bit e = element e."""
    rows, C = pos.shape
    bits = pos.view(rows, C // vec, vec).to(torch.int32) << torch.arange(vec, dtype=torch.int32)
    return bits.sum(-1).to(torch.uint8)


def unpack_mask(mask, vec):
    """The inverse of pack_mask: [rows, C / vec] bytes -> [rows, C] booleans."""
    rows = mask.shape[0]
    bits = (mask.to(torch.int32)[..., None] >> torch.arange(vec, dtype=torch.int32)) & 1
    return bits.view(rows, -1).bool()


# ------------------------------------------------------------------------------ pool
def pool_scatter(dy_pooled, argmax, H, W, pad, dtype):
    """dL/d(pool input) [N, H, W, C] of the 3x3 / stride-2 max pool: every pooled gradient
    element goes to the input pixel its argmax byte names (tap = 3 * row + column inside the
    window whose corner is (2 i - pad, 2 j - pad)), summed where windows overlap and rounded
    to the compute dtype — the gradient mmdx_bn_bwd_pool is documented to see."""
    N, P, Q, C = dy_pooled.shape
    am = argmax.long()
    n, i, j, c = torch.meshgrid(torch.arange(N), torch.arange(P), torch.arange(Q),
                                torch.arange(C), indexing="ij")
    h = 2 * i - pad + am // 3
    w = 2 * j - pad + am % 3
    assert (am < 9).all() and (h >= 0).all() and (h < H).all() and (w >= 0).all() and (w < W).all()
    out = torch.zeros(N, H, W, C, dtype=torch.float64)
    out.index_put_((n, h, w, c), dy_pooled.double(), accumulate=True)
    return out.to(dtype).double()
