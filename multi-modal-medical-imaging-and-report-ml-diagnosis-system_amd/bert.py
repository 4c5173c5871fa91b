"""BERT-base encoder on the mmdx kernels, state_dict-identical to transformers' BertModel.

The reference builds it with `AutoModel.from_pretrained("bert-base-uncased")`
(training_pipeline.py:360) and calls it at TP:470/473; its arithmetic is transformers'
BertEmbeddings / BertLayer (modeling_bert.py).  Here each BertLayer is ONE autograd node:
fused QKV GEMM -> attention core (MFMA, in-LDS softmax) -> out-proj GEMM -> Add&LayerNorm ->
FFN up GEMM (+GELU epilogue) -> FFN down GEMM -> Add&LayerNorm, with a hand-sequenced
backward whose residual gradients are summed inside GEMM epilogues (beta = 1).  The layer
is written once, in xlayers (bert_fwd / bert_bwd): _BertLayerFn here issues it call by call
(inference, no_grad, a frozen encoder parameter), xplan records the same body as a launch
plan for the whole stack (training).
Hidden-state dropout runs inside the LayerNorm kernel in train mode; attention-probability
dropout (BertSelfAttention's, p = config.attention_probs_dropout_prob) is fused into the
attention kernel (counter-based hash, keep bit carried in the saved probabilities' sign).
RNG streams cannot match torch's, so parity runs use p = 0 on both sides; the dropout
arithmetic itself is checked against an explicit masked reference (tests/test_text_gpu.py).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib as L
from . import functional as F
from . import xlayers as XL
from . import xplan
from ._lib import call, ptr, stream
from .layers import Embedding, LayerNorm, Linear


class _Out(SimpleNamespace):
    pass


class _BertLayerFn(torch.autograd.Function):
    """One transformers BertLayer (post-LN): xlayers.bert_fwd / bert_bwd issued at once."""

    @staticmethod
    def forward(ctx, h, mask, cfg, *params):
        B, Ls, D = h.shape
        keep = any(ctx.needs_input_grad)
        ctx.c = c = SimpleNamespace(
            B=B, Ls=Ls, D=D, H=cfg.num_attention_heads, I=params[10].shape[0],
            eps=cfg.layer_norm_eps, p=cfg.p_hidden if cfg.training else 0.0,
            pa=float(cfg.p_attn) if (cfg.training and keep) else 0.0)
        be = XL.Eager(h.dtype, h.device, keep)
        h2, saved = XL.bert_fwd(be, 0, h.reshape(B * Ls, D), mask, params, c)
        if keep:
            XL.save(ctx, dict(saved, mask=mask))
        return h2.reshape(B, Ls, D)

    @staticmethod
    def backward(ctx, dh2):
        c, s = ctx.c, XL.load(ctx)
        x = s["x"]
        be = XL.Eager(x.dtype, x.device, True)
        table = XL.bert_grads(c.D, c.I)
        gd = be.grad_bufs(table)
        dh2 = F.cast(dh2.contiguous().reshape(x.shape), x.dtype)
        dx = XL.bert_bwd(be, s, dh2, s["mask"], gd, c)
        return (dx.reshape(c.B, c.Ls, c.D), None, None, *XL.in_param_order(table, gd, 16))


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, tt, word, pos, typ, gamma, beta, eps, T):
        B, Ls = ids.shape
        D = word.shape[1]
        dev = ids.device
        y = torch.empty((B, Ls, D), dtype=T, device=dev)
        xs = torch.empty((B, Ls, D), dtype=T, device=dev)
        mean = torch.empty(B * Ls, dtype=torch.float32, device=dev)
        rstd = torch.empty(B * Ls, dtype=torch.float32, device=dev)
        call("mmdx_embed_ln_fwd", L.dtype_code(T), ptr(ids), ptr(tt), B, Ls, D, ptr(word),
             ptr(pos), ptr(typ), ptr(gamma), ptr(beta), float(eps), ptr(y), ptr(xs), ptr(mean),
             ptr(rstd), stream())
        ctx.save_for_backward(ids, tt, xs, mean, rstd, gamma)
        ctx.shapes = (word.shape, pos.shape, typ.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        ids, tt, xs, mean, rstd, gamma = ctx.saved_tensors
        B, Ls = ids.shape
        D = xs.shape[-1]
        dy = F.cast(dy.contiguous(), xs.dtype)
        dx, dg, db = F.ln_bwd(xs, dy, gamma, mean, rstd)
        dev = ids.device
        ws, ps, ts = ctx.shapes
        dword = torch.zeros(ws, dtype=torch.float32, device=dev)
        dpos = torch.zeros(ps, dtype=torch.float32, device=dev)
        dtyp = torch.zeros(ts, dtype=torch.float32, device=dev)
        call("mmdx_embed_bwd", L.dtype_code(xs.dtype), ptr(ids), ptr(tt), B, Ls, D, ptr(dx),
             ptr(dword), ptr(dpos), ptr(dtyp), 0, stream())
        return None, None, dword, dpos, dtyp, dg, db, None, None


# ----------------------------------------------------------------------------- modules
class BertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = Embedding(cfg.vocab_size, cfg.hidden_size, padding_idx=0)
        self.position_embeddings = Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.token_type_embeddings = Embedding(cfg.type_vocab_size, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class BertSelfAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.query = Linear(cfg.hidden_size, cfg.hidden_size)
        self.key = Linear(cfg.hidden_size, cfg.hidden_size)
        self.value = Linear(cfg.hidden_size, cfg.hidden_size)


class _DenseLN(nn.Module):
    def __init__(self, din, dout, eps):
        super().__init__()
        self.dense = Linear(din, dout)
        self.LayerNorm = LayerNorm(dout, eps=eps)


class BertAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.self = BertSelfAttention(cfg)
        self.output = _DenseLN(cfg.hidden_size, cfg.hidden_size, cfg.layer_norm_eps)


class _Intermediate(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = Linear(cfg.hidden_size, cfg.intermediate_size)


class BertLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attention = BertAttention(cfg)
        self.intermediate = _Intermediate(cfg)
        self.output = _DenseLN(cfg.intermediate_size, cfg.hidden_size, cfg.layer_norm_eps)

    def params(self):
        s, o = self.attention.self, self.attention.output
        return [s.query.weight, s.query.bias, s.key.weight, s.key.bias, s.value.weight,
                s.value.bias, o.dense.weight, o.dense.bias, o.LayerNorm.weight, o.LayerNorm.bias,
                self.intermediate.dense.weight, self.intermediate.dense.bias,
                self.output.dense.weight, self.output.dense.bias, self.output.LayerNorm.weight,
                self.output.LayerNorm.bias]


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(cfg) for _ in range(cfg.num_hidden_layers)])


class _Pooler(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = Linear(cfg.hidden_size, cfg.hidden_size)


def bert_base_config(num_hidden_layers=12, dropout=0.1):
    """BertConfig() defaults = bert-base-uncased geometry (transformers configuration_bert)."""
    return SimpleNamespace(vocab_size=30522, hidden_size=768, num_hidden_layers=num_hidden_layers,
                           num_attention_heads=12, intermediate_size=3072,
                           hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout,
                           max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                           initializer_range=0.02, pad_token_id=0,
                           _name_or_path="bert-base-uncased")


class BertModel(nn.Module):
    def __init__(self, config=None):
        super().__init__()
        self.config = config or bert_base_config()
        self.embeddings = BertEmbeddings(self.config)
        self.encoder = _Encoder(self.config)
        self.pooler = _Pooler(self.config)
        self.compute_dtype = torch.float32
        self._init_weights()

    @classmethod
    def from_name(cls, name: str):
        """'bert-base-uncased' (12 layers) or 'bert-base-uncased@N' (first N layers) —
        built offline from the BertConfig defaults; a local HF directory's weights can be
        loaded with load_state_dict (keys are identical)."""
        layers = 12
        if "@" in name:
            name, n = name.split("@", 1)
            layers = int(n)
        return cls(bert_base_config(layers))

    def _init_weights(self):  # BertPreTrainedModel._init_weights
        std = self.config.initializer_range
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0.0, std)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, 0.0, std)
                if m.padding_idx is not None:
                    with torch.no_grad():
                        m.weight[m.padding_idx].zero_()
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward_layers(self, input_ids, attention_mask, token_type_ids, keep, on_layer=None):
        """The embeddings and the eager layer bodies (xlayers.bert_fwd, the launches of forward()
        under no_grad in eval mode: p = pa = 0) without autograd: -> (last hidden state
        [B, Ls, D], c, the per-layer `saved` dicts when keep).  on_layer(li, saved) runs after
        each layer.  The counterpart of VitTrunk.forward_blocks, for mmdx.explain."""
        T = self.compute_dtype
        L.require_device(input_ids)
        with torch.no_grad():
            ids = input_ids.long().contiguous()
            B, Ls = ids.shape
            mask = (attention_mask.long().contiguous() if attention_mask is not None
                    else torch.ones_like(ids))
            tt = (token_type_ids.long().contiguous() if token_type_ids is not None
                  else torch.zeros_like(ids))
            e = self.embeddings
            h = _EmbedFn.apply(ids, tt, e.word_embeddings.weight, e.position_embeddings.weight,
                               e.token_type_embeddings.weight, e.LayerNorm.weight,
                               e.LayerNorm.bias, self.config.layer_norm_eps, T)
            D = h.shape[-1]
            c = SimpleNamespace(B=B, Ls=Ls, D=D, H=self.config.num_attention_heads,
                                I=self.config.intermediate_size, eps=self.config.layer_norm_eps,
                                p=0.0, pa=0.0)
            be = XL.Eager(T, h.device, keep)
            h = h.reshape(B * Ls, D)
            kept = []
            for li, layer in enumerate(self.encoder.layer):
                h, saved = XL.bert_fwd(be, 0, h, mask, layer.params(), c)
                if on_layer is not None:
                    on_layer(li, saved)
                if keep:
                    kept.append(saved)
        return h.reshape(B, Ls, D), c, kept

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, return_dict=True):
        T = self.compute_dtype
        L.require_device(input_ids)
        ids = input_ids.long().contiguous()
        B, Ls = ids.shape
        mask = (attention_mask.long().contiguous() if attention_mask is not None
                else torch.ones_like(ids))
        tt = (token_type_ids.long().contiguous() if token_type_ids is not None
              else torch.zeros_like(ids))
        e = self.embeddings
        h = _EmbedFn.apply(ids, tt, e.word_embeddings.weight, e.position_embeddings.weight,
                           e.token_type_embeddings.weight, e.LayerNorm.weight, e.LayerNorm.bias,
                           self.config.layer_norm_eps, T)
        cfg = SimpleNamespace(num_attention_heads=self.config.num_attention_heads,
                              layer_norm_eps=self.config.layer_norm_eps,
                              p_hidden=self.config.hidden_dropout_prob,
                              p_attn=self.config.attention_probs_dropout_prob,
                              training=self.training)
        # the whole layer stack as one native launch plan per direction (xplan); the eager
        # per-layer nodes when gradients are off or some encoder parameter is frozen
        params = [q for layer in self.encoder.layer for q in layer.params()]
        keep = torch.is_grad_enabled()
        pcfg = SimpleNamespace(heads=self.config.num_attention_heads,
                               eps=self.config.layer_norm_eps,
                               p=float(self.config.hidden_dropout_prob) if self.training else 0.0,
                               pa=(float(self.config.attention_probs_dropout_prob)
                                   if self.training and keep else 0.0))
        out = xplan.run_stack("bert", h, mask, pcfg, self.encoder, params) if params else None
        if out is not None:
            return _Out(last_hidden_state=out)
        for layer in self.encoder.layer:
            h = _BertLayerFn.apply(h, mask, cfg, *layer.params())
        return _Out(last_hidden_state=h)
