"""OpenAI-CLIP ViT two-tower shape (plumbing): random-init, with the parameter names, shapes,
dtypes, `named_parameters()` order and block contract of CoOp/clip/model.py:167-368 (the ResNet
backbones have no `resblocks` and are not built).  What a pruner touches is mirrored:
`visual.transformer.resblocks` / `transformer.resblocks` are `nn.Sequential`s whose blocks take and
return `[L, N, D]`, and each block exposes `attn` (an `nn.MultiheadAttention`: `in_proj_weight`,
`in_proj_bias`, `out_proj`), `attention(x)`, `attn_mask` (additive causal `-inf` upper triangle in
the text tower, `None` in the visual one), `ln_1`, `mlp.c_fc`, `mlp.c_proj`, `ln_2`.

On the CPU, with autograd, or in fp32 a block runs the reference's op chain through
`nn.MultiheadAttention`.  On the GPU under `no_grad` in fp16 the attention between the in- and the
out-projection is `fused.mha_attention` (csrc/mha_attention.hip: the in-projection's `[L, N, 3D]`
output read in place, causal in the text tower), and the patch embedding is one GEMM
(`fused.patches_gemm`, no MIOpen: DESIGN §5).  Where the kernel refuses a shape (head width other
than 64, more than 224 tokens) the block stays on `nn.MultiheadAttention`.

`clip_wanda_pruner` (pruners/clip.py) and `clip_sparsegpt_pruner` (pruners/clip_sparsegpt.py) prune
these towers.  While stage 2 hooks a block, the
block reports the operands of the two attention projections, which no `nn.Linear` hook can see
(`_stat_sink`, off by default: `attention()` then is the code above, unchanged): `ln_1(x)` for the
in-projection, and for the out-projection the output of the reference's UNMASKED side copy of the
attention (CoOp/trainers/pruners/wanda_pruner.py:300-322) — on the GPU in fp16 as the column
statistic `fused.mha_attention_colsq` leaves (in the visual tower the same kernel call that
produces the block's output), everywhere else as the reference's literal op chain in torch.  A sink
that answers `takes_kernel_operand()` (SparseGPT: a Hessian needs the rows themselves) gets the
unmasked `fused.mha_attention` output instead of the statistic, as a view of `[L, N, D]`.

Not here yet: `stage_plan()`."""
import math
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


class LayerNorm(nn.LayerNorm):
    """fp32 statistics whatever the activation's dtype (model.py:153-159)."""

    def forward(self, x):
        return super().forward(x.float()).to(x.dtype)


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


def causal_mask(context):
    return torch.full((context, context), float("-inf")).triu_(1)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model, n_head, attn_mask=None):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)),
                                              ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)
        self.attn_mask = attn_mask

    def _mask_is_causal(self, L):
        """None / the causal triangle -> False / True; any other mask -> None (no fused path).
        Checked once per mask object and length."""
        m = self.attn_mask
        if m is None:
            return False
        key = (id(m), L)
        held = self.__dict__.get("_causal_checked")
        if held is None or held[0] != key:
            ok = tuple(m.shape) == (L, L) and bool(torch.equal(m.float().cpu(), causal_mask(L)))
            held = self.__dict__["_causal_checked"] = (key, ok)
        return True if held[1] else None

    def _fused_attention(self, x):
        a = self.attn
        if (torch.is_grad_enabled() or x.device.type != "cuda" or x.dtype != torch.float16
                or x.dim() != 3 or a.in_proj_weight is None or a.in_proj_weight.dtype != torch.float16):
            return None
        causal = self._mask_is_causal(x.shape[0])
        if causal is None:
            return None
        from . import fused
        qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)             # [L, N, 3D], rows [3, heads, head_dim]
        y = fused.mha_attention(qkv, a.num_heads, a.head_dim ** -0.5, causal=causal, seq_first=True)
        return None if y is None else a.out_proj(y)

    # stage 2 of the CLIP pruners sets this on the block it hooks (pruners/clip.py::_AttentionSites,
    # pruners/clip_sparsegpt.py::_HessianSites)
    _stat_sink = None

    def _side_attention(self, x):
        """The reference's `hacky_attn` up to its `proj` (wanda_pruner.py:69-101 with this block's
        in-projection as `qkv`, :302-306): no mask in either tower, `q * scale` before the
        product, every op in the activation's dtype.  [L, N, D] -> `proj`'s input [N, L, D]."""
        a = self.attn
        x = x.permute(1, 0, 2)
        B, N, C = x.shape
        qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)
        qkv = qkv.reshape(B, N, 3, a.num_heads, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        q = q * (a.head_dim ** -0.5)
        attn = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        return (attn @ v).transpose(1, 2).reshape(B, N, -1)

    def _reporting_attention(self, x, sink):
        """`attention(x)` of a hooked block: the same result, and both projections' operands (or
        the out-projection's finished statistic) handed to `sink`."""
        a = self.attn
        sink.operand("attn.in_proj", x.permute(1, 0, 2))
        fused_ok = not (torch.is_grad_enabled() or x.device.type != "cuda" or x.dtype != torch.float16
                        or x.dim() != 3 or a.in_proj_weight is None
                        or a.in_proj_weight.dtype != torch.float16)
        causal = self._mask_is_causal(x.shape[0]) if fused_ok else None
        if causal is not None and getattr(sink, "takes_kernel_operand", bool)():
            # the out-projection's OPERAND from the kernels (a Hessian needs the rows, not their
            # column norms): in the visual tower it is the block's own attention output; in the text
            # tower one more, unmasked, call beside the causal forward.  [L, N, D] as it lies.
            from . import fused
            qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)         # [L, N, 3D]
            scale = a.head_dim ** -0.5
            y = fused.mha_attention(qkv, a.num_heads, scale, causal=causal, seq_first=True)
            side = y if (y is None or not causal) else fused.mha_attention(
                qkv, a.num_heads, scale, causal=False, seq_first=True)
            if side is not None:
                sink.operand("attn.out_proj", side.permute(1, 0, 2))
                return a.out_proj(y)
        elif causal is not None and sink.takes_statistic():
            from . import fused
            qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)         # [L, N, 3D]
            scale = a.head_dim ** -0.5
            if causal:      # the forward is masked, the statistic is not: a second, store-free pass
                y = fused.mha_attention(qkv, a.num_heads, scale, causal=True, seq_first=True)
                res = None if y is None else fused.mha_attention_colsq(qkv, a.num_heads, scale, out=False,
                                                                      seq_first=True)
            else:
                res = fused.mha_attention_colsq(qkv, a.num_heads, scale, out=True, seq_first=True)
                y = None if res is None else res[0]
            if res is not None:
                sink.statistic("attn.out_proj", res[1], x.shape[1])
                return a.out_proj(y)
        sink.operand("attn.out_proj", self._side_attention(x))
        return self._plain_attention(x)

    def attention(self, x):
        sink = self._stat_sink
        if sink is not None:
            return self._reporting_attention(x, sink)
        return self._plain_attention(x)

    def _plain_attention(self, x):
        y = self._fused_attention(x)
        if y is not None:
            return y
        if self.attn_mask is not None:
            self.attn_mask = self.attn_mask.to(dtype=x.dtype, device=x.device)
        return self.attn(x, x, x, need_weights=False, attn_mask=self.attn_mask)[0]

    def forward(self, x):
        x = x + self.attention(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, attn_mask=None):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask) for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class VisionTransformer(nn.Module):
    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.output_dim = input_resolution, output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.conv1._ecoflap_gemm_form = True        # its GPU forward is `embed` below, not MIOpen's
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def embed(self, x):
        """image -> [N, L, D] after ln_pre."""
        if x.is_cuda:
            from . import fused
            x = fused.patches_gemm(self.conv1, x)
        else:
            x = self.conv1(x)
            x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
        cls = self.class_embedding.to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype, device=x.device)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        return self.ln_pre(x)

    def forward(self, x):
        x = self.embed(x).permute(1, 0, 2)          # NLD -> LND
        x = self.transformer(x).permute(1, 0, 2)
        x = self.ln_post(x[:, 0, :])
        return x @ self.proj


class CLIP(nn.Module):
    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size,
                 context_length, vocab_size, transformer_width, transformer_heads, transformer_layers,
                 vision_heads=None):
        super().__init__()
        self.context_length = context_length
        self.visual = VisionTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                        vision_heads or vision_width // 64, embed_dim)
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads,
                                       attn_mask=causal_mask(context_length))
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self._init()

    def _init(self):
        """The standard deviations of model.py:295-322."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        w, n = self.transformer.width, self.transformer.layers
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=w ** -0.5)
            nn.init.normal_(blk.attn.out_proj.weight, std=(w ** -0.5) * ((2 * n) ** -0.5))
            nn.init.normal_(blk.mlp.c_fc.weight, std=(2 * w) ** -0.5)
            nn.init.normal_(blk.mlp.c_proj.weight, std=(w ** -0.5) * ((2 * n) ** -0.5))
        nn.init.normal_(self.text_projection, std=w ** -0.5)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image):
        return self.visual(image.type(self.dtype))

    def encode_text(self, text):
        x = self.token_embedding(text).type(self.dtype) + self.positional_embedding.type(self.dtype)
        x = self.transformer(x.permute(1, 0, 2)).permute(1, 0, 2)
        x = self.ln_final(x).type(self.dtype)
        # features at the end-of-text token = the highest id of each sequence (model.py:350)
        return x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ self.text_projection

    def forward(self, image, text):
        img, txt = self.encode_image(image), self.encode_text(text)
        img = img / img.norm(dim=-1, keepdim=True)
        txt = txt / txt.norm(dim=-1, keepdim=True)
        scale = self.logit_scale.exp()
        return scale * img @ txt.t(), scale * txt @ img.t()


def half_weights(model):
    """fp16 where `convert_weights` (model.py:371-392) puts it: Conv / Linear weights and biases,
    the attention's in-projection, `proj` and `text_projection`; LayerNorms, embeddings and
    `logit_scale` stay fp32."""
    for m in model.modules():
        if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)):
            m.weight.data = m.weight.data.half()
            if m.bias is not None:
                m.bias.data = m.bias.data.half()
        if isinstance(m, nn.MultiheadAttention):
            for name in ("in_proj_weight", "q_proj_weight", "k_proj_weight", "v_proj_weight",
                         "in_proj_bias", "bias_k", "bias_v"):
                t = getattr(m, name)
                if t is not None:
                    t.data = t.data.half()
        for name in ("text_projection", "proj"):
            t = getattr(m, name, None)
            if isinstance(t, nn.Parameter):
                t.data = t.data.half()
    return model


def clip_slice(visual_depth=2, text_depth=2, fp16=True):
    """ViT-B/16 at its true widths (768 / 12 heads / 197 tokens; 512 / 8 heads / 77 tokens; embed
    512) with a chosen depth per tower."""
    model = CLIP(embed_dim=512, image_resolution=224, vision_layers=visual_depth, vision_width=768,
                 vision_patch_size=16, context_length=77, vocab_size=49408, transformer_width=512,
                 transformer_heads=8, transformer_layers=text_depth)
    return half_weights(model) if fp16 else model


def clip_vit_b16(fp16=True):
    """OpenAI CLIP ViT-B/16: 12 + 12 blocks, 96 prunable matrices, 122 683 392 elements in them."""
    return clip_slice(12, 12, fp16=fp16)


def clip_toy(visual_depth=2, text_depth=2, fp16=False):
    """Toy towers (32 x 32 images in 16-pixel patches: 5 tokens of width 64, one head, the
    reference's `width // 64`; 6 text tokens of width 32, 2 heads; embed 16; vocabulary 64)."""
    model = CLIP(embed_dim=16, image_resolution=32, vision_layers=visual_depth, vision_width=64,
                 vision_patch_size=16, context_length=6, vocab_size=64, transformer_width=32,
                 transformer_heads=2, transformer_layers=text_depth)
    return half_weights(model) if fp16 else model


def prunable_names(model):
    """The reference's prunable set (CoOp/trainers/pruners/wanda_pruner.py:544-551): 2-D parameters
    whose name contains `.resblocks`, in `named_parameters()` order."""
    return [n for n, p in model.named_parameters() if p.dim() == 2 and ".resblocks" in n]
