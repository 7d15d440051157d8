"""LLaMA decoder shape (plumbing): random-init, with the parameter names, shapes and
`named_parameters()` order of transformers' `LlamaForCausalLM` (`tie_word_embeddings=False`, no
biases; `num_key_value_heads` below `num_attention_heads` gives grouped-query attention: narrower
`k_proj` / `v_proj`, query head h reading KV head h // (heads // kv_heads)) — the model the reference's `LLaMA/main.py` loads through
`AutoModelForCausalLM` in fp16 with `seqlen = 2048`:

    model.embed_tokens
    model.layers.N.self_attn.{q,k,v,o}_proj     (three separate q / k / v Linears: a pruner treats them apart)
    model.layers.N.mlp.{gate,up,down}_proj
    model.layers.N.input_layernorm, model.layers.N.post_attention_layernorm
    model.norm, lm_head

`model.model.layers` is an `nn.ModuleList` of blocks taking and returning `[B, T, D]`;
`model.seqlen` and `model.config.use_cache` exist because Wanda-style code touches them;
`model(input_ids, labels=None)` returns an object with `.logits` and `.loss` (transformers'
`ForCausalLMLoss`: labels padded by one -100 and shifted, flat fp32 cross entropy, mean).

On the CPU, with autograd, or in a dtype other than fp16 a block runs transformers' eager op chain
(tests/test_llama_shape_golden.py pins it to transformers' own logits bit for bit): RMSNorm with
fp32 statistics and `weight * x.to(dtype)`, `q * cos + rotate_half(q) * sin`, `matmul * scale +
mask`, `softmax(dtype=float32).to(dtype)`, `matmul`; with grouped-query attention k is rotated at
`kv_heads` heads and k / v then go through transformers' `repeat_kv` (`expand` + `reshape`;
tests/test_llama_gqa_shape_golden.py).  On the GPU under `no_grad` in fp16 a block
runs `fused.t5_rmsnorm` (LLaMA's RMSNorm is T5's formula), the projections through `fused.linear`,
`fused.causal_attention` with the rotary table (csrc/causal_attention.hip: rotation, mask, online
softmax and both products in one kernel, the projections' outputs read in place; with `kv_heads`
below `heads` its grouped-query entry, which reads the narrow k / v in place: no `repeat_kv` copy), `o_proj`,
`fused.t5_add_rmsnorm` for residual + post-attention norm, `fused.silu_mul`, `down_proj` and the
last residual.  Every `None` from a fused op falls back to the torch op at that site alone; the
kernel serves head width 128 and up to 4096 tokens.  There, too, the loss comes from
`fused.causal_lm_loss` (csrc/lm_loss.hip: the shift is an index inside the kernel and the fp16 logits
are read once; `ECOFLAP_NO_FUSED_LOSS` in the environment keeps torch's chain).

`stage_plan()` cuts the forward into `model.embed`, one stage per decoder block and `head` (final
norm, lm_head, loss) for `PrefixCachedLoss`; `forward` is their composition.  Calibration batches
are `{"input_ids": LongTensor [B, T]}` and the labels are the ids themselves (`llama_batches`,
`pruners/losses.py::loss_causal_lm`).

`llama_7b`, `llama3_8b`, `llama2_70b` and `mistral_7b` build the true shapes (under
`torch.device("meta")` without the memory); `llama_tiny` a toy.

Not here: Mistral's sliding window, bf16 attention, a KV cache, a tokenizer, datasets, perplexity
evaluation."""
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused


def rotary_table(tokens, head_dim, theta, device):
    """transformers' default rotary recipe for positions 0 .. tokens - 1: fp32 `inv_freq`, fp32
    `positions x inv_freq`, fp32 cos / sin -> (cos, sin), each [tokens, head_dim // 2] (the table
    transformers uses is `cat(freqs, freqs)`: both halves are this one)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float) / head_dim))
    pos = torch.arange(tokens, dtype=torch.float)
    freqs = pos[:, None] * inv_freq[None, :]
    return freqs.cos().to(device).contiguous(), freqs.sin().to(device).contiguous()


def rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def _linear(lin, x):
    """`lin(x)`; a plain, unhooked Linear goes through `fused.linear` where that serves it."""
    if lin._forward_hooks or lin._forward_pre_hooks or "forward" in lin.__dict__:
        return lin(x)
    y = fused.linear(x, lin.weight, lin.bias)
    return y if y is not None else lin(x)


class LlamaRMSNorm(nn.Module):
    def __init__(self, d, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.variance_epsilon = eps

    def torch_forward(self, x):
        dtype = x.dtype
        x = x.to(torch.float32)
        var = x.pow(2).mean(-1, keepdim=True)
        x = x * torch.rsqrt(var + self.variance_epsilon)
        return self.weight * x.to(dtype)

    def forward(self, x):
        y = fused.t5_rmsnorm(x, self.weight, self.variance_epsilon)
        return y if y is not None else self.torch_forward(x)


class LlamaAttention(nn.Module):
    def __init__(self, cfg, rope):
        super().__init__()
        self.num_heads, self.head_dim = cfg.num_attention_heads, cfg.head_dim
        self.scaling = self.head_dim ** -0.5
        self.num_kv_heads = cfg.num_key_value_heads
        if self.num_kv_heads < 1 or self.num_heads % self.num_kv_heads != 0:
            raise ValueError(f"{self.num_heads} heads cannot share {self.num_kv_heads} key / value heads")
        inner, kv_inner = self.num_heads * self.head_dim, self.num_kv_heads * self.head_dim
        self.q_proj = nn.Linear(cfg.hidden_size, inner, bias=False)
        self.k_proj = nn.Linear(cfg.hidden_size, kv_inner, bias=False)
        self.v_proj = nn.Linear(cfg.hidden_size, kv_inner, bias=False)
        self.o_proj = nn.Linear(inner, cfg.hidden_size, bias=False)
        self.__dict__["_rope"] = rope           # the model's table cache (not a submodule)

    def torch_attention(self, q, k, v):
        """transformers' eager chain on the projections' outputs (q [B, T, H * hd], k / v
        [B, T, KVH * hd]) -> [B, T, H * hd]."""
        B, T, _ = q.shape
        q = q.view(B, T, self.num_heads, self.head_dim).transpose(1, 2)
        k, v = (t.view(B, T, self.num_kv_heads, self.head_dim).transpose(1, 2) for t in (k, v))
        cos, sin = self._rope(T, q.device)
        cos = torch.cat((cos, cos), dim=-1).to(q.dtype)[None, None]
        sin = torch.cat((sin, sin), dim=-1).to(q.dtype)[None, None]
        q = (q * cos) + (rotate_half(q) * sin)
        k = (k * cos) + (rotate_half(k) * sin)
        groups = self.num_heads // self.num_kv_heads
        if groups > 1:                          # transformers' repeat_kv
            k, v = (t[:, :, None, :, :].expand(B, self.num_kv_heads, groups, T, self.head_dim)
                    .reshape(B, self.num_heads, T, self.head_dim) for t in (k, v))
        w = torch.matmul(q, k.transpose(2, 3)) * self.scaling
        mask = torch.full((T, T), torch.finfo(q.dtype).min, dtype=q.dtype, device=q.device).triu_(1)
        w = w + mask[None, None]
        w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        return torch.matmul(w, v).transpose(1, 2).contiguous().reshape(B, T, -1)

    def forward(self, x):
        q, k, v = _linear(self.q_proj, x), _linear(self.k_proj, x), _linear(self.v_proj, x)
        y = None
        if self.head_dim == 128 and x.dim() == 3:
            y = fused.causal_attention(q, k, v, self.num_heads, self.scaling,
                                       rope=self._rope(x.shape[1], x.device) if x.is_cuda else None,
                                       kv_heads=self.num_kv_heads)
        if y is None:
            y = self.torch_attention(q, k, v)
        return _linear(self.o_proj, y)


class LlamaMLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.gate_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, bias=False)
        self.up_proj = nn.Linear(cfg.hidden_size, cfg.intermediate_size, bias=False)
        self.down_proj = nn.Linear(cfg.intermediate_size, cfg.hidden_size, bias=False)

    def forward(self, x):
        a, b = _linear(self.gate_proj, x), _linear(self.up_proj, x)
        h = fused.silu_mul(a, b)
        if h is None:
            h = F.silu(a) * b
        return _linear(self.down_proj, h)


class LlamaDecoderLayer(nn.Module):
    """[B, T, D] -> [B, T, D]."""

    def __init__(self, cfg, rope):
        super().__init__()
        self.self_attn = LlamaAttention(cfg, rope)
        self.mlp = LlamaMLP(cfg)
        self.input_layernorm = LlamaRMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNorm(cfg.hidden_size, cfg.rms_norm_eps)

    def forward(self, x):
        a = self.self_attn(self.input_layernorm(x))
        norm = self.post_attention_layernorm
        res = fused.t5_add_rmsnorm(x, a, norm.weight, norm.variance_epsilon)    # residual + norm in one pass
        if res is not None:
            x, h = res
        else:
            x = x + a
            h = norm(x)
        return x + self.mlp(h)


class LlamaModel(nn.Module):
    def __init__(self, cfg, rope):
        super().__init__()
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList([LlamaDecoderLayer(cfg, rope) for _ in range(cfg.num_hidden_layers)])
        self.norm = LlamaRMSNorm(cfg.hidden_size, cfg.rms_norm_eps)

    def forward(self, input_ids):
        x = self.embed_tokens(input_ids)
        for layer in self.layers:
            x = layer(x)
        return self.norm(x)


class _RopeCache:
    """(tokens, device) -> (cos, sin), built once each."""

    def __init__(self, head_dim, theta):
        self.head_dim, self.theta, self.tables = head_dim, theta, {}

    def __call__(self, tokens, device):
        key = (int(tokens), str(device))
        if key not in self.tables:
            self.tables[key] = rotary_table(tokens, self.head_dim, self.theta, device)
        return self.tables[key]


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg, seqlen=2048):
        super().__init__()
        self.config = cfg
        self.seqlen = seqlen
        rope = _RopeCache(cfg.head_dim, cfg.rope_theta)
        self.__dict__["_rope"] = rope
        self.model = LlamaModel(cfg, rope)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, std=cfg.initializer_range)

    def head(self, hidden, labels=None):
        """lm_head and the loss on the output of `model.norm` -> (logits, loss or None)."""
        logits = _linear(self.lm_head, hidden)
        loss = None
        if labels is not None:
            if logits.dtype == torch.float16:
                loss = fused.causal_lm_loss(logits, labels)
            if loss is None:
                shifted = F.pad(labels, (0, 1), value=-100)[..., 1:].contiguous()
                loss = F.cross_entropy(logits.float().view(-1, self.config.vocab_size), shifted.view(-1),
                                       ignore_index=-100, reduction="mean")
        return logits, loss

    def _embed_stage(self, batch):
        if torch.is_tensor(batch):
            batch = {"input_ids": batch}
        ids = batch["input_ids"].to(self.lm_head.weight.device)
        labels = batch.get("labels", ids)
        return {"x": self.model.embed_tokens(ids),
                "labels": None if labels is None else labels.to(ids.device)}

    def _head_stage(self, state):
        logits, loss = self.head(self.model.norm(state["x"]), state["labels"])
        return {"loss": loss, "logits": logits}

    def stage_plan(self):
        """[(name, owned parameter prefixes, fn(state) -> state)]; stage 0 takes the batch
        `{"input_ids": [B, T]}` (labels: the ids unless the batch carries "labels"), a block stage
        maps {"x", "labels"} to itself and `head` returns {"loss", "logits"}."""
        def block(layer):
            return lambda state: {"x": layer(state["x"]), "labels": state["labels"]}
        return ([("model.embed", ["model.embed_tokens."], self._embed_stage)]
                + [(f"model.layers.{i}", [f"model.layers.{i}."], block(layer))
                   for i, layer in enumerate(self.model.layers)]
                + [("head", ["model.norm.", "lm_head."], self._head_stage)])

    def forward(self, input_ids, labels=None):
        state = {"input_ids": input_ids, "labels": labels}
        for _, _, fn in self.stage_plan():
            state = fn(state)
        return SimpleNamespace(logits=state["logits"], loss=state["loss"])


def llama_batches(n, batch_size, seqlen, vocab, seed=0, device=None):
    """n seeded calibration batches `{"input_ids": LongTensor [batch_size, seqlen]}`; a causal LM's
    labels are its input ids."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        ids = torch.randint(0, vocab, (batch_size, seqlen), generator=g)
        out.append({"input_ids": ids if device is None else ids.to(device)})
    return out


def llama_config(hidden_size, heads, intermediate_size, layers, vocab_size, head_dim=None,
                 rms_norm_eps=1e-6, rope_theta=10000.0, kv_heads=None):
    return SimpleNamespace(hidden_size=hidden_size, num_attention_heads=heads,
                           num_key_value_heads=heads if kv_heads is None else kv_heads,
                           head_dim=head_dim or hidden_size // heads, intermediate_size=intermediate_size,
                           num_hidden_layers=layers, vocab_size=vocab_size, rms_norm_eps=rms_norm_eps,
                           rope_theta=rope_theta, initializer_range=0.02, use_cache=False,
                           tie_word_embeddings=False)


def _build(cfg, dtype, seqlen):
    model = LlamaForCausalLM(cfg, seqlen=seqlen)
    return model if dtype is None or dtype == torch.float32 else model.to(dtype)


def llama_7b(dtype=torch.float16):
    """LLaMA-7B: 32 layers, 4096 wide, 32 heads of 128, MLP 11008, vocabulary 32000, eps 1e-6,
    theta 10000, fp16 (6 738 415 616 parameters; build it under `torch.device("meta")` to look at
    its shape without the memory)."""
    return _build(llama_config(4096, 32, 11008, 32, 32000), dtype, 2048)


def llama3_8b(dtype=torch.float16):
    """Llama-3-8B: 32 layers, 4096 wide, 32 query heads of 128 on 8 key / value heads, MLP 14336,
    vocabulary 128256, eps 1e-5, theta 500000, fp16."""
    return _build(llama_config(4096, 32, 14336, 32, 128256, rms_norm_eps=1e-5, rope_theta=500000.0, kv_heads=8),
                  dtype, 2048)


def llama2_70b(dtype=torch.float16):
    """Llama-2-70B: 80 layers, 8192 wide, 64 query heads of 128 on 8 key / value heads, MLP 28672,
    vocabulary 32000, eps 1e-5, theta 10000, fp16."""
    return _build(llama_config(8192, 64, 28672, 80, 32000, rms_norm_eps=1e-5, kv_heads=8), dtype, 2048)


def mistral_7b(dtype=torch.float16):
    """Mistral-7B's shape: 32 layers, 4096 wide, 32 query heads of 128 on 8 key / value heads, MLP
    14336, vocabulary 32000, eps 1e-5, theta 10000, fp16.  Its sliding window is not modelled: within
    4096 tokens, the window of v0.1, full causal attention is the same function."""
    return _build(llama_config(4096, 32, 14336, 32, 32000, rms_norm_eps=1e-5, kv_heads=8), dtype, 2048)


def llama_tiny(hidden_size=64, heads=2, head_dim=128, intermediate_size=176, layers=2, vocab_size=96,
               dtype=torch.float32, seqlen=128, kv_heads=None):
    """A toy decoder for tests; head width 128 by default, the width the fused attention serves."""
    return _build(llama_config(hidden_size, heads, intermediate_size, layers, vocab_size, head_dim=head_dim,
                               kv_heads=kv_heads), dtype, seqlen)

