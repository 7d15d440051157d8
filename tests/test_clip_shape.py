"""CPU: `ecoflap_amd/shapes/clip.py`, the OpenAI-CLIP ViT two-tower shape — parameter names in the
reference's `named_parameters()` order (CoOp/clip/model.py:167-368), shapes, dtypes after
`half_weights`, the block contract a pruner touches, and the contrastive closure on it."""
import torch

from ecoflap_amd.shapes import clip as C

BLOCK = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
         "ln_1.weight", "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
         "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias"]


def expected_names(visual_depth, text_depth):
    """A module's own parameters first, then its children in the order they were assigned."""
    names = ["positional_embedding", "text_projection", "logit_scale",
             "visual.class_embedding", "visual.positional_embedding", "visual.proj",
             "visual.conv1.weight", "visual.ln_pre.weight", "visual.ln_pre.bias"]
    names += [f"visual.transformer.resblocks.{i}.{p}" for i in range(visual_depth) for p in BLOCK]
    names += ["visual.ln_post.weight", "visual.ln_post.bias"]
    names += [f"transformer.resblocks.{i}.{p}" for i in range(text_depth) for p in BLOCK]
    return names + ["token_embedding.weight", "ln_final.weight", "ln_final.bias"]


def test_parameter_names_are_in_the_reference_order():
    assert [n for n, _ in C.clip_toy(3, 2).named_parameters()] == expected_names(3, 2)
    with torch.device("meta"):
        big = C.clip_vit_b16()
    assert [n for n, _ in big.named_parameters()] == expected_names(12, 12)


def test_vit_b16_has_96_prunable_matrices_of_122683392_elements():
    with torch.device("meta"):
        big = C.clip_vit_b16()
    params = dict(big.named_parameters())
    names = C.prunable_names(big)
    assert len(names) == 96 and sum(params[n].numel() for n in names) == 122683392
    assert all(n.startswith(("visual.transformer.resblocks.", "transformer.resblocks.")) for n in names)
    assert tuple(params["visual.transformer.resblocks.0.attn.in_proj_weight"].shape) == (2304, 768)
    assert tuple(params["transformer.resblocks.11.mlp.c_proj.weight"].shape) == (512, 2048)
    assert tuple(params["visual.positional_embedding"].shape) == (197, 768)
    assert tuple(params["positional_embedding"].shape) == (77, 512)
    assert tuple(params["token_embedding.weight"].shape) == (49408, 512)
    assert big.visual.transformer.resblocks[0].attn.num_heads == 12
    assert big.transformer.resblocks[0].attn.num_heads == 8


def test_half_weights_converts_what_convert_weights_converts():
    with torch.device("meta"):
        big = C.clip_vit_b16()
    for n, p in big.named_parameters():
        fp32 = (".ln_" in n or n.startswith(("ln_final", "visual.ln_", "token_embedding", "logit_scale"))
                or n in ("positional_embedding", "visual.class_embedding", "visual.positional_embedding"))
        assert p.dtype == (torch.float32 if fp32 else torch.float16), n
    assert big.dtype == torch.float16


def test_block_contract():
    model = C.clip_toy().eval()
    vis, txt = model.visual.transformer.resblocks, model.transformer.resblocks
    assert isinstance(vis, torch.nn.Sequential) and isinstance(txt, torch.nn.Sequential)
    assert vis[0].attn_mask is None
    mask = txt[0].attn_mask
    assert tuple(mask.shape) == (6, 6) and torch.equal(mask, torch.full((6, 6), float("-inf")).triu_(1))
    assert all(blk.attn_mask is mask for blk in txt)
    x = torch.randn(6, 3, 32)                                   # [L, N, D]
    with torch.no_grad():
        y = txt[0](x)
        assert y.shape == x.shape
        a = txt[0].attention(txt[0].ln_1(x))
        want = txt[0].attn(txt[0].ln_1(x), txt[0].ln_1(x), txt[0].ln_1(x), need_weights=False, attn_mask=mask)[0]
        assert torch.equal(a, want)
        # causal: a token's output does not depend on later tokens
        x2 = x.clone()
        x2[4:] += 1.0
        assert torch.equal(txt[0](x2)[:4], y[:4])
        assert vis[0](torch.randn(5, 3, 64)).shape == (5, 3, 64)
    assert type(txt[0].attn.out_proj) is not torch.nn.Linear    # (the subclass `find_layers` does not hook)
    assert txt[0].attn.embed_dim == 32 and txt[0].attn.num_heads == 2


def test_forward_and_the_contrastive_closure():
    from ecoflap_amd.pruners.losses import clip_contrastive
    torch.manual_seed(0)
    model = C.clip_toy().eval()
    img = torch.randn(4, 3, 32, 32)
    prompts = torch.randint(1, 60, (10, 6))
    prompts[torch.arange(10), torch.randint(1, 6, (10,))] = 63      # end of text = the row's maximum
    labels = torch.tensor([7, 2, 9, 0])
    with torch.no_grad():
        per_image, per_text = model(img, prompts[labels])
        assert per_image.shape == (4, 4) and torch.isfinite(per_image).all()
        assert torch.allclose(per_image, per_text.t(), rtol=1e-5, atol=1e-5)
        assert per_image.abs().max() <= 1 / 0.07 * (1 + 1e-5)         # cosine similarities x exp(logit_scale)
        # the text feature is read at the end-of-text position
        feats = model.encode_text(prompts[labels])
        moved = prompts[labels].clone()
        for r in range(4):                                           # ids after the end of text do not matter (causal)
            e = int(moved[r].argmax())
            moved[r, e + 1:] = 1
        assert torch.equal(model.encode_text(moved), feats)
        loss, n = clip_contrastive(prompts)(model, {"img": img, "label": labels}, torch.device("cpu"))
    assert n == 4 and loss.dim() == 0 and loss.dtype == torch.float32 and torch.isfinite(loss)
    # fp16 weights run on the CPU too (the reference's own mode)
    half = C.clip_toy(fp16=True).eval()
    with torch.no_grad():
        assert half(img, prompts[labels])[0].dtype == torch.float16
