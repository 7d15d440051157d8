"""CPU: `LlamaForCausalLM.stage_plan()` — the stages compose to `forward` bit for bit, every
parameter has exactly one owning stage, and the closure / batch helpers of the LLaMA path."""
import torch

from llama_pruner_fixture import seeded_tiny


def _model():
    return seeded_tiny().eval()


def test_stage_composition_is_forward_bit_for_bit():
    from ecoflap_amd.shapes.llama import llama_batches
    model = _model()
    ids = llama_batches(1, 2, 70, model.config.vocab_size, seed=3)[0]["input_ids"]
    with torch.no_grad():
        want = model(ids, labels=ids)
        plan = model.stage_plan()
        state = {"input_ids": ids}
        for _, _, fn in plan:
            state = fn(state)
    assert [name for name, _, _ in plan] == (["model.embed"]
                                             + [f"model.layers.{i}" for i in range(len(model.model.layers))]
                                             + ["head"])
    assert set(state) == {"loss", "logits"}
    assert torch.equal(state["logits"], want.logits) and torch.equal(state["loss"], want.loss)
    assert state["loss"].dim() == 0 and state["loss"].dtype == torch.float32
    # no labels: logits alone
    with torch.no_grad():
        assert model(ids).loss is None and torch.equal(model(ids).logits, want.logits)


def test_head_is_the_last_stage_alone():
    model = _model()
    ids = torch.randint(0, model.config.vocab_size, (2, 9), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = model(ids, labels=ids)
        logits, loss = model.head(model.model(ids), ids)
    assert torch.equal(logits, want.logits) and torch.equal(loss, want.loss)


def test_every_parameter_has_exactly_one_owner():
    model = _model()
    plan = model.stage_plan()
    for name, _ in model.named_parameters():
        owners = [stage for stage, prefixes, _ in plan if any(name.startswith(p) for p in prefixes)]
        assert len(owners) == 1, (name, owners)
    owned = {"model.embed": "model.embed_tokens.weight", "head": "lm_head.weight"}
    for stage, prefixes, _ in plan:
        if stage in owned:
            assert any(owned[stage].startswith(p) for p in prefixes)
    assert any("model.norm.weight".startswith(p) for p in plan[-1][1])


def test_closure_and_batch_helpers():
    from ecoflap_amd.pruners.layer_sparsity import _default_batch_len
    from ecoflap_amd.pruners.losses import loss_causal_lm
    from ecoflap_amd.pruners.prefix_cache import PrefixCachedLoss
    from ecoflap_amd.shapes.llama import llama_batches
    model = _model()
    a = llama_batches(3, 2, 16, 96, seed=5)
    b = llama_batches(3, 2, 16, 96, seed=5)
    assert len(a) == 3 and all(set(x) == {"input_ids"} for x in a)
    assert all(torch.equal(x["input_ids"], y["input_ids"]) for x, y in zip(a, b))
    assert a[0]["input_ids"].shape == (2, 16) and a[0]["input_ids"].dtype == torch.int64
    assert int(a[0]["input_ids"].max()) < 96 and not torch.equal(a[0]["input_ids"], a[1]["input_ids"])
    assert _default_batch_len(a[0]) == 2
    with torch.no_grad():
        loss, n = loss_causal_lm(model, a[0], False)
        assert n == 2 and torch.equal(loss, model(a[0]["input_ids"], labels=a[0]["input_ids"]).loss)
        staged = PrefixCachedLoss(model)
        got, n2 = staged(model, a[0], False)
    assert n2 == 2 and torch.equal(got, loss)
