"""GPU: `ecoflap_causal_lm_loss` (csrc/lm_loss.hip) against a float64 log_softmax of the very same
16-bit logits, and its exactness properties: ignored rows, the shifted last token, out-of-range
targets, padding never read, repeatability, batch invariance, graph capture.

Accuracy bound per row: |err| <= 2 * E_torch + 4 * 2^-24 * (|max| + ln(vocab)), where E_torch is the
largest error of torch's own fp32 `F.cross_entropy(logits.float(), reduction="none")` on the GPU
against the same fp64 values in that case (the factor 2: a different exponential and summation order
in the same precision; the second term: the three final roundings every fp32 evaluation has).  The
mean is held against the fp64 mean of the kernel's own row_loss within rows * 2^-24 relative (the
sequential-sum bound).

Measured on an MI355X (profiles/r14_llama_pruner/pytest_new_gpu_tests.txt): largest |err| / bound
0.30 over all cases ((2, 5, 8, 8) f16), largest |err| 1.4e-06 on 4 x normal logits where torch's own
fp32 rows have 1.1e-06; the +-65504 row 1.4e-03 (torch's own: the same) under a bound of 2.7e-03."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGNORE = -100
CANARY = 16
# (batch, tokens, vocab, row stride)
CASES = [(1, 1, 1, 8), (1, 2, 7, 8), (2, 5, 8, 8), (2, 70, 96, 96), (1, 3, 1000, 1008),
         (1, 3, 32000, 32000), (1, 2, 128256, 128256), (3, 4, 2048, 4096)]
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _buffer(batch, tokens, vocab, stride, dtype, seed):
    """[batch, tokens, stride] with 4 x standard normal in the first `vocab` columns and NaN / +inf
    poison behind them -> (buffer, its [batch, tokens, vocab] view)."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.empty(batch, tokens, stride, dtype=dtype)
    buf[..., :vocab] = (4 * torch.randn(batch, tokens, vocab, generator=g)).to(dtype)
    if stride > vocab:
        buf[..., vocab:] = float("nan")
        buf[..., vocab::2] = float("inf")
    buf = buf.to(_dev())
    return buf, buf[..., :vocab]


def _labels(batch, tokens, vocab, seed):
    """Random targets, with column 0, column vocab - 1 and (vocab % 8 != 0) the ragged tail among them."""
    g = torch.Generator().manual_seed(seed + 1)
    lab = torch.randint(0, vocab, (batch, tokens), generator=g)
    flat = lab.view(-1)
    special = [0, vocab - 1] + ([vocab - (vocab % 8)] if vocab % 8 else [])
    for i, col in enumerate(special):
        flat[(i + 1) % flat.numel()] = col       # (position 1 first: the target of row 0 under shift)
    return lab.to(_dev())


def _targets(labels, shift):
    """Per row the target the kernel is to use ([batch, tokens], IGNORE where there is none)."""
    if not shift:
        return labels
    return F.pad(labels, (0, 1), value=IGNORE)[..., 1:].contiguous()


def _call(view, labels, shift, ignore=IGNORE):
    """The C entry point on a [batch, tokens, vocab] view -> (row_loss [batch, tokens], mean, canary)."""
    from ecoflap_amd import hip
    from ecoflap_amd.shapes import fused
    batch, tokens, vocab = view.shape
    assert view.stride(2) == 1 or vocab == 1
    assert batch == 1 or view.stride(0) == tokens * view.stride(1)
    rows = batch * tokens
    out = torch.full((rows + CANARY,), -7.25, dtype=torch.float32, device=view.device)
    loss = torch.full((1,), -7.25, dtype=torch.float32, device=view.device)
    rc = fused._get().ecoflap_causal_lm_loss(view.data_ptr(), labels.data_ptr(), out.data_ptr(), loss.data_ptr(),
                                             batch, tokens, vocab, view.stride(1), ignore, int(shift),
                                             hip.DTYPE_CODE[view.dtype], fused._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out[:rows].view(batch, tokens), loss[0], out[rows:]


def _fp64_rows(view, targets):
    x = view.double()
    lsm = torch.log_softmax(x, dim=-1)
    has = targets != IGNORE
    picked = lsm.gather(-1, targets.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    return torch.where(has, -picked, torch.zeros_like(picked)), has


def _torch_rows(view, targets):
    v = view.shape[-1]
    return F.cross_entropy(view.float().reshape(-1, v), targets.reshape(-1), ignore_index=IGNORE,
                           reduction="none").view(targets.shape)


def _check(view, labels, shift, what):
    targets = _targets(labels, shift)
    ref, has = _fp64_rows(view, targets)
    e_torch = float((_torch_rows(view, targets).double() - ref).abs().max())
    rows, mean, canary = _call(view, labels, shift)
    vocab = view.shape[-1]
    bound = 2 * e_torch + 4 * 2.0 ** -24 * (view.double().amax(-1).abs() + math.log(vocab))
    err = (rows.double() - ref).abs()
    print(f"{what}: max |err| {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}, "
          f"E_torch {e_torch:.3e}, worst err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.min()))
    assert bool((rows[~has] == 0).all())
    assert bool((canary == -7.25).all())
    n = int(has.sum())
    own = float(rows.double()[has].sum() / n) if n else float("nan")
    if n:
        assert abs(float(mean) - own) <= rows.numel() * 2.0 ** -24 * abs(own) + 1e-45, (what, float(mean), own)
    else:
        assert math.isnan(float(mean))
    return rows, mean


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_against_fp64(case, dtype, shift):
    batch, tokens, vocab, stride = case
    buf, view = _buffer(batch, tokens, vocab, stride, DTYPES[dtype], seed=vocab)
    before = buf.clone()
    labels = _labels(batch, tokens, vocab, seed=vocab)
    _check(view, labels, shift, f"{case} {dtype} shift={shift}")
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16))       # logits and padding untouched


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("vocab,stride", [(1000, 1008), (32000, 32000)])
def test_special_rows(vocab, stride, dtype):
    """A row of equal values (nll = ln vocab), the largest finite magnitudes (fp16) and -inf
    everywhere but three columns."""
    dt = DTYPES[dtype]
    buf, view = _buffer(1, 3, vocab, stride, dt, seed=5)
    big = 65504.0 if dt == torch.float16 else 3.0e38
    view[0, 0, :] = 1.5
    view[0, 1, :] = -big
    view[0, 1, ::3] = big
    view[0, 2, :] = float("-inf")
    cols = [0, vocab // 2 + 1, vocab - 1]
    view[0, 2, cols] = torch.tensor([0.5, -2.0, 3.0], dtype=dt, device=view.device)
    labels = torch.tensor([[7, 1, vocab - 1]], device=view.device)           # row 1: a -big target
    if dt == torch.bfloat16:
        labels[0, 1] = 0        # 2 x 3e38 overflows fp32; the fp16 case is the one that is asked for
    rows, _ = _check(view, labels, 0, f"special {vocab} {dtype}")
    assert abs(float(rows[0, 0]) - math.log(vocab)) <= 4 * 2.0 ** -24 * (1.5 + math.log(vocab))


def test_ignored_rows_and_the_shifted_last_token():
    buf, view = _buffer(3, 4, 2048, 4096, torch.float16, seed=1)
    labels = _labels(3, 4, 2048, seed=1)
    labels[1, 2] = IGNORE
    for shift in (0, 1):
        rows, mean = _check(view, labels, shift, f"ignored shift={shift}")
        targets = _targets(labels, shift)
        assert bool((rows[targets == IGNORE] == 0).all()) and bool((rows[targets != IGNORE] > 0).all())
        if shift:
            assert bool((rows[:, -1] == 0).all()) and float(rows[1, 1]) == 0.0
        else:
            assert float(rows[1, 2]) == 0.0
        counted = int((targets != IGNORE).sum())
        assert abs(float(mean) - float(rows.double().sum() / counted)) <= 12 * 2.0 ** -24 * float(mean)
    labels[:] = IGNORE
    rows, mean, _ = _call(view, labels, 0)
    assert bool((rows == 0).all()) and math.isnan(float(mean))
    one = torch.full((3, 1), 5, dtype=torch.int64, device=view.device)         # one token, shifted: no target at all
    _, short = _buffer(3, 1, 2048, 4096, torch.float16, seed=8)
    rows, mean, _ = _call(short, one, 1)
    assert bool((rows == 0).all()) and math.isnan(float(mean))
    # another ignore_index
    labels = _labels(3, 4, 2048, seed=2)
    labels[0, 0] = 17
    rows, _, _ = _call(view, labels, 0, ignore=17)
    assert float(rows[0, 0]) == 0.0 and bool((rows.view(-1)[1:] > 0).all())


@pytest.mark.parametrize("case", [(1, 3, 1000, 1008), (3, 4, 2048, 4096)], ids=lambda c: "x".join(map(str, c)))
def test_out_of_range_targets_are_loud_and_read_nothing(case):
    """A target equal to vocab, and one of -5: NaN for that row and for the mean, the other rows
    as without them.  Padded strides: even a wrong index would stay inside the allocation."""
    batch, tokens, vocab, stride = case
    buf, view = _buffer(batch, tokens, vocab, stride, torch.float16, seed=3)
    before = buf.clone()
    labels = _labels(batch, tokens, vocab, seed=3)
    good, good_mean, _ = _call(view, labels, 0)
    assert bool(torch.isfinite(good).all()) and math.isfinite(float(good_mean))
    for bad in (vocab, -5):
        lab = labels.clone()
        lab.view(-1)[1] = bad
        rows, mean, canary = _call(view, lab, 0)
        assert math.isnan(float(rows.view(-1)[1])) and math.isnan(float(mean))
        keep = torch.ones(batch * tokens, dtype=torch.bool, device=rows.device)
        keep[1] = False
        assert torch.equal(rows.view(-1)[keep], good.view(-1)[keep])
        assert bool((canary == -7.25).all())
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16))


def test_repeatable_and_batch_invariant():
    buf, view = _buffer(3, 4, 2048, 4096, torch.float16, seed=4)
    labels = _labels(3, 4, 2048, seed=4)
    for shift in (0, 1):
        a, ma, _ = _call(view, labels, shift)
        b, mb, _ = _call(view, labels, shift)
        assert torch.equal(a, b) and torch.equal(ma, mb)
        for s in range(3):
            alone, _, _ = _call(view[s:s + 1], labels[s:s + 1].contiguous(), shift)
            assert torch.equal(alone[0], a[s]), (shift, s)


def test_mean_survives_graph_capture():
    from ecoflap_amd.shapes import fused
    buf, view = _buffer(2, 70, 96, 96, torch.float16, seed=6)
    labels = _labels(2, 70, 96, seed=6)
    with torch.no_grad():
        eager, eager_rows = fused.causal_lm_loss(view, labels, return_row_loss=True)
        _, direct, _ = _call(view, labels, 1)
        assert torch.equal(eager, direct)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            fused.causal_lm_loss(view, labels)              # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured, captured_rows = fused.causal_lm_loss(view, labels, return_row_loss=True)
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager) and torch.equal(captured_rows, eager_rows)
