"""CPU: `ecoflap_causal_lm_loss` is exported as plumbing (include/ecoflap_shape_ops.h, not the pruner
ABI), rejects bad arguments with the documented codes before anything is launched (fake pointers, no
GPU), and `fused.causal_lm_loss` refuses what the kernel does not serve."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDTYPE, ENULL, ESIZE, EMODE, EALIGN = -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2


def _lib():
    from ecoflap_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.ecoflap_causal_lm_loss.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, i64, ci, ci, vp]
    return lib


def test_the_name_is_plumbing_not_pruner_abi():
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)  # noqa: E731
    shape_ops = re.findall(r"\b(ecoflap_[a-z0-9_]+)\s*\(", strip("ecoflap_shape_ops.h"))
    abi = re.findall(r"\b(ecoflap_[a-z0-9_]+)\s*\(", strip("ecoflap_hip.h"))
    from ecoflap_amd import hip
    assert "ecoflap_causal_lm_loss" in shape_ops and "ecoflap_causal_lm_loss" not in abi
    assert "ecoflap_causal_lm_loss" not in hip.EXPORTS
    assert hasattr(_lib(), "ecoflap_causal_lm_loss")


def test_argument_errors():
    lib = _lib()

    def call(logits=4096, labels=8192, row_loss=12288, loss=16384, batch=2, tokens=5, vocab=96, stride=96,
             ignore=-100, shift=1, dtype=F16):
        return lib.ecoflap_causal_lm_loss(logits, labels, row_loss, loss, batch, tokens, vocab, stride, ignore,
                                          shift, dtype, None)

    for name in ("logits", "labels", "row_loss", "loss"):
        assert call(**{name: None}) == ENULL, name
    assert call(dtype=F32) == EDTYPE and call(dtype=7) == EDTYPE and call(dtype=-1) == EDTYPE
    assert call(batch=-1) == ESIZE and call(tokens=-2) == ESIZE and call(vocab=-8) == ESIZE
    assert call(vocab=0, stride=0) == ESIZE and call(vocab=0, stride=8) == ESIZE     # rows > 0
    assert call(stride=88) == ESIZE and call(vocab=97, stride=96) == ESIZE
    assert call(batch=1 << 16, tokens=1 << 15) == ESIZE                              # 2^31 rows
    assert call(batch=1 << 40) == ESIZE and call(tokens=1 << 40) == ESIZE and call(batch=1 << 62, tokens=4) == ESIZE
    assert call(shift=2) == EMODE and call(shift=-1) == EMODE
    assert call(logits=4096 + 8) == EALIGN and call(logits=4096 + 2) == EALIGN
    assert call(stride=100) == EALIGN and call(vocab=90, stride=92) == EALIGN
    assert call(labels=8192 + 4) == EALIGN and call(row_loss=12288 + 2) == EALIGN and call(loss=16384 + 1) == EALIGN
    # the order: nulls, dtype, sizes, shift, alignment
    assert call(logits=None, dtype=F32, vocab=-1, shift=3) == ENULL
    assert call(dtype=F32, vocab=-1, shift=3, stride=100) == EDTYPE
    assert call(vocab=-1, shift=3, stride=100) == ESIZE
    assert call(shift=3, stride=100) == EMODE
    assert call(dtype=BF16, stride=100) == EALIGN


def test_fused_wrapper_refuses(monkeypatch):
    from ecoflap_amd.shapes import fused
    labels = torch.zeros(2, 5, dtype=torch.int64)
    with torch.no_grad():
        assert fused.causal_lm_loss(torch.zeros(2, 5, 96, dtype=torch.float16), labels) is None          # CPU
        assert fused.causal_lm_loss(torch.zeros(2, 5, 96, dtype=torch.float32), labels) is None          # fp32
    with torch.enable_grad():
        assert fused.causal_lm_loss(torch.zeros(2, 5, 96, dtype=torch.float16), labels) is None
    if torch.cuda.is_available():
        dev = torch.device("cuda")
        x, lab = torch.zeros(2, 5, 96, dtype=torch.float16, device=dev), labels.to(dev)
        with torch.no_grad():
            assert fused.causal_lm_loss(x.float(), lab) is None
            assert fused.causal_lm_loss(x, lab) is not None
            monkeypatch.setenv("ECOFLAP_NO_FUSED_LOSS", "1")
            assert fused.causal_lm_loss(x, lab) is None
        with torch.enable_grad():
            assert fused.causal_lm_loss(x, lab) is None
    else:
        # the switch is consulted before any device work: a tensor that only claims to be served
        monkeypatch.setenv("ECOFLAP_NO_FUSED_LOSS", "1")
        monkeypatch.setattr(fused, "_usable", lambda *t: True)
        with torch.no_grad():
            assert fused.causal_lm_loss(torch.zeros(2, 5, 96, dtype=torch.float16), labels) is None
