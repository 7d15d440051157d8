"""CPU: `ecoflap_causal_attention` and `ecoflap_silu_mul` reject bad arguments with the documented
codes before anything is launched (fake pointers, no GPU), and both are declared where the
plumbing ops live (include/ecoflap_shape_ops.h), not in the pruner ABI."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDTYPE, ENULL, ESIZE, EALIGN = -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 2


def _lib():
    from ecoflap_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    vp, i64, f32, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    lib.ecoflap_causal_attention.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, i64,
                                             f32, ci, vp]
    lib.ecoflap_silu_mul.argtypes = [vp, vp, vp, i64, ci, vp]
    return lib


def test_dtype_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "ecoflap_hip.h")).read()
    for name, value in (("ECOFLAP_F32", F32), ("ECOFLAP_F16", F16), ("ECOFLAP_BF16", BF16),
                        ("ECOFLAP_EDTYPE", EDTYPE), ("ECOFLAP_ENULL", ENULL), ("ECOFLAP_ESIZE", ESIZE),
                        ("ECOFLAP_EALIGN", EALIGN)):
        assert re.search(rf"\b{name}\b\s*=?\s*\(?{value}\b", text), name


def test_causal_attention_argument_errors():
    lib = _lib()
    H, row = 2, 2 * 128

    def call(q=4096, k=8192, v=12288, o=16384, cos=20480, sin=24576, batch=2, tokens=70, heads=H, hd=128,
             qts=row, qbs=70 * row, ots=row, obs=70 * row, scale=128 ** -0.5, dtype=F16):
        return lib.ecoflap_causal_attention(q, k, v, o, cos, sin, batch, tokens, heads, hd, qts, qbs, ots, obs,
                                            scale, dtype, None)

    assert call(dtype=BF16) == EDTYPE and call(dtype=F32) == EDTYPE and call(dtype=7) == EDTYPE
    # sizes
    assert call(hd=64) == ESIZE and call(hd=96) == ESIZE and call(hd=256) == ESIZE
    assert call(tokens=0) == ESIZE and call(tokens=-5) == ESIZE and call(tokens=4097) == ESIZE
    assert call(batch=0) == ESIZE and call(batch=-1) == ESIZE and call(heads=0) == ESIZE and call(heads=-2) == ESIZE
    assert call(batch=1 << 20, heads=1 << 6, tokens=1024) == ESIZE           # 2^26 items x 32 query tiles = 2^31
    assert call(batch=1 << 40) == ESIZE and call(heads=1 << 40) == ESIZE
    assert call(scale=0.0) == ESIZE and call(scale=-1.0) == ESIZE
    assert call(scale=float("inf")) == ESIZE and call(scale=float("nan")) == ESIZE
    assert call(qts=row - 8) == ESIZE and call(ots=row - 8) == ESIZE        # a token stride shorter than a row
    assert call(qbs=-8) == ESIZE and call(obs=-8) == ESIZE
    # pointers
    for name in ("q", "k", "v", "o"):
        assert call(**{name: None}) == ENULL, name
    assert call(cos=None) == ENULL and call(sin=None) == ENULL              # one table pointer alone
    # alignment
    for name in ("q", "k", "v", "o", "cos", "sin"):
        assert call(**{name: 4096 + 8}) == EALIGN, name
    assert call(qts=row + 4) == EALIGN and call(qbs=70 * row + 2) == EALIGN
    assert call(ots=row + 4) == EALIGN and call(obs=70 * row + 6) == EALIGN
    # the order of mha_attention: dtype, sizes, nulls, alignment
    assert call(dtype=BF16, hd=64, q=None) == EDTYPE
    assert call(hd=64, q=None) == ESIZE
    assert call(q=None, k=4096 + 2) == ENULL


def test_silu_mul_argument_errors():
    lib = _lib()

    def call(a=4096, b=8192, y=12288, n=64, dtype=F16):
        return lib.ecoflap_silu_mul(a, b, y, n, dtype, None)

    assert call(dtype=F32) == EDTYPE and call(dtype=9) == EDTYPE
    assert call(n=0) == ESIZE and call(n=-8) == ESIZE and call(n=12) == ESIZE and call(n=4103) == ESIZE
    assert call(n=12, dtype=BF16) == ESIZE
    assert call(a=None) == ENULL and call(b=None) == ENULL and call(y=None) == ENULL
    assert call(a=4096 + 2) == EALIGN and call(b=8192 + 8) == EALIGN and call(y=12288 + 4) == EALIGN
    assert call(dtype=F32, n=12, a=None) == EDTYPE and call(n=12, a=None) == ESIZE


def test_the_new_names_are_plumbing_not_pruner_abi():
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)  # noqa: E731
    shape_ops = re.findall(r"\b(ecoflap_[a-z0-9_]+)\s*\(", strip("ecoflap_shape_ops.h"))
    abi = re.findall(r"\b(ecoflap_[a-z0-9_]+)\s*\(", strip("ecoflap_hip.h"))
    for name in ("ecoflap_causal_attention", "ecoflap_silu_mul"):
        assert name in shape_ops and name not in abi
        assert hasattr(_lib(), name)
