"""CPU: `ecoflap_causal_attention_gqa` rejects bad arguments with the documented codes before
anything is launched (fake pointers, no GPU): everything `ecoflap_causal_attention` rejects, in its
order, and the grouped-query arguments on top; the rule behind `heads_per_workgroup == 0`; and the
entry is declared where the plumbing ops live (include/ecoflap_shape_ops.h), not in the pruner ABI."""
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
    lib.ecoflap_causal_attention_gqa.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, i64,
                                                 i64, i64, i64, f32, ci, ci, vp]
    lib.ecoflap_causal_attention_gqa_default_p.argtypes = [i64]
    return lib


def _caller(lib, H=8, KVH=2):
    row, kvrow = H * 128, KVH * 128

    def call(q=4096, k=8192, v=12288, o=16384, cos=20480, sin=24576, batch=2, tokens=70, heads=H, kv=KVH,
             hd=128, qts=row, qbs=70 * row, kts=kvrow, kbs=70 * kvrow, ots=row, obs=70 * row,
             scale=128 ** -0.5, P=0, dtype=F16):
        return lib.ecoflap_causal_attention_gqa(q, k, v, o, cos, sin, batch, tokens, heads, kv, hd, qts, qbs,
                                                kts, kbs, ots, obs, scale, P, dtype, None)
    return call, row, kvrow


def test_the_argument_errors_of_the_plain_entry_carry_over():
    call, row, kvrow = _caller(_lib())
    assert call(dtype=BF16) == EDTYPE and call(dtype=F32) == EDTYPE and call(dtype=7) == EDTYPE
    assert call(hd=64) == ESIZE and call(hd=96) == ESIZE and call(hd=256) == ESIZE
    assert call(tokens=0) == ESIZE and call(tokens=-5) == ESIZE and call(tokens=4097) == ESIZE
    assert call(batch=0) == ESIZE and call(batch=-1) == ESIZE and call(heads=0) == ESIZE and call(heads=-2) == ESIZE
    assert call(batch=1 << 40) == ESIZE and call(heads=1 << 40, kv=1 << 38) == ESIZE
    assert call(scale=0.0) == ESIZE and call(scale=-1.0) == ESIZE
    assert call(scale=float("inf")) == ESIZE and call(scale=float("nan")) == ESIZE
    assert call(qts=row - 8) == ESIZE and call(ots=row - 8) == ESIZE
    assert call(qbs=-8) == ESIZE and call(obs=-8) == ESIZE and call(kbs=-8) == ESIZE
    for name in ("q", "k", "v", "o"):
        assert call(**{name: None}) == ENULL, name
    assert call(cos=None) == ENULL and call(sin=None) == ENULL              # one table pointer alone
    for name in ("q", "k", "v", "o", "cos", "sin"):
        assert call(**{name: 4096 + 8}) == EALIGN, name
    assert call(qts=row + 4) == EALIGN and call(qbs=70 * row + 2) == EALIGN
    assert call(kts=kvrow + 4) == EALIGN and call(kbs=70 * kvrow + 2) == EALIGN
    assert call(ots=row + 4) == EALIGN and call(obs=70 * row + 6) == EALIGN
    # the order: dtype, sizes, nulls, alignment
    assert call(dtype=BF16, hd=64, q=None) == EDTYPE
    assert call(hd=64, q=None) == ESIZE and call(kv=3, q=None) == ESIZE and call(P=8, q=None) == ESIZE
    assert call(q=None, k=4096 + 2) == ENULL


def test_the_grouped_query_argument_errors():
    call, row, kvrow = _caller(_lib())                  # 8 heads, 2 KV heads: G = 4
    assert call(kv=0) == ESIZE and call(kv=-1) == ESIZE
    assert call(kv=3) == ESIZE and call(kv=5) == ESIZE and call(kv=16) == ESIZE     # heads % kv_heads != 0
    for P in (-1, 3, 5, 6, 7, 16, 32):                  # not one of 1, 2, 4, 8
        assert call(P=P) == ESIZE, P
    assert call(P=8) == ESIZE                           # 8 does not divide G = 4
    assert call(heads=6, kv=1, qts=6 * 128, ots=6 * 128, kts=128, P=4) == ESIZE     # 4 does not divide G = 6
    assert call(kv=8, kts=row, P=2) == ESIZE            # G = 1 admits P = 1 alone
    assert call(kts=kvrow - 8) == ESIZE                 # a kv token stride shorter than a k / v row
    # a grid past 2^31: 2^26 (sample, head) items x 32 query tiles
    assert call(batch=1 << 20, heads=1 << 6, kv=1 << 3, tokens=1024, qts=1 << 13, ots=1 << 13, kts=1 << 10) == ESIZE
    # every valid P gets past the size checks (and stops at the null pointer)
    for P in (0, 1, 2, 4):
        assert call(P=P, q=None) == ENULL, P
    assert call(kv=8, kts=row, P=1, q=None) == ENULL and call(kv=8, kts=row, P=0, q=None) == ENULL
    assert call(heads=16, kv=1, qts=2048, ots=2048, kts=128, P=8, q=None) == ENULL
    assert call(kts=kvrow + 8, kbs=0, q=None) == ENULL  # kv strides of their own


def test_the_default_heads_per_workgroup():
    """`heads_per_workgroup == 0` at G = heads / kv_heads.  The candidate was the largest of 8, 4, 2,
    1 that divides G; the measurement at G = 4 and G = 8 (profiles/r17_llama_gqa) found no P > 1 whose
    median is below P = 1's by more than P = 1's own max - min at both token counts, so by the
    project's criterion one head per workgroup is the default for every G."""
    lib = _lib()
    want = {1: 1, 2: 1, 3: 1, 4: 1, 6: 1, 8: 1, 16: 1}
    for G, P in want.items():
        assert lib.ecoflap_causal_attention_gqa_default_p(G) == P, G
    assert lib.ecoflap_causal_attention_gqa_default_p(0) == 0 and lib.ecoflap_causal_attention_gqa_default_p(-4) == 0


def test_the_new_names_are_plumbing_not_pruner_abi():
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)  # noqa: E731
    shape_ops = re.findall(r"\b(ecoflap_[a-z0-9_]+)\s*\(", strip("ecoflap_shape_ops.h"))
    abi = re.findall(r"\b(ecoflap_[a-z0-9_]+)\s*\(", strip("ecoflap_hip.h"))
    for name in ("ecoflap_causal_attention_gqa", "ecoflap_causal_attention_gqa_default_p"):
        assert name in shape_ops and name not in abi
        assert hasattr(_lib(), name)
