"""GPU: the row and element-wise kernels of csrc/shape_ops.hip (`ecoflap_amd.shapes.fused`) at the
sizes where a lane, a wave, a vector or a grid-stride trip begins or ends, per element against
fp64.  Inputs are made on the CPU from a seeded generator, the fp64 reference is computed on the
CPU from the same 16-bit inputs, and only the op under test runs on the GPU.  ulp(v) is the spacing
of the dtype at |v| (under the smallest normal: one subnormal step), `helpers._ulp`.  Every test
prints its measured maximum before it asserts.

Row kernels (one 64-lane wave per row, four rows per workgroup), `ROW_SHAPES` x `KINDS`:

  sum output   s == dtype(x + r), with residual_bias r' = dtype(r + rb) first: single correctly
               rounded additions, so the CPU's are the reference, bit for bit.
  RMS norm     y = w * dtype(s * rsqrt(mean(s^2) + eps)):  |y - y64| <= 2 ulp(y64).  Rounding the
               normalised value before the product with w costs at most 1 ulp of the product, the
               final rounding half an ulp, the fp32 statistics take the rest (the reasoning of
               test_silu_mul_gpu.py).  `_rms32`, the same arithmetic in fp32 on the CPU, is at most
               1.46 ulp from fp64 over all cases of this file.
  LayerNorm    y = dtype((s - mean) * rstd * w + b), one rounding:
                   |y - y64| <= 0.5 ulp(y64) + C_LN * 2**-24 * (|t| + |b| + |mean| * rstd * |w|),
               t = (s - mean) * rstd * w.  The last term is the fp32 rounding of the mean, amplified
               by the cancellation in s - mean: without it the `offset` rows (mean 6, std 0.25) are
               past any ulp bound by arithmetic alone.  C_LN comes from the reference, not from the
               kernel: `_ln32`, the formula in fp32 on the CPU (torch's summation order), needs a
               factor of 1.23 at most over all cases of this file (3 variants x 5 shapes x 4 kinds x
               2 dtypes; the worst is fp16 (7, 520) `randn` without residual); the smallest power of
               two above that is 2, and C_LN = 4 * 2 because the kernel sums in another order
               (eight-element runs per lane, then a 64-lane tree).  A constant row gives y == dtype(b) exactly: the mean of
               d equal 11-bit values is exact in fp32 and every s - mean is 0.
  fused == unfused, and a row alone == the row in its batch: bit for bit (same arithmetic per row).
  canary       y and sum_out are three rows longer than `rows` and hold 7.0: they still do afterwards.

Element-wise kernels (grid-stride loops; the launchers cap the grid at 4096 workgroups for
gelu_mul / silu_mul / qkv_bias_add and at 8192 for bias_gelu / bias_add_residual, of 256 lanes x 8
elements): 8 elements, one ragged block, one size past the cap (`BIG_N`, `BIG_ROWS_D`, `BIG_QKV`),
and every finite bit pattern of the dtype as the activation's argument times b in {1, -1.5, 2**-10}:

  silu_mul     |y - y64| <= 2 ulp(y64) + 2**-126 * |b|  (test_silu_mul_gpu.py's bound; the floor is
               for results under fp32's smallest normal, which the device may flush to zero while
               bf16 still holds them).  The plain fp32 quotient a / (1 + exp(-a)) does not meet
               this: exp(-a) is inf for a < -88.7, the quotient -0, and at the six bf16 values
               a = -89 .. -91.5 that is up to 223 ulp from silu(a) = 2e-37, a normal bf16 number
               (the CPU's fp32 evaluation shows the same); the kernel takes a * exp(a) there.
  gelu_mul     |y - y64| <= 2 ulp(y64) + C_GELU * 2**-24 * |a * b|
  bias_gelu    |y - y64| <= 1 ulp(y64) + C_GELU * 2**-24 * |u|,   u = dtype(a + bias)
               The absolute terms are fp32 erf's rounding where 1 + erf(u / sqrt 2) cancels: the
               fp32 formula alone is 250 bf16 ulp from fp64 near u = -5.  With a factor of 1 the
               CPU's fp32 evaluation (`_gelu32`) is within 0.50 ulp (plain GELU, bound 1) and 1.25
               ulp (product with b in {1, -1.5, 2**-10}, bound 2) of fp64 over all finite arguments
               of both dtypes, and 255 bf16 ulp without it; C_GELU = 4 * 1 for the device library's
               erff.
               Where |y64| is past the dtype's largest finite value, inf of that sign is right.
               Non-finite arguments are outside the bounds: a NaN argument gives NaN.
  bias_add_residual == dtype(x + dtype(m + bias)), qkv_bias_add: q and v thirds ==
               dtype(qkv + dtype(bias)), the k third byte for byte (-0.0 planted): CPU arithmetic.

The past-the-cap cases are also compared with the same call on the first row / the first 8 * 256
elements alone, so that a wrong stride shows as a position."""
import ctypes
import functools

import pytest
import torch

from helpers import _ulp

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# (rows, d): d / 8 vectors over 64 lanes
ROW_SHAPES = [(1, 8),        # one lane has work, three of the workgroup's four waves exit
              (5, 504),      # 63 vectors: lane 63 idle; rows % 4 = 1
              (7, 520),      # 65 vectors: only lane 0 makes a second trip; rows % 4 = 3
              (6, 1408),     # 176 vectors: the ViT-g width; rows % 4 = 2
              (3, 4104)]     # 513 vectors: nine trips for lane 0, eight for the rest
KINDS = ("randn", "offset", "tiny", "const")
EPS = float(torch.tensor(1e-6, dtype=torch.float32))       # what the kernels receive (a C float)
C_LN = 8.0
C_GELU = 4.0
# one ragged trip past the launcher's grid cap: some lanes make two trips, the last one is ragged
BIG_N = 4096 * 256 * 8 + 8 * 300          # gelu_mul / silu_mul: cap 4096 workgroups x 256 lanes x 8
BIG_ROWS_D = (4100, 4104)                 # bias consumers: 16 826 400 > 8192 x 256 x 8; 513 vectors per row
BIG_QKV = (1990, 1416)                    # qkv_bias_add: 1990 x 3 x 1416 = 8 453 520 > 4096 x 256 x 8


def _fused():
    from ecoflap_amd.shapes import fused
    return fused


def _tag(dtype):
    return str(dtype).split(".")[-1]


def _seed(dtype, *ints):
    s = 1 if dtype == torch.bfloat16 else 0
    for i in ints:
        s = s * 10007 + int(i)
    return s % (2 ** 31)


def _sum(a, b):
    """dtype(a + b) on the CPU as the kernels take it: the fp32 sum, rounded to the dtype; both
    steps are correctly rounded on either machine, so the bits must agree."""
    return (a.float() + b.float()).to(a.dtype)


# ---------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _row_case(dtype, rows, d, kind):
    """x, r (a residual), m + rb (a Linear's output without its bias, and the bias), the RMS weight
    w16, the LayerNorm's fp32 w / b.  `const`: the last row of every sum is 1.5."""
    g = torch.Generator().manual_seed(_seed(dtype, rows, d, KINDS.index(kind)))

    def n(*shape):
        return torch.randn(*shape, generator=g)

    if kind == "offset":
        x, r, rb = 6 + 0.25 * n(rows, d), 0.25 * n(rows, d), 0.25 * n(d)
    elif kind == "tiny":
        x, r, rb = n(rows, d) * 2.0 ** -10, 0.5 * n(rows, d) * 2.0 ** -10, 0.2 * n(d) * 2.0 ** -10
    else:
        x, r, rb = n(rows, d), 0.5 * n(rows, d), 0.5 * n(d)
    x, r, rb = x.to(dtype), r.to(dtype), rb.to(dtype)
    m = r.clone()
    if kind == "const":
        rb = (torch.round(rb.float() * 16) / 16).clamp(-2, 2).to(dtype)     # sixteenths: 0.5 - rb is exact
        x[-1], r[-1], m[-1] = 1.0, 0.5, (0.5 - rb.float()).to(dtype)
        assert torch.equal(_sum(m[-1], rb), torch.full((d,), 0.5, dtype=dtype))
    w16 = (1 + 0.1 * n(d)).to(dtype)
    wf, bf = 1 + 0.1 * n(d), 0.1 * n(d)
    return {"x": x, "r": r, "m": m, "rb": rb, "w16": w16, "wf": wf, "bf": bf}


def _row_sums(c):
    """{variant: (residual handed to the op, its bias, the CPU's sum = the norm's input)}"""
    return {"plain": (None, None, c["x"]),
            "residual": (c["r"], None, _sum(c["x"], c["r"])),
            "residual_bias": (c["m"], c["rb"], _sum(c["x"], _sum(c["m"], c["rb"])))}


def _rms64(s, w):
    s64 = s.double()
    return w.double() * (s64 * torch.rsqrt((s64 * s64).mean(-1, keepdim=True) + EPS))


def _rms32(s, w):
    """the kernel's arithmetic in fp32 on the CPU (torch's summation order)."""
    f = s.float()
    h = (f * torch.rsqrt((f * f).mean(-1, keepdim=True) + EPS)).to(s.dtype)
    return (w.float() * h.float()).to(s.dtype)


def _ln64(s, wf, bf):
    """-> (y64, the factor of C * 2**-24 in the bound)."""
    s64, w, b = s.double(), wf.double(), bf.double()
    mean = s64.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((s64 - mean) ** 2).mean(-1, keepdim=True) + EPS)
    t = (s64 - mean) * rstd * w
    return t + b, t.abs() + b.abs() + mean.abs() * rstd * w.abs()


def _ln32(s, wf, bf):
    """the documented formula in fp32 on the CPU: the reference C_LN is taken from."""
    f = s.float()
    mean = f.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((f - mean) * (f - mean)).mean(-1, keepdim=True) + EPS)
    return (((f - mean) * rstd) * wf + bf).to(s.dtype)


def _assert_within(y, y64, k, slack, dtype, what):
    """|y - y64| <= k * ulp(y64) + slack, per element.  Past the dtype's largest finite value the
    correctly rounded result is inf: inf of y64's sign passes there.  Prints and returns the
    largest error in ulp and the largest share of the absolute term any element needed."""
    yd = y.detach().cpu().double()
    ulp = _ulp(y64, dtype)
    err = (yd - y64).abs_()
    ok = err <= k * ulp + slack                                     # (a NaN error is not ok)
    if not bool(ok.all()):
        ok |= (y64.abs() > torch.finfo(dtype).max) & torch.isinf(yd) & (torch.sign(yd) == torch.sign(y64))
    err = torch.where(ok & torch.isfinite(err), err, torch.zeros_like(err))
    ulps = (err / ulp).max().item()
    need = torch.where(slack > 0, (err - k * ulp) / slack, torch.zeros_like(err)).max().item()
    print(f"{what}: max error {ulps:.3f} ulp, {max(need, 0.0):.3f} of the absolute term used")
    if not bool(ok.all()):
        bad = (~ok).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} elements over their bound, the first at flat index {i}: "
                             f"got {y.flatten()[i].item()!r}, fp64 {y64.flatten()[i].item()!r}")
    return ulps, max(need, 0.0)


def _norm(c):
    d = c["wf"].numel()
    norm = torch.nn.LayerNorm(d, eps=1e-6).cuda()
    norm.weight.data.copy_(c["wf"])
    norm.bias.data.copy_(c["bf"])
    return norm


def _cuda(t):
    return None if t is None else t.cuda()


def _rms(x, r, w):
    """-> (sum or None, y) from fused.t5_rmsnorm / fused.t5_add_rmsnorm."""
    fused = _fused()
    with torch.no_grad():
        if r is None:
            y = fused.t5_rmsnorm(x, w, 1e-6)
            assert y is not None
            return None, y
        out = fused.t5_add_rmsnorm(x, r, w, 1e-6)
    assert out is not None
    return out


def _ln(x, r, norm, rb=None):
    """-> (sum or x, y) from fused.add_layernorm."""
    with torch.no_grad(), torch.autocast("cuda", dtype=x.dtype):
        out = _fused().add_layernorm(x, r, norm, residual_bias=rb)
    assert out is not None
    return out


@pytest.mark.parametrize("rows,d", ROW_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_sum_bit_for_bit_and_output_within_two_ulp_of_fp64(dtype, rows, d):
    worst = 0.0
    for kind in KINDS:
        c = _row_case(dtype, rows, d, kind)
        sums = _row_sums(c)
        w = c["w16"].cuda()
        for variant in ("plain", "residual"):
            r, _, s_cpu = sums[variant]
            s, y = _rms(c["x"].cuda(), _cuda(r), w)
            if r is not None:
                assert torch.equal(s.cpu(), s_cpu), (kind, variant)
            assert y.dtype == dtype and y.shape == (rows, d)
            y64 = _rms64(s_cpu, c["w16"])
            worst = max(worst, _assert_within(y, y64, 2, torch.zeros(()), dtype,
                                              f"t5 rmsnorm {_tag(dtype)} {rows}x{d} {kind} {variant}")[0])
    print(f"t5 rmsnorm {_tag(dtype)} {rows}x{d}: max error {worst:.3f} ulp (bound 2)")


@pytest.mark.parametrize("rows,d", ROW_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_sum_bit_for_bit_and_output_against_fp64(dtype, rows, d):
    worst = 0.0
    for kind in KINDS:
        c = _row_case(dtype, rows, d, kind)
        norm = _norm(c)
        for variant, (r, rb, s_cpu) in _row_sums(c).items():
            s, y = _ln(c["x"].cuda(), _cuda(r), norm, _cuda(rb))
            assert torch.equal(s.cpu(), s_cpu), (kind, variant)
            assert y.dtype == dtype and y.shape == (rows, d)
            y64, slack = _ln64(s_cpu, c["wf"], c["bf"])
            _, need = _assert_within(y, y64, 0.5, C_LN * 2.0 ** -24 * slack, dtype,
                                     f"layernorm {_tag(dtype)} {rows}x{d} {kind} {variant}")
            if kind == "const":
                assert torch.equal(y[-1].cpu(), c["bf"].to(dtype)), (kind, variant)
            worst = max(worst, need)
    print(f"layernorm {_tag(dtype)} {rows}x{d}: needs C_LN = {worst * C_LN:.3f} (has {C_LN})")


@pytest.mark.parametrize("rows,d", ROW_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_norms_equal_the_unfused_ones_and_rows_are_independent(dtype, rows, d):
    for kind in KINDS:
        c = _row_case(dtype, rows, d, kind)
        sums = _row_sums(c)
        x, w, norm = c["x"].cuda(), c["w16"].cuda(), _norm(c)
        # the add fused in front == the norm alone on the CPU's rounded sum
        s_r = sums["residual"][2].cuda()
        _, y_fused = _rms(x, c["r"].cuda(), w)
        _, y_alone = _rms(s_r, None, w)
        assert torch.equal(y_fused, y_alone), (kind, "t5_add_rmsnorm")
        _, ln_fused = _ln(x, c["r"].cuda(), norm)
        _, ln_alone = _ln(s_r, None, norm)
        assert torch.equal(ln_fused, ln_alone), (kind, "add_layernorm")
        s_b, ln_bias = _ln(x, c["m"].cuda(), norm, c["rb"].cuda())
        s_b2, ln_bias2 = _ln(x, _sum(c["m"], c["rb"]).cuda(), norm)
        assert torch.equal(s_b, s_b2) and torch.equal(ln_bias, ln_bias2), (kind, "residual_bias")
        # a row alone == the row inside its batch (first and last row)
        for i in sorted({0, rows - 1}):
            xi, ri, mi = x[i:i + 1], c["r"][i:i + 1].cuda(), c["m"][i:i + 1].cuda()
            assert torch.equal(_rms(xi, None, w)[1], _rms(x, None, w)[1][i:i + 1]), (kind, i)
            assert torch.equal(_rms(xi, ri, w)[1], y_fused[i:i + 1]), (kind, i)
            assert torch.equal(_ln(xi, None, norm)[1], _ln(x, None, norm)[1][i:i + 1]), (kind, i)
            assert torch.equal(_ln(xi, ri, norm)[1], ln_fused[i:i + 1]), (kind, i)
            assert torch.equal(_ln(xi, mi, norm, c["rb"].cuda())[1], ln_bias[i:i + 1]), (kind, i)


@pytest.mark.parametrize("rows,d", ROW_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_kernels_write_nothing_past_the_last_row(dtype, rows, d):
    """The C entry points, called directly: the wrappers allocate exactly `rows` rows, so what a
    workgroup's waves past the last row do would not show.  `y` and `sum_out` are three rows
    longer than `rows` here, which covers every wave of the last workgroup."""
    from ecoflap_amd import hip
    fused = _fused()
    lib = fused._get()
    code = hip.DTYPE_CODE[dtype]
    c = _row_case(dtype, rows, d, "randn")
    x, r, m, rb, w = (c[k].cuda() for k in ("x", "r", "m", "rb", "w16"))
    norm = _norm(c)
    wf, bf = norm.weight.data, norm.bias.data

    def padded():
        return torch.full((rows + 3, d), 7.0, dtype=dtype, device="cuda")

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def check(what, rc, y, s, want_s, want_y):
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        assert bool((y[rows:] == 7.0).all()), f"{what}: y written past row {rows}"
        assert bool((s[rows:] == 7.0).all()), f"{what}: sum_out written past row {rows}"
        assert torch.equal(y[:rows], want_y), what
        if want_s is None:
            assert bool((s == 7.0).all()), f"{what}: sum_out written without a residual"
        else:
            assert torch.equal(s[:rows], want_s), what

    y, s = padded(), padded()
    rc = lib.ecoflap_t5_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, d, 1e-6, code, stream())
    check("t5_rmsnorm", rc, y, s, None, _rms(x, None, w)[1])
    y, s = padded(), padded()
    rc = lib.ecoflap_t5_add_rmsnorm(x.data_ptr(), r.data_ptr(), w.data_ptr(), s.data_ptr(), y.data_ptr(),
                                    rows, d, 1e-6, code, stream())
    check("t5_add_rmsnorm", rc, y, s, *_rms(x, r, w))
    y, s = padded(), padded()
    rc = lib.ecoflap_add_layernorm(x.data_ptr(), None, wf.data_ptr(), bf.data_ptr(), s.data_ptr(),
                                   y.data_ptr(), rows, d, 1e-6, code, stream())
    check("add_layernorm", rc, y, s, None, _ln(x, None, norm)[1])
    y, s = padded(), padded()
    rc = lib.ecoflap_add_layernorm(x.data_ptr(), r.data_ptr(), wf.data_ptr(), bf.data_ptr(), s.data_ptr(),
                                   y.data_ptr(), rows, d, 1e-6, code, stream())
    check("add_layernorm + residual", rc, y, s, *_ln(x, r, norm))
    y, s = padded(), padded()
    rc = lib.ecoflap_add_bias_layernorm(x.data_ptr(), m.data_ptr(), rb.data_ptr(), wf.data_ptr(),
                                        bf.data_ptr(), s.data_ptr(), y.data_ptr(), rows, d, 1e-6, code, stream())
    check("add_bias_layernorm", rc, y, s, *_ln(x, m, norm, rb))


# ---------------------------------------------------------------------------------------------
# element-wise kernels
# ---------------------------------------------------------------------------------------------
def _gelu64(a64):
    return 0.5 * a64 * torch.special.erfc(-a64 * 0.5 ** 0.5)       # (erfc: no cancellation in the left tail)


def _silu64(a64):
    return a64 / (1 + torch.exp(-a64))


def _gelu32(a):
    """the kernels' formula in fp32 on the CPU: the reference C_GELU is taken from."""
    f = a.float()
    return 0.5 * f * (1.0 + torch.erf(f * 0.70710678118654752440))


def _gelu_mul_check(y, a, b, what):
    dtype = a.dtype
    a64, b64 = a.double(), b.double()
    y64 = _gelu64(a64) * b64
    return _assert_within(y, y64, 2, C_GELU * 2.0 ** -24 * (a64 * b64).abs(), dtype, what)[0]


def _silu_mul_check(y, a, b, what):
    dtype = a.dtype
    a64, b64 = a.double(), b.double()
    y64 = _silu64(a64) * b64
    return _assert_within(y, y64, 2, 2.0 ** -126 * b64.abs(), dtype, what)[0]


def _bias_gelu_check(y, a, bias, what):
    dtype = a.dtype
    u64 = _sum(a, bias.expand_as(a)).double()
    y64 = _gelu64(u64)
    return _assert_within(y, y64, 1, C_GELU * 2.0 ** -24 * u64.abs(), dtype, what)[0]


MUL_OPS = {"gelu_mul": _gelu_mul_check, "silu_mul": _silu_mul_check}


def _all_finite(dtype):
    """every finite bit pattern of `dtype`, subnormals and both zeros included."""
    a = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    a = a[torch.isfinite(a)]
    assert a.numel() == {torch.float16: 63488, torch.bfloat16: 65280}[dtype] and a.numel() % 8 == 0
    return a.contiguous()


@functools.lru_cache(maxsize=None)
def _mul_case(dtype, n):
    g = torch.Generator().manual_seed(_seed(dtype, n))
    a = (3 * torch.randn(n, generator=g)).to(dtype)
    b = torch.randn(n, generator=g).to(dtype)
    return a, b


@pytest.mark.parametrize("n", [8, 2056, BIG_N])
@pytest.mark.parametrize("op", sorted(MUL_OPS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_mul_and_silu_mul_against_fp64(dtype, op, n):
    a, b = _mul_case(dtype, n)
    fn = getattr(_fused(), op)
    with torch.no_grad():
        ag, bg = a.cuda(), b.cuda()
        y = fn(ag, bg)
        assert y is not None and y.dtype == dtype and y.shape == a.shape
        MUL_OPS[op](y, a, b, f"{op} {_tag(dtype)} n={n}")
        if n > 8 * 256:
            head = fn(ag[:8 * 256], bg[:8 * 256])
            assert torch.equal(head, y[:8 * 256])


@pytest.mark.parametrize("op", sorted(MUL_OPS) + ["bias_gelu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_activations_over_every_finite_argument(dtype, op):
    """a = every finite value of the dtype, b in {1, -1.5, 2**-10}: the activation's whole domain,
    and the scalar `round` of the intermediate against the packed converts of the stores."""
    fused = _fused()
    a1 = _all_finite(dtype)
    with torch.no_grad():
        if op == "bias_gelu":
            a = a1.view(-1, 8)
            bias = torch.zeros(8, dtype=dtype)
            y = fused.bias_gelu(a.cuda(), bias.cuda())
            _bias_gelu_check(y, a, bias, f"{op} {_tag(dtype)} all finite a")
        else:
            a = a1.repeat(3)
            b = torch.cat([torch.full_like(a1, v) for v in (1.0, -1.5, 2.0 ** -10)])
            y = getattr(fused, op)(a.cuda(), b.cuda())
            assert y is not None
            MUL_OPS[op](y, a, b, f"{op} {_tag(dtype)} all finite a x b in (1, -1.5, 2**-10)")
        # a NaN argument gives NaN, and only there
        a = torch.tensor([float("nan"), 1.0, -1.0, 0.0, 2.0, -2.0, 0.5, -0.5], dtype=dtype)
        if op == "bias_gelu":
            y = fused.bias_gelu(a.view(1, 8).cuda(), torch.zeros(8, dtype=dtype).cuda()).view(-1)
        else:
            y = getattr(fused, op)(a.cuda(), torch.ones(8, dtype=dtype).cuda())
        assert bool(torch.isnan(y[0])) and bool(torch.isfinite(y[1:]).all())


@functools.lru_cache(maxsize=None)
def _bias_case(dtype, rows, d):
    g = torch.Generator().manual_seed(_seed(dtype, rows, d, 5))
    m = (2 * torch.randn(rows, d, generator=g)).to(dtype)          # a Linear's output without its bias
    x = torch.randn(rows, d, generator=g).to(dtype)
    bias = (0.5 * torch.randn(d, generator=g)).to(dtype)
    return m, x, bias


@pytest.mark.parametrize("rows,d", [(1, 8), (3, 520), BIG_ROWS_D])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_gelu_against_fp64(dtype, rows, d):
    fused = _fused()
    m, _, bias = _bias_case(dtype, rows, d)
    with torch.no_grad():
        mg, bg = m.cuda(), bias.cuda()
        y = fused.bias_gelu(mg, bg)
        assert y.dtype == dtype and y.shape == m.shape
        yc = y.cpu()
        step = 1025                                                 # (fp64 temporaries of 4 M elements)
        worst = max(_bias_gelu_check(yc[i:i + step], m[i:i + step], bias,
                                     f"bias_gelu {_tag(dtype)} {rows}x{d} rows {i}..")
                    for i in range(0, rows, step))
        print(f"bias_gelu {_tag(dtype)} {rows}x{d}: max error {worst:.3f} ulp")
        assert torch.equal(fused.bias_gelu(mg[:1], bg), y[:1])      # the first row alone


@pytest.mark.parametrize("rows,d", [(1, 8), (3, 520), BIG_ROWS_D])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_add_residual_is_the_cpu_arithmetic_bit_for_bit(dtype, rows, d):
    fused = _fused()
    m, x, bias = _bias_case(dtype, rows, d)
    with torch.no_grad():
        xg, mg, bg = x.cuda(), m.cuda(), bias.cuda()
        y = fused.bias_add_residual(xg, mg, bg)
        assert y.dtype == dtype and y.shape == x.shape
        want = _sum(x, _sum(m, bias.expand_as(m)))
        diff = (y.cpu().view(torch.int16) != want.view(torch.int16)).flatten().nonzero()
        print(f"bias_add_residual {_tag(dtype)} {rows}x{d}: {diff.numel()} elements differ")
        assert diff.numel() == 0, f"first difference at flat index {int(diff[0])}"
        assert torch.equal(fused.bias_add_residual(xg[:1], mg[:1], bg), y[:1])


@pytest.mark.parametrize("rows,dim", [(1, 8), (3, 520), BIG_QKV])
@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_bias_add_is_the_cpu_arithmetic_and_leaves_k_alone(dtype, rows, dim):
    fused = _fused()
    g = torch.Generator().manual_seed(_seed(dtype, rows, dim, 9))
    qkv = torch.randn(rows, 3 * dim, generator=g).to(dtype)
    qkv[:, dim:2 * dim:3] = -0.0                                     # k + 0 would make these +0.0
    qkv[:, ::7] = -0.0
    qb, vb = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    qb[::5] = 0.0
    want = qkv.clone()
    want[:, :dim] = _sum(qkv[:, :dim], qb.to(dtype).expand(rows, dim))
    want[:, 2 * dim:] = _sum(qkv[:, 2 * dim:], vb.to(dtype).expand(rows, dim))
    with torch.no_grad():
        got = fused.qkv_bias_add(qkv.cuda(), qb.cuda(), vb.cuda())
        assert got is not None
        gc = got.cpu()
        assert torch.equal(gc[:, dim:2 * dim].contiguous().view(torch.int16),
                           qkv[:, dim:2 * dim].contiguous().view(torch.int16)), "the k third changed"
        diff = (gc.view(torch.int16) != want.view(torch.int16)).flatten().nonzero()
        print(f"qkv_bias_add {_tag(dtype)} {rows}x3x{dim}: {diff.numel()} elements differ")
        assert diff.numel() == 0, f"first difference at flat index {int(diff[0])}"
        assert torch.equal(fused.qkv_bias_add(qkv[:1].cuda(), qb.cuda(), vb.cuda()), got[:1])


# ---------------------------------------------------------------------------------------------
# what the wrappers refuse
# ---------------------------------------------------------------------------------------------
def _off_by_8_bytes(t):
    """the same values in a contiguous tensor that starts 8 bytes after a 16-byte boundary."""
    n = 8 // t.element_size()
    buf = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
    view = buf[n:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view


@pytest.mark.parametrize("dtype", DTYPES)
def test_pointers_off_a_16_byte_boundary_go_to_the_torch_ops(dtype):
    """The kernels read and write 16-byte vectors.  ecoflap_add_layernorm, ecoflap_add_bias_layernorm
    and ecoflap_qkv_bias_add answer ECOFLAP_EALIGN (-5) like their siblings, and the wrappers
    return None for it (the caller runs the torch ops) instead of raising."""
    fused = _fused()
    c = _row_case(dtype, 5, 504, "randn")
    x, r, rb = c["x"].cuda(), c["r"].cuda(), c["rb"].cuda()
    norm = _norm(c)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        assert fused.add_layernorm(x, r, norm, residual_bias=rb) is not None
        assert fused.add_layernorm(_off_by_8_bytes(x), None, norm) is None
        assert fused.add_layernorm(x, _off_by_8_bytes(r), norm) is None
        assert fused.add_layernorm(x, r, norm, residual_bias=_off_by_8_bytes(rb)) is None
        off = _norm(c)
        off.bias.data = _off_by_8_bytes(off.bias.data)
        assert fused.add_layernorm(x, r, off) is None
        off = _norm(c)
        off.weight.data = _off_by_8_bytes(off.weight.data)
        assert fused.add_layernorm(x, None, off) is None
        # the parameters' dtype and device: both, not the weight's alone
        off = _norm(c)
        off.bias.data = off.bias.data.to(dtype)
        assert fused.add_layernorm(x, r, off) is None
        off = _norm(c)
        off.bias.data = off.bias.data.cpu()
        assert fused.add_layernorm(x, r, off) is None
    qkv = torch.randn(3, 3 * 504, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
    qb, vb = c["wf"].cuda(), c["bf"].cuda()
    with torch.no_grad():
        before = qkv.clone()
        assert fused.qkv_bias_add(qkv, _off_by_8_bytes(qb), vb) is None
        assert fused.qkv_bias_add(qkv, qb, _off_by_8_bytes(vb)) is None
        assert torch.equal(qkv, before)                                # refused before anything ran
        off = _off_by_8_bytes(qkv)
        assert fused.qkv_bias_add(off, qb, vb) is None and torch.equal(off, before)
        assert fused.qkv_bias_add(qkv, qb, vb) is qkv and not torch.equal(qkv, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_consumers_read_only_a_bias_row_of_their_own_dtype(dtype):
    """`bias_gelu` / `bias_add_residual` hand `bias.data_ptr()` to a kernel that reads d values of
    the activation's dtype in 16-byte vectors: any other bias (fp32 under autocast, another
    length, a strided or misaligned view, another device) takes the torch op chain."""
    import torch.nn.functional as F
    fused = _fused()
    m, x, bias = (t.cuda() for t in _bias_case(dtype, 3, 520))
    with torch.no_grad():
        fast_g, fast_r = fused.bias_gelu(m, bias), fused.bias_add_residual(x, m, bias)
        wide = torch.stack((bias, bias), 1)[:, 0]                       # every second element
        assert not wide.is_contiguous()
        for other in (_off_by_8_bytes(bias), wide):                     # the same values: the same sums
            assert torch.equal(fused.bias_add_residual(x, m, other), fast_r)
            assert torch.equal(fused.bias_gelu(m, other), F.gelu(m + other))
        b32 = bias.float() + 2.0 ** -12                                 # not representable in 16 bits
        assert torch.equal(fused.bias_gelu(m, b32), F.gelu(m + b32))
        assert torch.equal(fused.bias_add_residual(x, m, b32), x + (m + b32))
        one = bias[:1].contiguous()                                     # broadcasts in torch; not a row of d
        assert torch.equal(fused.bias_gelu(m, one), F.gelu(m + one))
        assert torch.equal(fused.bias_add_residual(x, m, one), x + (m + one))
        _bias_gelu_check(fast_g, m.cpu(), bias.cpu(), f"bias_gelu {_tag(dtype)} 3x520")


def test_pinned_block_with_fp32_biases_under_autocast_keeps_them_in_its_linears(monkeypatch):
    """torch runs a Linear with a 16-bit weight and an fp32 bias under autocast.  A `pin_linears`
    block of such Linears must not defer those biases to the 16-bit bias consumers (their bytes
    would be read as 16-bit values): `take_pending_bias` answers None, and the block computes what
    the plain block computes, to the bound test_pinned_gemm.py sets for the same comparison with
    16-bit biases (2e-2 of the output's maximum: two GEMM kernels, fp16 rounding between the ops)."""
    import copy
    from ecoflap_amd.shapes.eva_vit import Block, half_linear_weights
    fused = _fused()
    monkeypatch.setenv("ECOFLAP_PINNED_GEMM", "1")          # every Linear on its pinned solution: deferral is live
    torch.manual_seed(4)
    plain = Block(1408, 16, 6144).eval()
    for p in plain.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.0, 0.05)              # non-zero biases
    plain.norm1.weight.data.add_(1.0)
    plain.norm2.weight.data.add_(1.0)
    half_linear_weights(plain)
    x = (torch.randn(1, 257, 1408) * 0.5).half().cuda()
    plain = plain.cuda()
    lins = lambda blk: (blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)         # noqa: E731
    # control: with 16-bit biases the pinned block does defer
    pinned16 = copy.deepcopy(plain)
    fused.pin_linears(pinned16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        with fused.deferring_bias(pinned16.mlp.fc1):
            pinned16.mlp.fc1(x)
        assert fused.take_pending_bias(pinned16.mlp.fc1) is pinned16.mlp.fc1.bias
    for lin in lins(plain):
        lin.bias.data = lin.bias.data.float()
    pinned = copy.deepcopy(plain)
    assert fused.pin_linears(pinned) == 4
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for lin, ref in zip(lins(pinned), lins(plain)):
            h = x if lin.in_features == 1408 else torch.cat([x] * 5, -1)[..., :6144].contiguous()
            with fused.deferring_bias(lin):
                out = lin(h)
            assert fused.take_pending_bias(lin) is None
            want = ref(h)
            assert out.dtype == want.dtype == torch.float16
            assert (out.float() - want.float()).abs().max().item() <= 2e-2 * want.float().abs().max().item()
        y0 = plain(x, None).float()
        y1 = pinned(x, None).float()
    assert not any(m.__dict__.get("_bias_pending") for m in pinned.modules())
    err = (y0 - y1).abs().max().item()
    print(f"pinned block, fp32 biases: max difference {err:.3e} at output scale {y0.abs().max().item():.3f}")
    assert bool(torch.isfinite(y1).all()) and err <= 2e-2 * y0.abs().max().item(), err
