"""CPU reference of one attention head, softmax(q k^T * scale [+ causal mask]) v, for the tests of the
two kernels that share csrc/attention_tile.h (`ecoflap_vit_attention`, `ecoflap_mha_attention` /
`ecoflap_mha_attention_colsq`): the fp64 result with an elementwise a-priori error bound, a
restatement of the tile's documented arithmetic in torch CPU ops (with two switchable faults), and
the seeded inputs the tests run.  No GPU imports; all tensors are [B, H, N, D]."""
import math

import torch

U16 = 2.0 ** -11        # unit roundoff of fp16 (round to nearest)
U32 = 2.0 ** -24        # unit roundoff of fp32
P_SUBNORMAL = 2.0 ** -14    # below this an fp16 is subnormal: spacing 2^-24, rounding error <= 2^-25
LOG2E_F32 = 1.4426950408889634


def _mask(N):
    return torch.ones(N, N, dtype=torch.bool).triu_(1)      # True: key above the diagonal


def exact_and_bound(q, k, v, scale, causal):
    """fp16 q, k, v [B, H, N, D] -> (A, bound), both fp64 [B, H, N, D]: the exact attention of the
    fp16 inputs and, per element, how far a correct run of attention_tile.h's steps can land from
    it.  Per query row, with u16 = 2^-11, u32 = 2^-24:

        t_i    = scale * q.k_i (masked keys: -inf),  ta_i = scale * |q|.|k_i|
        delta  = u32 * max_i[(D + 2) * ta_i + 4 * |t_i| + 4 * |t_max|]
        rho    = 2 * delta + (N + 8) * u32
        P_i    = exp(t_i - t_max) / L,  L = sum_i exp(t_i - t_max) >= 1
        bound  = (u16 + rho + (N + 2) * u32) * sum_i P_i * |v_id|
               + 2^-25 * (sum over unmasked i of |v_id|) / L
               + u16 * |A_qd| + 2^-25

    Where each term comes from (the tile's steps, in its order):
      * S^T = K Q^T: the products of two fp16 are exact in fp32, the D-term fp32 sum is off by at
        most (D - 1) * u32 * |q|.|k_i| in ANY order of summation: (D - 1) * ta_i * u32 in units of t.
      * p = exp2(s * c2 - m * c2), c2 = fl(fl(scale) * fl(log2 e)): c2 carries three roundings
        (3 * u32 relative, acting on t_i - t_max, at most |t_i| + |t_max|), the product s * c2 one
        (u32 * |t_i|), the subtraction one (u32 * |t_i - t_max|); the rounding of m * c2 and any
        error of m itself shift every exponent of the row alike and cancel in p_i / l.  Together
        with the dot product: (D - 1) * ta_i + 5 * |t_i| + 4 * |t_max| <= (D + 2) * ta_i +
        4 * |t_i| + 4 * |t_max| (|t_i| <= ta_i), in units of u32; a fused multiply-add only drops
        a rounding.  delta is its maximum over the row's keys.
      * rho, the relative error of p_i / l before P is rounded: delta once for p_i and once for
        the sum l (a weighted mean of the same perturbations), an exp2 good to one ulp = 2 * u32
        for each of the two, the N-term fp32 row sum in any order ((N - 1) * u32), the reciprocal
        1 / l and the product o * inv (one ulp and one rounding): 2 * delta + (N + 8) * u32.
      * P is rounded to fp16 as it stands (unnormalised, p <= 1): relatively u16 in the normal
        range, and absolutely 2^-25 (half the spacing 2^-24) in the subnormal range below 2^-14;
        the absolute part reaches the output as 2^-25 * |v_id| / l per key, summed over every
        unmasked key whatever its range.
      * O^T = V^T P^T: fp16 products exact in fp32, sums of at most N + 2 terms (the padded keys of
        the last tile add exact zeros) in any order: (N + 2) * u32 on sum_i P_i * |v_id|.
      * one fp16 rounding of the output: u16 * |A_qd| in the normal range, 2^-25 below it.
    All first order in u32; no term is measured on a kernel."""
    B, H, N, D = q.shape
    if B > 8:           # (the [N, N] fp64 temporaries of a few samples at a time)
        parts = [exact_and_bound(q[b:b + 8], k[b:b + 8], v[b:b + 8], scale, causal) for b in range(0, B, 8)]
        return torch.cat([a for a, _ in parts]), torch.cat([b for _, b in parts])
    q, k, v = q.double(), k.double(), v.double()
    t = (q @ k.transpose(-1, -2)) * scale
    ta = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    seen = torch.ones(N, N, dtype=torch.bool)
    if causal:
        seen = ~_mask(N)
        t = t.masked_fill(~seen, float("-inf"))
    tmax = t.max(dim=-1, keepdim=True).values
    per_key = (D + 2) * ta + 4 * t.abs() + 4 * tmax.abs()
    delta = U32 * per_key.masked_fill(~seen, 0.0).max(dim=-1, keepdim=True).values
    rho = 2 * delta + (N + 8) * U32
    e = torch.exp(t - tmax)
    L = e.sum(dim=-1, keepdim=True)
    P = e / L
    A = P @ v
    bound = ((U16 + rho + (N + 2) * U32) * (P @ v.abs())
             + 2.0 ** -25 * (seen.double() @ v.abs()) / L
             + U16 * A.abs() + 2.0 ** -25)
    return A, bound


def emulate_tile(q, k, v, scale, causal, fault=None):
    """The arithmetic attention_tile.h documents, in torch CPU ops -> fp16 [B, H, N, D]: fp32 scores
    s, m = max s, p = exp2(s * c2 - m * c2) with c2 = scale * log2(e) in fp32, l = sum p (of the
    unrounded p), P rounded to fp16, fp32 P V, times 1 / l, one rounding to fp16.
    fault="flush": probabilities below 2^-14 (fp16 subnormals) become 0 before the fp16 rounding.
    fault="leak":  l also receives exp2(-m * c2): one padded key of score 0 with a zero V row."""
    assert fault in (None, "flush", "leak")
    N = q.shape[2]
    qf, kf, vf = q.float(), k.float(), v.float()
    s = qf @ kf.transpose(-1, -2)
    if causal:
        s = s.masked_fill(_mask(N), float("-inf"))
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)
    mc = s.max(dim=-1, keepdim=True).values * c2
    p = torch.exp2(s * c2 - mc)
    l = p.sum(dim=-1, keepdim=True)
    if fault == "leak":
        l = l + torch.exp2(-mc)
    if fault == "flush":
        p = torch.where(p < P_SUBNORMAL, torch.zeros_like(p), p)
    o = p.half().float() @ vf
    return (o * (1.0 / l)).half()


# ---- inputs ----------------------------------------------------------------------------------------

def _gen(name, B, H, N, D, causal):
    seed = sum(ord(c) for c in name) * 1000003 + ((B * 131 + H) * 521 + N) * 97 + D + (7 if causal else 0)
    return torch.Generator().manual_seed(seed)


def _randn(g, B, H, N, D):
    return torch.randn(B, H, N, D, generator=g)


def gauss(amp, B, H, N, D, causal=False):
    """q, k, v = randn * amp."""
    g = _gen(f"gauss{amp}", B, H, N, D, causal)
    return tuple((_randn(g, B, H, N, D) * amp).half() for _ in range(3))


def equal_keys(B, H, N, D, causal=False):
    """Every K row of a head equals its row 0, V is Gaussian: all scores of a query are one number,
    every unmasked probability is exactly 1 / visible, the output the plain mean of the visible V
    rows.  A key that leaks into the row sum scales the output by visible / (visible + 1) with
    nowhere to hide."""
    g = _gen("equal_keys", B, H, N, D, causal)
    q, k, v = (_randn(g, B, H, N, D).half() for _ in range(3))
    k = k[:, :, :1].expand(B, H, N, D).contiguous()
    return q, k, v


def equal_rows(B, H, N, D, causal=False):
    """`equal_keys` with every V row of a head equal to its row 0 as well.  The output is that V
    row, bit for bit: the scores of a query are identical, so s * c2 - m * c2 = 0 and p = 1
    exactly; l = visible and visible * v are exact in fp32 (11 + 9 bits); visible * fl(1 / visible)
    perturbs by about 1e-7, far below the half fp16 ulp (2.4e-4 relative) that would move the
    rounded output off v.  This also holds for any causal prefix: the mean of equal rows is the
    row."""
    g = _gen("equal_rows", B, H, N, D, causal)
    q, k, v = (_randn(g, B, H, N, D).half() for _ in range(3))
    k = k[:, :, :1].expand(B, H, N, D).contiguous()
    v = v[:, :, :1].expand(B, H, N, D).contiguous()
    return q, k, v


def subnormal_p(B, H, N, D, causal=False):
    """Key 0 has score ~ 12 (q[..., 0] = 4 against k[key 0, 0] = 3 * sqrt(D)), every other key a
    score near 0, so their unnormalised probabilities are ~ e^-12 = 2^-17.3: fp16 subnormals.  V of
    key 0 is zero and every other V row is randn + 8: the subnormal probabilities carry the whole
    output."""
    g = _gen("subnormal_p", B, H, N, D, causal)
    q = _randn(g, B, H, N, D) * 0.05
    k = _randn(g, B, H, N, D) * 0.05
    v = _randn(g, B, H, N, D) + 8.0
    q[..., 0] = 4.0
    k[..., 0] = 0.0
    k[:, :, 0, 0] = 3.0 * math.sqrt(D)
    v[:, :, 0] = 0.0
    return q.half(), k.half(), v.half()


def subnormal_fraction(q, k, scale, causal):
    """Per head, of the last query's row (every key visible to it, causal or not): the fraction of
    the unnormalised probabilities exp(t_i - t_max) that lie in (0, 2^-14), from the fp64 scores."""
    t = (q[:, :, -1:].double() @ k.double().transpose(-1, -2)) * scale
    e = torch.exp(t - t.max(dim=-1, keepdim=True).values)
    return ((e > 0) & (e < P_SUBNORMAL)).double().mean(dim=-1).flatten()


def last_key(B, H, N, D, causal=False):
    """Gaussian at amplitude 1.7 with key N - 1 = 0.9 * q of query N // 2 (causal: of query N - 1,
    the only one that sees it): that row's maximum, by a wide margin, sits in the last slot of the
    tail key tile."""
    g = _gen("last_key", B, H, N, D, causal)
    q, k, v = ((_randn(g, B, H, N, D) * 1.7).half() for _ in range(3))
    k[:, :, N - 1] = (0.9 * q[:, :, N - 1 if causal else N // 2].float()).half()
    return q, k, v


def huge_v(B, H, N, D, causal=False):
    """Gaussian q, k at amplitude 0.3 (a flat softmax), V rows alternating +65504 and -65504: the
    largest fp16 in every product, fp32 partial sums up to N * 65504 / 2, heavy cancellation."""
    g = _gen("huge_v", B, H, N, D, causal)
    q, k = ((_randn(g, B, H, N, D) * 0.3).half() for _ in range(2))
    sign = 1.0 - 2.0 * (torch.arange(N) % 2).float()
    v = (65504.0 * sign)[None, None, :, None].expand(B, H, N, D).contiguous().half()
    return q, k, v


BUILDERS = {
    "gauss0.3": lambda *a, **kw: gauss(0.3, *a, **kw),
    "gauss1.7": lambda *a, **kw: gauss(1.7, *a, **kw),
    "gauss8.0": lambda *a, **kw: gauss(8.0, *a, **kw),
    "equal_keys": equal_keys,
    "equal_rows": equal_rows,
    "subnormal_p": subnormal_p,
    "last_key": last_key,
    "huge_v": huge_v,
}


def build(name, B, H, N, D, causal=False):
    """fp16 q, k, v [B, H, N, D] of the named builder (seeded by name and shape)."""
    return BUILDERS[name](B, H, N, D, causal=causal)
