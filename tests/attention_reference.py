"""CPU reference of one attention head, softmax(q k^T * scale [+ causal mask]) v, for the tests of the
two kernels that share csrc/attention_tile.h (`ecoflap_vit_attention`, `ecoflap_mha_attention` /
`ecoflap_mha_attention_colsq`): the fp64 result with an elementwise a-priori error bound, a
restatement of the tile's documented arithmetic in torch CPU ops (with two switchable faults), and
the seeded inputs the tests run.  The second half does the same for the streaming causal kernel
(`ecoflap_causal_attention`, csrc/attention_stream.h): its bound, its arithmetic block by block,
its rotation op for op and three tables on which the rotation is exact.  No GPU imports; all tensors
are [B, H, N, D]."""
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


# ---- the streaming causal kernel (csrc/attention_stream.h, csrc/causal_attention.hip) ---------------

STREAM_KEYS = 64        # keys per block of attention_stream.h (AS_KEYS)
STREAM_QTILE = 32       # queries of one wave


def exact_and_bound_stream(q, k, v, scale):
    """fp16 q, k, v [B, H, N, 128] (rotated already, see `rotate_documented`) -> (A, bound), both
    fp64 [B, H, N, 128]: the exact causal attention of the fp16 operands and, per element, how far
    a correct run of attention_stream.h's steps can land from it.  Query i sees the keys 0 .. i:
    n_i = i + 1 of them, in nb_i = i // 64 + 1 blocks of 64.  Per query row, with u16 = 2^-11,
    u32 = 2^-24 and t, ta, delta, P, L as in `exact_and_bound` (over the row's own keys):

        delta  = u32 * max_j[(D + 2) * ta_j + 4 * |t_j| + 4 * |t_max|]
        rho    = 2 * delta + (min(n_i, 64) + 6 * nb_i + 2) * u32
        bound  = (u16 + rho + (n_i + nb_i) * u32) * sum_j P_j * |v_jd|
               + 2^-25 * (sum over the row's keys of |v_jd|) / L
               + u16 * |A_id| + 2^-25

    The steps of `stream_block` and `stream_store`, in their order, against the two-pass derivation:
      * S^T = K Q^T, c2 and the product s * c2 are the tile's: (D - 1) * ta_j + 4 * |t_j| +
        3 * |t_max| in units of u32, before the subtraction.
      * the exponent of a key.  Block b computes m_b = max(m_{b-1}, the block's scores),
        mc_b = fl(m_b * c2), alpha_b = exp2(fl(mc_{b-1} - mc_b)) and, for its keys,
        p_j = exp2(fl(fl(s_j * c2) - mc_b)); st.m * c2 of block b + 1 is the same fp32 product
        mc_b again.  After the last block, key j of block b carries exp2 of
            fl(fl(s_j c2) - mc_b) + sum_{b' > b} fl(mc_{b'-1} - mc_{b'}).
        Without the roundings of the subtractions this telescopes to fl(s_j c2) - mc_last: the
        intermediate mc_b drop out whatever their own rounding (or any error of m_b) was, and
        mc_last is common to the row and cancels in O / l, as m * c2 does in the tile.  The
        subtractions each round relatively to u32.  m is monotone and fl and * c2 (c2 > 0)
        preserve order, so fl(s_j c2) <= mc_b <= mc_{b+1} <= ... <= mc_last: every difference has
        one sign and their magnitudes ADD UP to mc_last - fl(s_j c2).  The first subtraction costs
        u32 * (m_b - t_j), the later ones together u32 * (t_max - m_b), in sum u32 * (t_max - t_j)
        <= u32 * (|t_j| + |t_max|): what the one subtraction of the two-pass tile costs.  delta is
        therefore the tile's expression, taken over the row's own keys.
      * alpha_b is one exp2, good to one ulp = 2 * u32, and multiplies O and l alike.  It does not
        cancel: it scales only the keys of the EARLIER blocks, so it perturbs their weights
        relative to the later keys'.  A key passes at most nb_i - 1 of them: 2 * (nb_i - 1) * u32
        on its weight, once in p_j and once more in l (a weighted mean of the same perturbations):
        4 * (nb_i - 1) * u32 in rho.
      * l = fl(fl(l * alpha) + lb), lb the block's sum of its unrounded p in any order: a key's p
        passes at most min(n_i, 64) - 1 additions inside its block (masked keys are exact zeros),
        then one addition and one product per later block: (min(n_i, 64) - 1 + 2 * (nb_i - 1)) *
        u32 in rho.  With the exp2 of p_j and of l's terms (2 * u32 each), 1 / l (one ulp) and
        o * inv (one rounding): rho = 2 * delta + (min(n_i, 64) + 6 * (nb_i - 1) + 6) * u32
        <= 2 * delta + (min(n_i, 64) + 6 * nb_i + 2) * u32.
      * the first block: m = -inf, st.m * c2 - mc = -inf, alpha = exp2(-inf) = 0 exactly, times
        the zeros of `stream_init`: nothing is rounded, which the counts above already allow for.
      * P is rounded to fp16 against the block's running maximum m_b, p <= 1: relatively u16 in
        the normal range.  In the subnormal range the error is at most 2^-25 in units of
        exp2(mc_b); every later alpha is exp2 of a number <= 0, so at most 1, and the error reaches
        the end as at most 2^-25 in units of exp2(mc_last), the units of L: 2^-25 * |v_jd| / L per
        key, the tile's term unchanged.  (A p that is normal against m_b and tiny against the final
        maximum carries only the relative error.)
      * O = fl(O * alpha) + V^T f16(p): fp16 products exact in fp32; a product passes at most
        n_i - 1 additions in any order (padded and masked keys add exact zeros) and nb_i - 1
        products with alpha: (n_i + nb_i) * u32 on sum_j P_j * |v_jd| (alpha <= 1 keeps every
        partial sum below it).
      * one fp16 rounding of the output: u16 * |A_id| in the normal range, 2^-25 below it.
    exp2 results below 2^-126 may be flushed: an absolute 2^-126 per key, far below the 2^-25
    terms.  All first order in u32; no term is measured on a kernel."""
    B, H, N, D = q.shape
    q, k, v = q.double(), k.double(), v.double()
    A = torch.empty(B, H, N, D, dtype=torch.float64)
    bound = torch.empty_like(A)
    for r0 in range(0, N, 1024):            # (bounds the [rows, keys] fp64 temporaries at N = 4096)
        r1 = min(N, r0 + 1024)
        qr, kr, vr = q[:, :, r0:r1], k[:, :, :r1], v[:, :, :r1]
        rows = torch.arange(r0, r1)
        seen = torch.arange(r1)[None, :] <= rows[:, None]
        t = ((qr @ kr.transpose(-1, -2)) * scale).masked_fill(~seen, float("-inf"))
        ta = (qr.abs() @ kr.abs().transpose(-1, -2)) * scale
        tmax = t.max(dim=-1, keepdim=True).values
        per_key = (D + 2) * ta + 4 * t.abs() + 4 * tmax.abs()
        delta = U32 * per_key.masked_fill(~seen, 0.0).max(dim=-1, keepdim=True).values
        n = (rows + 1).double()[:, None]
        nb = (rows // STREAM_KEYS + 1).double()[:, None]
        rho = 2 * delta + (n.clamp(max=STREAM_KEYS) + 6 * nb + 2) * U32
        e = torch.exp(t - tmax)
        L = e.sum(dim=-1, keepdim=True)
        P = e / L
        a = P @ vr
        A[:, :, r0:r1] = a
        bound[:, :, r0:r1] = ((U16 + rho + (n + nb) * U32) * (P @ vr.abs())
                              + 2.0 ** -25 * (seen.double() @ vr.abs()) / L
                              + U16 * a.abs() + 2.0 ** -25)
    return A, bound


def emulate_stream(q, k, v, scale, fault=None):
    """The arithmetic `stream_block` and `stream_store` document, block by block in torch CPU fp32
    ops -> fp16 [B, H, N, D]: per block of 64 keys m' = max(m, the block's scores),
    alpha = exp2(m * c2 - m' * c2), p = exp2(s * c2 - m' * c2), l = l * alpha + sum p (of the
    unrounded p), O = O * alpha + f16(p) V; at the end O * (1 / l), one rounding to fp16.
    fault="flush": probabilities below 2^-14 (fp16 subnormals against the block's running maximum)
                   become 0 before the fp16 rounding.
    fault="leak":  for the queries of the last 32-query tile, l also receives exp2(-m * c2): one
                   padded key of the tail block, score 0 and a zero V row, that escaped the mask."""
    assert fault in (None, "flush", "leak")
    B, H, N, D = q.shape
    qf, kf, vf = q.float(), k.float(), v.float()
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)
    m = torch.full((B, H, N, 1), float("-inf"))
    l = torch.zeros(B, H, N, 1)
    o = torch.zeros(B, H, N, D)
    for k0 in range(0, N, STREAM_KEYS):
        k1 = min(N, k0 + STREAM_KEYS)
        rows = torch.arange(k0, N)                      # the queries that see key k0
        s = qf[:, :, k0:] @ kf[:, :, k0:k1].transpose(-1, -2)
        s = s.masked_fill(torch.arange(k0, k1)[None, :] > rows[:, None], float("-inf"))
        mo = m[:, :, k0:]
        mn = torch.maximum(mo, s.max(dim=-1, keepdim=True).values)
        mc = mn * c2
        alpha = torch.exp2(mo * c2 - mc)
        p = torch.exp2(s * c2 - mc)
        l[:, :, k0:] = l[:, :, k0:] * alpha + p.sum(dim=-1, keepdim=True)
        if fault == "flush":
            p = torch.where(p < P_SUBNORMAL, torch.zeros_like(p), p)
        o[:, :, k0:] = o[:, :, k0:] * alpha + p.half().float() @ vf[:, :, k0:k1]
        m[:, :, k0:] = mn
    if fault == "leak":
        tail = STREAM_QTILE * ((N - 1) // STREAM_QTILE)
        l[:, :, tail:] = l[:, :, tail:] + torch.exp2(-(m[:, :, tail:] * c2))
    return (o * (1.0 / l)).half()


# ---- the rotary embedding of causal_attention.hip ---------------------------------------------------

def rope_table(T, theta=10000.0):
    """fp32 cos, sin [T, 64] of positions 0 .. T - 1 (transformers' LlamaRotaryEmbedding)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    freqs = torch.arange(T, dtype=torch.float)[:, None] * inv_freq[None, :]
    return freqs.cos(), freqs.sin()


def rotate_documented(x, cos, sin):
    """fp16 x [..., T, 128], fp32 cos, sin [T, 64] -> fp16: causal_attention.hip's `rotate8` op for
    op.  Element d pairs with d + 64: lo' = fl(fl(lo * c) - fl(hi * s)), hi' = fl(fl(hi * c) +
    fl(lo * s)) in fp32 (the library is built without fma contraction), then one rounding to fp16,
    to nearest even."""
    lo, hi = x[..., :64].float(), x[..., 64:].float()
    c, s = cos.float(), sin.float()
    return torch.cat((lo * c - hi * s, hi * c + lo * s), dim=-1).half()


def identity_table(T):
    """cos = 1, sin = 0: the rotation returns its input, without a rounding."""
    return torch.ones(T, 64), torch.zeros(T, 64)


def swap_table(T):
    """cos = 0, sin = 1: lo' = -hi, hi' = lo, without a rounding."""
    return torch.zeros(T, 64), torch.ones(T, 64)


def parity_table(T):
    """`identity_table` on the even positions, `swap_table` on the odd ones: a query or key that
    reads a neighbour's table row comes out permuted."""
    odd = (torch.arange(T) % 2 == 1).float()[:, None].expand(T, 64).contiguous()
    return 1.0 - odd, odd


def swap_halves(x, odd_only=False):
    """x [..., T, 128] -> cat(-hi, lo), what `swap_table` computes; odd_only: on the odd positions
    alone, what `parity_table` computes."""
    y = torch.cat((-x[..., 64:], x[..., :64]), dim=-1)
    if odd_only:
        y = y.clone()
        y[..., 0::2, :] = x[..., 0::2, :]
    return y


EXACT_TABLES = {"identity": identity_table, "swap": swap_table, "parity": parity_table}


# ---- one more input, for the streaming kernel -------------------------------------------------------

def late_key(N):
    """Where `subnormal_p_late` puts its towering key."""
    return max(N - 70, 0)


def subnormal_p_late(B, H, N, D, causal=True):
    """`subnormal_p` with the towering key at position N - 70 (at 0 where N < 71) instead of 0, for
    a causal kernel that streams key blocks of 64.  The last 70 queries see it, in the block before
    their last or earlier: what they accumulated before it at p ~ 1 is rescaled by alpha ~ e^-12,
    and the probabilities of the 69 keys after it are fp16 subnormals; V of the big key is zero, so
    those two groups carry the whole output.  The queries before N - 70 are plain flat rows."""
    g = _gen("subnormal_p_late", B, H, N, D, causal)
    j = late_key(N)
    q = _randn(g, B, H, N, D) * 0.05
    k = _randn(g, B, H, N, D) * 0.05
    v = _randn(g, B, H, N, D) + 8.0
    q[..., 0] = 4.0
    k[..., 0] = 0.0
    k[:, :, j, 0] = 3.0 * math.sqrt(D)
    v[:, :, j] = 0.0
    return q.half(), k.half(), v.half()


def late_key_profile(q, k, scale):
    """Of the last query's row, per head, from the fp64 scores, with j = late_key(N) ->
    (alpha, before, after): alpha = exp(max of the scores before key j - t_j), the factor that
    rescales what was accumulated before j; before = the smallest exp(t_i - their own maximum) over
    the keys i < j (1.0 where j = 0); after = the fraction of the keys i > j whose exp(t_i - t_j)
    lies in (0, 2^-14)."""
    N = q.shape[2]
    j = late_key(N)
    t = ((q[:, :, -1:].double() @ k.double().transpose(-1, -2)) * scale).flatten(0, 2)     # [B * H, N]
    if j > 0:
        head = t[:, :j].max(dim=-1).values
        alpha = torch.exp(head - t[:, j])
        before = torch.exp(t[:, :j] - head[:, None]).min(dim=-1).values
    else:
        alpha, before = torch.zeros(t.shape[0], dtype=torch.float64), torch.ones(t.shape[0], dtype=torch.float64)
    e = torch.exp(t[:, j + 1:] - t[:, j:j + 1])
    after = ((e > 0) & (e < P_SUBNORMAL)).double().mean(dim=-1)
    return alpha, before, after


STREAM_BUILDERS = dict(BUILDERS, subnormal_p_late=subnormal_p_late)


def build_stream(name, B, H, N, D=128):
    """fp16 q, k, v [B, H, N, D] of the named builder for the causal kernel (`BUILDERS` plus
    `subnormal_p_late`; seeded by name and shape)."""
    return STREAM_BUILDERS[name](B, H, N, D, causal=True)
