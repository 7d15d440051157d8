"""GPU: `ecoflap_sparsegpt_matrix_group` (csrc/sparsegpt.hip) through `HipKernels`, against the single
entry `ecoflap_sparsegpt_matrix` on clones of the same inputs: every member of a group ends with
exactly the bits of its own call — compared as integers — in fp16, bf16 and fp32, with a dead
column, under n:m with no ranks; the members differ in rows, scale and sparsity, so a pooled
histogram or a neighbour's rank changes the masks.  The call is repeatable, writes nothing past a
member's storage, and its launches per column block do not depend on the member count."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = 128
# rows, scale, sparsity: 130 rows end inside a sweep workgroup and a trailing tile, 33 and 1 likewise
MEMBERS = [(130, 0.05, 0.3), (33, 0.5, 0.5), (1, 5.0, 0.7)]
GUARD = 64


@pytest.fixture(scope="module")
def kern():
    from ecoflap_amd import hip
    return hip.HipKernels()


def _inverse_factor(cols, g):
    """An upper Cholesky factor of an inverse Hessian, as `fasterprune` has it (the construction of
    tests/test_sparsegpt_matrix_gpu.py)."""
    mix = 0.3 * torch.randn(cols, cols, generator=g) / cols ** 0.5 + torch.eye(cols)
    x = torch.randn(2 * cols + 64, cols, generator=g) @ mix
    H = (x.t() @ x * (2.0 / x.shape[0])).double()
    return torch.linalg.cholesky(torch.linalg.inv(H), upper=True).float().contiguous().cuda()


_FACTORS = {}


def factor(cols):
    if cols not in _FACTORS:
        _FACTORS[cols] = _inverse_factor(cols, torch.Generator().manual_seed(cols))
    return _FACTORS[cols]


def ranks_of(rows, cols, sparsity):
    return [int(rows * (min(i1 + BLOCK, cols) - i1) * sparsity) for i1 in range(0, cols, BLOCK)]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def weights(members, cols, dtype, seed):
    """Each member's weight inside a buffer with a guard band behind it -> (views, buffers)."""
    g = torch.Generator().manual_seed(seed)
    views, bufs = [], []
    for rows, scale, _ in members:
        buf = torch.full((rows * cols + GUARD,), 7.0, dtype=dtype).cuda()
        w = buf[:rows * cols].view(rows, cols)
        w.copy_((torch.randn(rows, cols, generator=g) * scale).to(dtype))
        views.append(w)
        bufs.append(buf)
    return views, bufs


def one_by_one(kern, ws, members, Hinv, dead, nm):
    out = []
    for w, (rows, _, sparsity) in zip(ws, members):
        c = w.clone()
        kern.sparsegpt_matrix(c, Hinv, dead, BLOCK, None if nm[0] else ranks_of(rows, w.shape[1], sparsity),
                              nm[0], nm[1])
        out.append(c)
    return out


def grouped(kern, ws, members, Hinv, dead, nm):
    ranks = None if nm[0] else [ranks_of(rows, ws[0].shape[1], s) for rows, _, s in members]
    return kern.sparsegpt_matrix_group(ws, Hinv, dead, BLOCK, ranks, nm[0], nm[1])


def expected_launches(cols, n_members, thresholded):
    blocks = -(-cols // BLOCK)
    return dict(state_clears=blocks if thresholded else 0, histogram=3 * blocks if thresholded else 0,
                sweep=blocks, trailing=blocks - 1, convert=2 * n_members)


def check(kern, members, cols, dtype, dead_col=None, nm=(0, 0)):
    Hinv = factor(cols)
    dead = None
    if dead_col is not None:
        dead = torch.zeros(cols, dtype=torch.bool, device="cuda")
        dead[dead_col] = True
    ws, bufs = weights(members, cols, dtype, seed=cols + len(members))
    want = one_by_one(kern, ws, members, Hinv, dead, nm)
    launches = grouped(kern, ws, members, Hinv, dead, nm)
    torch.cuda.synchronize()
    for i, (w, ref, buf, (rows, _, sparsity)) in enumerate(zip(ws, want, bufs, members)):
        assert torch.equal(bits(w), bits(ref)), f"member {i} ({rows} rows) differs from its own sweep"
        assert bool((buf[rows * cols:] == 7.0).all()), f"guard band of member {i}"
        if rows * cols >= 4096:
            assert abs(float((w == 0).float().mean()) - (0.5 if nm[0] else sparsity)) < 0.01
        if dead is not None:
            assert bool((w[:, dead_col] == 0).all())
    # a pooled or swapped threshold would have shown: the members' masks differ in density
    if not nm[0] and len({s for _, _, s in members}) > 1:
        fr = [float((w == 0).float().mean()) for w in ws]
        assert fr[0] < fr[1] < fr[-1] or len(ws) < 3, fr
    assert launches == expected_launches(cols, len(members), nm[0] == 0), launches
    return ws


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_three_unequal_members_equal_their_own_sweeps(kern, dtype):
    """cols 328: two full blocks and a ragged one of 72, two trailing updates."""
    check(kern, MEMBERS, 328, dtype)


def test_with_a_dead_column(kern):
    check(kern, MEMBERS, 328, torch.float16, dead_col=77)


def test_n_of_m_without_ranks(kern):
    check(kern, MEMBERS, 328, torch.float32, nm=(2, 4))


def test_a_group_of_one_is_the_single_call(kern):
    check(kern, MEMBERS[:1], 328, torch.float16)


def test_q_k_v_in_small(kern):
    check(kern, [(256, 0.05, 0.6)] * 3, 256, torch.float16)


def test_one_ragged_block_without_a_trailing_launch(kern):
    check(kern, [(64, 0.05, 0.4), (64, 0.3, 0.6)], 96, torch.float16)


def test_the_same_call_twice_gives_the_same_bits_and_a_flat_launch_count(kern):
    Hinv = factor(328)
    first, _ = weights(MEMBERS, 328, torch.float16, seed=5)
    again = [w.clone() for w in first]
    a = grouped(kern, first, MEMBERS, Hinv, None, (0, 0))
    b = grouped(kern, again, MEMBERS, Hinv, None, (0, 0))
    torch.cuda.synchronize()
    for x, y in zip(first, again):
        assert torch.equal(bits(x), bits(y))
    # per column block: one clear, three histogram launches, one sweep, one trailing update
    # (none after the last block) — for three members as for one
    alone, _ = weights(MEMBERS[:1], 328, torch.float16, seed=5)
    c = grouped(kern, alone, MEMBERS[:1], Hinv, None, (0, 0))
    torch.cuda.synchronize()
    assert a == b
    for kind in ("state_clears", "histogram", "sweep", "trailing"):
        assert a[kind] == c[kind], kind
    assert (a["state_clears"], a["histogram"], a["sweep"], a["trailing"]) == (3, 9, 3, 2)
