"""GPU: the SparseGPT trailing-update kernel and the one-call sweep (csrc/sparsegpt.hip), through
the C ABI.

  * `ecoflap_sparsegpt_trailing` against fp64 under the standard dot-product bound
    |got - exact| <= (count + 2) u (|W| + sum_k |e_k| |h_kj|), u = 2^-24, which holds for ANY
    summation order; repeatable bit for bit; nothing outside rows x [j0, cols) is written.
  * `ecoflap_sparsegpt_matrix` == the same steps composed by hand (torch's `.float()`, the block
    step, the trailing kernel, `.to(dtype)`), bit for bit: orchestration, ranks, both conversions.
  * `SparseGPT.whole_matrix_sweep` on against off (the library GEMM for the trailing product), held
    to the bounds test_gpu_parity.py sets for two factorisations that differ by rounding."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def kern():
    from ecoflap_amd import hip
    return hip.HipKernels()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("rows,count,tail", [(1, 128, 1), (33, 128, 31), (70, 32, 65), (130, 128, 200),
                                             (768, 128, 2944)])
def test_trailing_update_against_fp64(kern, rows, count, tail):
    g = torch.Generator().manual_seed(rows * 1000 + tail)
    i1, j0 = 5, 5 + count
    cols = j0 + tail
    ldw, ldh, pad_rows = cols + 3, cols + 7, 2
    W = torch.randn(rows + pad_rows, ldw, generator=g).cuda()
    Hinv = torch.randn(i1 + count + 1, ldh, generator=g).cuda()
    err = torch.randn(rows, count, generator=g).cuda()
    W0 = W.clone()

    def call(dst):
        rc = kern.lib.ecoflap_sparsegpt_trailing(dst.data_ptr(), rows, cols, ldw, err.data_ptr(), Hinv.data_ptr(),
                                                 ldh, i1, count, j0, _stream())
        assert rc == 0
        return dst

    got = call(W.clone())
    again = call(W.clone())
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))          # two calls, equal bits
    # left of j0, the pitch padding and the rows past `rows` are untouched
    assert torch.equal(got[:, :j0], W0[:, :j0]) and torch.equal(got[:, cols:], W0[:, cols:])
    assert torch.equal(got[rows:], W0[rows:])
    e64, h64, w64 = err.double(), Hinv[i1:i1 + count, j0:cols].double(), W0[:rows, j0:cols].double()
    exact = w64 - e64 @ h64
    bound = (count + 2) * U * (w64.abs() + e64.abs() @ h64.abs())
    excess = ((got[:rows, j0:cols].double() - exact).abs() - bound).max().item()
    worst = ((got[:rows, j0:cols].double() - exact).abs() / bound).max().item()
    print(f"trailing {rows}x{count}x{tail}: worst error / bound = {worst:.3f}")
    assert excess <= 0


def _inverse_factor(cols, g):
    """An upper Cholesky factor of an inverse Hessian, as `fasterprune` has it."""
    mix = 0.3 * torch.randn(cols, cols, generator=g) / cols ** 0.5 + torch.eye(cols)
    x = torch.randn(2 * cols + 64, cols, generator=g) @ mix
    H = (x.t() @ x * (2.0 / x.shape[0])).double()
    return torch.linalg.cholesky(torch.linalg.inv(H), upper=True).float().contiguous().cuda()


CASES = [
    # rows, cols, dtype, dead column, (n, m)
    (64, 96, torch.float16, None, (0, 0)),           # one ragged block, no trailing call
    (130, 328, torch.float16, 77, (0, 0)),           # ragged last block of 72, rows that fill no tile
    (130, 328, torch.bfloat16, None, (0, 0)),
    (130, 328, torch.float32, None, (2, 4)),
    (64, 96, torch.bfloat16, None, (2, 4)),
    (768, 3072, torch.float16, None, (0, 0)),        # the CLIP shapes
    (1536, 512, torch.float16, None, (0, 0)),
    (1536, 512, torch.float32, None, (0, 0)),
    (768, 3072, torch.bfloat16, None, (0, 0)),
]


@pytest.mark.parametrize("rows,cols,dtype,dead_col,nm", CASES,
                         ids=[f"{r}x{c}-{str(d)[6:]}{'-dead' if dc is not None else ''}{'-2of4' if nm[0] else ''}"
                              for r, c, d, dc, nm in CASES])
def test_one_call_equals_the_composed_steps_bit_for_bit(kern, rows, cols, dtype, dead_col, nm):
    g = torch.Generator().manual_seed(rows + cols)
    Hinv = _inverse_factor(cols, g)
    w0 = (torch.randn(rows, cols, generator=g) * 0.05).to(dtype).cuda()
    dead = None
    if dead_col is not None:
        dead = torch.zeros(cols, dtype=torch.bool, device="cuda")
        dead[dead_col] = True
    sparsity, blocksize = 0.4, 128
    ranks = [int(rows * (min(i1 + blocksize, cols) - i1) * sparsity) for i1 in range(0, cols, blocksize)]
    # by hand: the reference's sequence on the existing entry points + the trailing kernel
    W = w0.clone().float()
    if dead is not None:
        W[:, dead] = 0
    for b, i1 in enumerate(range(0, cols, blocksize)):
        i2 = min(i1 + blocksize, cols)
        err = torch.empty((rows, i2 - i1), dtype=torch.float32, device="cuda")
        if nm[0]:
            kern.sparsegpt_block_nm(W, Hinv, i1, i2 - i1, nm[0], nm[1], err)
        else:
            kern.sparsegpt_block(W, Hinv, i1, i2 - i1, ranks[b], err)
        if i2 < cols:
            kern.sparsegpt_trailing(W, err, Hinv, i1, i2 - i1, i2)
    want = W.to(dtype)
    got = w0.clone()
    kern.sparsegpt_matrix(got, Hinv, dead, blocksize, None if nm[0] else ranks, nm[0], nm[1])
    torch.cuda.synchronize()
    view = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(view), want.view(view))
    zeros = float((got == 0).float().mean())
    assert abs(zeros - (0.5 if nm[0] else sparsity)) < 0.01
    if dead is not None:
        assert bool((got[:, dead_col] == 0).all())


@pytest.mark.parametrize("cols,rows,tokens", [(320, 130, 2048), (1408, 256, 8 * 257)])
def test_whole_matrix_sweep_stays_within_rounding_of_the_library_gemm_path(kern, cols, rows, tokens):
    """The same `SparseGPT` object with `whole_matrix_sweep` on and off, inputs built as
    test_fasterprune_with_the_own_cholesky_stays_within_rounding_of_the_librarys builds them: the two
    differ only by the rounding of the trailing product, and are held to that test's bounds."""
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    g = torch.Generator().manual_seed(cols)
    mix = 0.3 * torch.randn(cols, cols, generator=g) / cols ** 0.5 + torch.eye(cols)
    xs = [(torch.randn(tokens // 4, cols, generator=g) @ mix).cuda() for _ in range(4)]
    w0 = (torch.randn(rows, cols, generator=g) * 0.05).cuda()
    out = {}
    for whole in (True, False):
        lin = torch.nn.Linear(cols, rows, bias=False).cuda()
        with torch.no_grad():
            lin.weight.copy_(w0)
        sp = SparseGPT(lin, kernels=kern)
        sp.whole_matrix_sweep = whole
        for x in xs:
            sp.add_batch(x.unsqueeze(0), None)
        sp.fasterprune(0.5)
        out[whole] = lin.weight.data.clone()
    a, b = out[True], out[False]
    masks_differ = int(((a == 0) != (b == 0)).sum())
    same_rows = ((a == 0) == (b == 0)).all(dim=1)
    worst = float((a - b)[same_rows].abs().max()) / float(b.abs().max())
    print(f"whole_matrix_sweep {rows}x{cols}: sparsity {float((a == 0).float().mean()):.4f}, {masks_differ} mask "
          f"flips of {a.numel()}, {int(same_rows.sum())} of {rows} rows with equal masks, kept weights within "
          f"{worst:.2e} of the scale")
    assert abs(float((a == 0).float().mean()) - 0.5) < 0.01
    assert masks_differ <= 2e-3 * a.numel(), (masks_differ, a.numel())
    assert int(same_rows.sum()) >= 0.8 * a.shape[0]
    assert worst <= 1e-4
