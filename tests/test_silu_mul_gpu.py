"""GPU: `ecoflap_silu_mul` (`fused.silu_mul`), the LLaMA MLP's `act_fn(gate) * up` in one pass,
against y64 = silu(a) * b in fp64 from the same 16-bit inputs:

    |y - y64| <= 2 ulp of the dtype at |y64|   (under the smallest normal: one subnormal step)

The kernel rounds silu(a) to the dtype and then the product, as torch's two ops do: the first
rounding costs at most 1 ulp of the product (half an ulp of silu, whose spacing relative to the
product's can be twice as coarse), the final rounding half an ulp, and the rest is left for the
fast exponential."""
import pytest
import torch

from helpers import _ulp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [8, 4104, 11008 * 3])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_within_two_ulp_of_fp64(dtype, n):
    from ecoflap_amd.shapes import fused
    g = torch.Generator().manual_seed(n + (1 if dtype == torch.bfloat16 else 0))
    a = (4 * torch.randn(n, generator=g)).to(dtype)
    b = torch.randn(n, generator=g).to(dtype)
    with torch.no_grad():
        y = fused.silu_mul(a.cuda(), b.cuda())
    assert y is not None and y.dtype == dtype and y.shape == a.shape
    a64, b64 = a.double(), b.double()
    y64 = a64 / (1 + torch.exp(-a64)) * b64
    err = (y.cpu().double() - y64).abs() / _ulp(y64, dtype)
    print(f"{dtype} n={n}: max error {err.max().item():.3f} ulp")
    assert err.max().item() <= 2.0


def test_shapes_and_refusals():
    from ecoflap_amd.shapes import fused
    a = torch.randn(2, 5, 16, device="cuda").half()
    b = torch.randn(2, 5, 16, device="cuda").half()
    with torch.no_grad():
        y = fused.silu_mul(a, b)
        assert y.shape == a.shape
        want = torch.nn.functional.silu(a) * b
        assert (y.float() - want.float()).abs().max().item() <= 2 * 2.0 ** -10 * want.abs().max().item()
        assert fused.silu_mul(a[..., :4], b[..., :4]) is not None          # 40 elements, a view: copied
        assert fused.silu_mul(a[..., :3], b[..., :3]) is None              # 30 elements
        assert fused.silu_mul(a, b[:1]) is None and fused.silu_mul(a.float(), b.float()) is None
        assert fused.silu_mul(a.cpu(), b.cpu()) is None and fused.silu_mul(a, b.bfloat16()) is None
    assert fused.silu_mul(a, b) is None                                     # autograd on
