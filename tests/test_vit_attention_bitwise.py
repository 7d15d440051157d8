"""GPU: the ViT-g attention kernel's production schedule (`ecoflap_vit_attention`: 8 waves per
workgroup, query tiles split over workgroups at small batches, XCD-grouped item order) gives the
same bits as the previous schedule (`ecoflap_vit_attention_v1`), accepts exactly the same shapes,
and stays batch invariant."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H_VIT, D_VIT = 16, 88

SHAPES = ([(8, 257, 16, 88), (3, 257, 16, 88), (20, 257, 16, 88), (40, 257, 16, 88), (2, 288, 4, 72),
           (2, 220, 3, 96), (2, 33, 2, 64), (1, 1, 1, 8), (2, 100, 3, 40), (5, 197, 12, 64)]
          + [(1, 257, 16, 88), (16, 257, 16, 88), (128, 257, 16, 88)]
          + [(4, n, H_VIT, D_VIT) for n in (32, 33, 255, 256, 257, 261)])


def _both(qkv, heads, scale):
    from ecoflap_amd.shapes import fused
    with torch.no_grad():
        new = fused.vit_attention(qkv, heads, scale)
        old = fused.vit_attention_v1(qkv, heads, scale)
    torch.cuda.synchronize()
    return new, old


@pytest.mark.parametrize("B,N,H,D", SHAPES)
def test_new_schedule_equals_old_bit_for_bit(B, N, H, D):
    g = torch.Generator(device="cuda").manual_seed(7 * B + 1000 * N + D)
    scale = D ** -0.5
    for amp in (0.7, 1.7, 8.0):                     # 8: large scores, sharp softmax
        qkv = (torch.randn(B, N, 3 * H * D, device="cuda", generator=g) * amp).half()
        new, old = _both(qkv, H, scale)
        assert new is not None and old is not None
        assert torch.equal(new, old), (amp, (new.float() - old.float()).abs().max().item())
    # integer data, one-hot attention (huge scale)
    qi = torch.randint(-2, 3, (B, N, 3 * H * D), device="cuda", generator=g).half()
    new, old = _both(qi, H, 64.0)
    assert torch.equal(new, old)


@pytest.mark.parametrize("B,N,H,D", [(2, 262, 16, 88), (2, 222, 16, 96), (1, 288, 2, 96), (1, 289, 2, 8)])
def test_refused_shapes_stay_refused(B, N, H, D):
    qkv = torch.randn(B, N, 3 * H * D, device="cuda").half()
    new, old = _both(qkv, H, D ** -0.5)
    assert new is None and old is None


@pytest.mark.parametrize("B", [8, 128])
def test_batch_invariance(B):
    from ecoflap_amd.shapes import fused
    g = torch.Generator(device="cuda").manual_seed(B)
    N, H, D = 257, H_VIT, D_VIT
    qkv = (torch.randn(B, N, 3 * H * D, device="cuda", generator=g) * 1.7).half()
    with torch.no_grad():
        full = fused.vit_attention(qkv, H, D ** -0.5)
        for i in (0, B // 2, B - 1):
            alone = fused.vit_attention(qkv[i:i + 1].contiguous(), H, D ** -0.5)
            assert torch.equal(alone[0], full[i]), i
