"""checkpoint.quantize_mxfp4 / dequantize_mxfp4 (OCP MXFP4: e2m1 codes, one e8m0 scale byte per 32 elements along K; include/vlo.h
vlo_config.weight_dtype = 2) on the CPU, no library: known answers, the wire format's nibble order, an independent restatement of the rule
(bucketize on the grid's midpoints with the tie rule) bit for bit, and the exactness of the dequantised values in bf16."""
import pytest
import torch

from videollm_online_amd.checkpoint import dequantize_mxfp4, quantize_mxfp4

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _unpack(codes):
    """uint8 [N, K/2] -> codes [N, K] (element 2j in the low nibble of byte j)"""
    return torch.stack((codes & 15, codes >> 4), dim=-1).reshape(codes.shape[0], -1)


def test_known_answer_block_ties_to_even_code_and_clamp():
    v = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0])
    x = torch.zeros(1, 32)
    x[0, :8], x[0, 8:16], x[0, 16] = v, -v, 4.0                # max|x| = 7: floor(log2) = 2, E = 0
    codes, scale = quantize_mxfp4(x)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.uint8 and tuple(codes.shape) == (1, 16) and tuple(scale.shape) == (1, 1)
    assert scale.item() == 127
    want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0])
    d = dequantize_mxfp4(codes, scale)[0]
    assert torch.equal(d[:8], want) and torch.equal(d[8:16], -want) and d[16].item() == 4.0 and not d[17:].any()
    c = _unpack(codes)[0]
    assert c[:8].tolist() == [0, 2, 2, 4, 4, 6, 6, 7] and c[8:16].tolist() == [8, 10, 10, 12, 12, 14, 14, 15]


def test_zero_block():
    x = torch.zeros(2, 64)
    x[1, 40] = 3.0                                              # one live block next to three all-zero ones
    codes, scale = quantize_mxfp4(x)
    assert scale.tolist() == [[127, 127], [127, 126]]           # 3 = 1.5 * 2^1: E = 1 - 2
    assert not codes[0].any() and not codes[1, :16].any()
    assert torch.equal(dequantize_mxfp4(codes, scale), x)


def test_nibble_order_and_code_bits():
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3], x[0, 31] = 6.0, -0.5, 1.5, -4.0, 3.0
    codes, scale = quantize_mxfp4(x)
    assert scale.item() == 127
    # sign bit 3, exponent bits 2:1, mantissa bit 0: 6 = 0b0111, -0.5 = 0b1001, 1.5 = 0b0011, -4 = 0b1110, 3 = 0b0101
    assert codes[0, 0].item() == (0b1001 << 4 | 0b0111) and codes[0, 1].item() == (0b1110 << 4 | 0b0011) and codes[0, 15].item() == 0b0101 << 4


def _restated(W):
    """The rule again, written differently: floor(log2) from log2 of the exact power-of-two bracket, the rounding as a bucketize over the
    midpoints with the tie direction per midpoint."""
    N, K = W.shape
    x = W.double().reshape(N, K // 32, 32)
    amax = x.abs().amax(-1)
    e = torch.floor(torch.log2(amax.clamp_min(2.0 ** -200)))
    e = torch.where(torch.exp2(e + 1) <= amax, e + 1, e)
    e = torch.where(torch.exp2(e) > amax, e - 1, e)             # exp2(e) <= amax < exp2(e + 1), exactly
    E = torch.where(amax > 0, (e - 2).clamp(-125, 127), torch.zeros_like(e))
    y = (x / torch.exp2(E)[..., None]).clamp(-6.0, 6.0)
    a = y.abs()
    mids = ((GRID[1:] + GRID[:-1]) / 2).double()                # 0.25 0.75 1.25 1.75 2.5 3.5 5
    up = torch.bucketize(a, mids, right=True)                   # a == midpoint counts as above it
    dn = torch.bucketize(a, mids, right=False)                  # a == midpoint counts as below it
    code = torch.where(up % 2 == 0, up, dn)                     # off a midpoint up == dn; on one, exactly one of them is even
    code = (code + 8 * (y < 0)).to(torch.uint8).reshape(N, K)
    return code, (E + 127).to(torch.uint8)


@pytest.mark.parametrize("N,K", [(256, 4096), (64, 14336)])
def test_agrees_with_an_independent_restatement(N, K):
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * K ** -0.5 * (1 + 3 * torch.rand(N, 1, generator=g))).bfloat16()
    codes, scale = quantize_mxfp4(W)
    rc, rs = _restated(W)
    assert torch.equal(scale, rs)
    assert torch.equal(_unpack(codes), rc)
    assert 2 <= int(scale.min()) and int(scale.max()) <= 254
    d = dequantize_mxfp4(codes, scale)
    assert d.dtype == torch.float32 and tuple(d.shape) == (N, K)
    assert torch.equal(d.bfloat16().float(), d)                 # every dequantised weight is a bf16 value


def test_dequantize_covers_every_code_and_scale_exactly_in_bf16():
    """all 256 code pairs under every scale byte whose largest product (6 * 2^(s - 127)) is a finite bf16: s = 2 .. 252"""
    codes = torch.arange(256, dtype=torch.uint8).repeat(251, 1)           # [251, 256] bytes = 512 codes = 16 blocks per row
    scale = torch.arange(2, 253, dtype=torch.uint8).reshape(251, 1).repeat(1, 16)
    d = dequantize_mxfp4(codes, scale)
    assert torch.isfinite(d).all() and torch.equal(d.bfloat16().float(), d)
    assert d[0].abs()[d[0] != 0].min().item() == 2.0 ** -126              # 0.5 * 2^(2 - 127): still a normal bf16


def test_rejects_a_k_that_is_not_whole_blocks():
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(4, 48))
