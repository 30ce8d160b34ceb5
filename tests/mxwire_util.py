"""Shared helpers of the block-scaled FP8 (mxfp8) wire tests."""
import torch

BLOCK = 32


def block_amax(x: torch.Tensor) -> torch.Tensor:
    """Per-element amax of the element's 32-block (fp32, finite inputs)."""
    flat = x.detach().reshape(-1).float().cpu()
    n = flat.numel()
    nblk = (n + BLOCK - 1) // BLOCK
    pad = torch.zeros(nblk * BLOCK)
    pad[:n] = flat.abs()
    amax = pad.view(nblk, BLOCK).amax(dim=1, keepdim=True)
    return amax.expand(nblk, BLOCK).reshape(-1)[:n]


def error_bound(x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """|x^ - x| <= 2^-4 |x| + amax_block 2^-17 (+ 2^-8 |x| for 16-bit out).

    e4m3 has 3 mantissa bits: half an ulp of a normal is 2^-4 relative.
    The scaled amax is > 224, and the scaled e4m3 subnormal step is 2^-9
    (half: 2^-10), so the absolute term is amax * 2^-10 / 224 < amax *
    2^-17.  Rounding the decoded value to bf16/f16 adds at most 2^-8
    (bf16: 2^-9 relative of a value <= (1 + 2^-4)|x|)."""
    ax = x.detach().reshape(-1).double().cpu().abs()
    bound = ax * 2.0 ** -4 + block_amax(x).double() * 2.0 ** -17
    if out_dtype in (torch.bfloat16, torch.float16):
        bound = bound + ax * 2.0 ** -8
    return bound


def assert_within_bound(got: torch.Tensor, x: torch.Tensor,
                        out_dtype: torch.dtype) -> float:
    """Assert the per-element bound; returns the relative L2 error."""
    g = got.detach().reshape(-1).double().cpu()
    w = x.detach().reshape(-1).double().cpu()
    assert g.shape == w.shape
    err = (g - w).abs()
    bound = error_bound(x, out_dtype)
    worst = (err - bound).max().item()
    assert worst <= 0, f"per-element bound exceeded by {worst}"
    return (err.norm() / w.norm().clamp_min(1e-300)).item()


def special_vector() -> torch.Tensor:
    """Four blocks: [zeros] [nan,1,0..] [inf,-inf,2,0..] [896,-1.75,3e38,1e-45,0..]."""
    v = torch.zeros(4 * BLOCK, dtype=torch.float32)
    v[32], v[33] = float("nan"), 1.0
    v[64], v[65], v[66] = float("inf"), float("-inf"), 2.0
    v[96], v[97], v[98], v[99] = 896.0, -1.75, 3e38, 1e-45
    return v


def check_special_decode(scales: torch.Tensor, dec: torch.Tensor) -> None:
    """Assertions on the wire scale bytes and the f32 decode of special_vector()."""
    assert scales.tolist() == [0, 119, 120, 247]
    dec = dec.reshape(-1).float().cpu()
    nan_idx = torch.isnan(dec).nonzero().reshape(-1).tolist()
    assert nan_idx == [32], nan_idx
    assert dec[33].item() == 1.0
    assert dec[64].item() == 3.5 and dec[65].item() == -3.5
    assert dec[66].item() == 2.0
    assert torch.equal(dec[:32], torch.zeros(32))
    assert dec[:32].view(torch.int32).eq(0).all()  # +0.0 exactly
    assert not torch.isinf(dec).any()
