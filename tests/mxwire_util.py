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


def assert_wire_equal(x_cpu: torch.Tensor, got: torch.Tensor,
                      want: torch.Tensor, what: str = "") -> None:
    """Two wire buffers of ``x_cpu`` byte for byte: scale bytes, payload and
    the zero padding of the last block.  On a difference, reports the first
    few elements with the input's bits, both codes and the scaled value
    x * 2^(127-b) under the expected scale byte."""
    n = x_cpu.numel()
    nblk = (n + BLOCK - 1) // BLOCK
    assert got.dtype == torch.uint8 and got.numel() == want.numel() == 33 * nblk, what
    got, want = got.reshape(-1).cpu(), want.reshape(-1).cpu()
    if torch.equal(got, want):
        return
    lines = []
    sbad = (got[32 * nblk:] != want[32 * nblk:]).nonzero().reshape(-1)
    for k in sbad[:8].tolist():
        blk = x_cpu.reshape(-1)[32 * k: 32 * k + 32].float()
        fin = blk[torch.isfinite(blk)].abs()
        amax = fin.max() if fin.numel() else torch.zeros(())
        lines.append(f"block {k}: scale byte got {got[32 * nblk + k].item()} "
                     f"want {want[32 * nblk + k].item()}, amax bits "
                     f"{amax.view(torch.int32).item() & 0xFFFFFFFF:#010x}")
    pbad = (got[: 32 * nblk] != want[: 32 * nblk]).nonzero().reshape(-1)
    flat = x_cpu.reshape(-1)
    for i in pbad[:8].tolist():
        if i >= n:
            lines.append(f"padding byte {i}: got {got[i].item():#04x}, want 0x00")
            continue
        b = want[32 * nblk + i // BLOCK].item()
        xi = flat[i: i + 1]
        width = 8 * xi.element_size()
        bits = xi.view(torch.int32 if width == 32 else torch.int16).item()
        scaled = xi.double().item() * 2.0 ** (127 - b)
        lines.append(f"element {i}: input bits {bits & ((1 << width) - 1):#x} "
                     f"({xi.item()!r}), scale byte {b}, scaled {scaled!r}: "
                     f"got {got[i].item():#04x} want {want[i].item():#04x}")
    raise AssertionError(
        f"{what}: {sbad.numel()} scale bytes and {pbad.numel()} payload bytes "
        f"of {n} elements differ\n" + "\n".join(lines))


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
