"""Block-scaled FP8 wire codec (OCP MXFP8; format spec: docs/mxwire.md).

Every 32 consecutive elements share one power-of-two scale byte (E8M0)
and travel as one OCP ``e4m3fn`` byte each.  For ``numel`` elements,
``nblk = ceil(numel/32)`` and the wire buffer is ``uint8[33*nblk]``:
payload bytes ``[0, 32*nblk)``, then one scale byte per block.  It costs
33/32 bytes per element, survives any magnitude (an unscaled e4m3 cast
zeroes gradient-sized values and overflows large ones) and, being plain
uint8, crosses RCCL and gloo alike.

``mx8_pack_torch``/``mx8_unpack_torch`` are the reference codec: integer
bit arithmetic on the fp32 view, byte-for-byte the layout the HIP kernels
(``lzy_amd.ops.mx8_pack``/``mx8_unpack``) produce.  They serve CPU tensors
and are the kernels' test oracle.  ``mx8_pack``/``mx8_unpack`` dispatch.

``mx8_axpby_torch`` is the reference of the fused decode-combine
(``lzy_amd.ops.mx8_axpby``), the combine of a wire-cast merge-tree edge
(channels/treeplan.py); ``mx8_axpby`` dispatches the same way.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch

MX_BLOCK = 32
_MX_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def mx8_nbytes(numel: int) -> int:
    return 33 * ((int(numel) + MX_BLOCK - 1) // MX_BLOCK)


def _numel(shape: Sequence[int]) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def mx8_pack_torch(t: torch.Tensor) -> torch.Tensor:
    """Encode ``t`` (f32/bf16/f16, any device) with torch ops only."""
    if t.dtype not in _MX_DTYPES:
        raise ValueError(f"mx8_pack: dtype must be f32/bf16/f16, got {t.dtype}")
    x = t.detach().reshape(-1).to(torch.float32)
    n = x.numel()
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    out = torch.empty(33 * nblk, dtype=torch.uint8, device=x.device)
    if n == 0:
        return out
    if nblk * MX_BLOCK != n:  # the padded tail encodes as 0.0
        x = torch.cat([x, x.new_zeros(nblk * MX_BLOCK - n)])
    x = x.view(nblk, MX_BLOCK)
    # amax over the block's finite elements, on raw bits (for |x| the
    # integer order is the float order)
    mag = x.view(torch.int32) & 0x7FFFFFFF
    mag = torch.where(mag < 0x7F800000, mag, torch.zeros_like(mag))
    amax = mag.amax(dim=1)
    e = amax >> 23
    m = amax & 0x7FFFFF
    # smallest 2^(b-127) with amax / 2^(b-127) <= 448 = 1.75 * 2^8
    b = (e - 8 + (m > 0x600000).to(torch.int32)).clamp_(min=0)
    mult = ((254 - b) << 23).view(torch.float32)
    v = torch.clamp(x * mult[:, None], -448.0, 448.0)  # NaN stays NaN
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where(torch.isnan(v), torch.full_like(q, 0x7F), q)
    out[: 32 * nblk] = q.reshape(-1)
    out[32 * nblk:] = b.to(torch.uint8)
    return out


def mx8_unpack_torch(buf: torch.Tensor, shape: Union[int, Sequence[int]],
                     dtype: torch.dtype) -> torch.Tensor:
    """Decode a wire buffer into a tensor of ``shape``/``dtype``."""
    if dtype not in _MX_DTYPES:
        raise ValueError(f"mx8_unpack: dtype must be f32/bf16/f16, got {dtype}")
    shape = (int(shape),) if isinstance(shape, int) else tuple(shape)
    n = _numel(shape)
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    if buf.dtype != torch.uint8 or buf.numel() != 33 * nblk:
        raise ValueError(
            f"mx8_unpack: buffer must be uint8[{33 * nblk}] for {n} elements, "
            f"got {buf.dtype}[{buf.numel()}]"
        )
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=buf.device)
    buf = buf.reshape(-1)
    q = buf[: 32 * nblk].contiguous().view(torch.float8_e4m3fn).to(torch.float32)
    b = buf[32 * nblk:].to(torch.int32)
    # 2^(b-127); b == 0 is the fp32 subnormal 2^-127
    mult = torch.where(b > 0, b << 23, torch.full_like(b, 0x00400000))
    x = q.view(nblk, MX_BLOCK) * mult.view(torch.float32)[:, None]
    return x.reshape(-1)[:n].to(dtype).reshape(shape)


def _f32(v: float) -> float:
    # the kernel takes alpha/beta as C floats
    return float(torch.tensor(float(v), dtype=torch.float32))


def mx8_axpby_torch(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``alpha*a + beta*decode(wire)`` with torch ops only: the reference
    of the fused decode-combine kernel and the CPU path of wired plans.

    The wire decodes to fp32 (never to a 16-bit type), ``p = x̂*beta`` is
    rounded to fp32 as the kernel's multiply is, ``a*alpha + p`` is
    evaluated in float64 and rounded to fp32, then to ``out_dtype``
    (default: ``a.dtype``).  The kernel's FMA rounds the exact sum once, so
    the two differ by at most the float64 rounding ahead of the fp32 one.
    """
    if a.dtype not in _MX_DTYPES:
        raise ValueError(f"mx8_axpby: dtype must be f32/bf16/f16, got {a.dtype}")
    out_dtype = a.dtype if out_dtype is None else out_dtype
    if out_dtype not in _MX_DTYPES:
        raise ValueError(
            f"mx8_axpby: out dtype must be f32/bf16/f16, got {out_dtype}"
        )
    x = mx8_unpack_torch(wire, a.numel(), torch.float32)  # checks the buffer
    p = x * torch.tensor(_f32(beta), dtype=torch.float32, device=x.device)
    af = a.detach().reshape(-1).to(torch.float64)
    r = (af * _f32(alpha) + p.to(torch.float64)).to(torch.float32)
    return r.to(out_dtype).reshape(a.shape)


def _native(t: torch.Tensor) -> bool:
    # same rule as transport.wire_pack: a device tensor on a box with the
    # HIP library takes the kernel (ops raises NativeExtensionMissing if
    # that library predates the mx8 exports — never a quiet torch detour)
    if not t.is_cuda:
        return False
    from lzy_amd import ops

    return ops.NATIVE


def mx8_pack(t: torch.Tensor) -> torch.Tensor:
    if _native(t):
        from lzy_amd import ops

        return ops.mx8_pack(t)
    return mx8_pack_torch(t)


def mx8_unpack(buf: torch.Tensor, shape: Union[int, Sequence[int]],
               dtype: torch.dtype) -> torch.Tensor:
    if _native(buf):
        from lzy_amd import ops

        return ops.mx8_unpack(buf, shape, dtype)
    return mx8_unpack_torch(buf, shape, dtype)


def mx8_axpby(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
              beta: float = 1.0,
              dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dst = alpha*a + beta*decode(wire)``; returns ``dst`` (a new tensor
    like ``a`` when not given; ``dst`` may be ``a``)."""
    if _native(a):
        from lzy_amd import ops

        return ops.mx8_axpby(a, wire, alpha, beta, dst=dst)
    if dst is None:
        return mx8_axpby_torch(a, wire, alpha, beta)
    if dst.shape != a.shape:
        raise ValueError(
            f"mx8_axpby: dst has shape {tuple(dst.shape)}, "
            f"expected {tuple(a.shape)}"
        )
    dst.copy_(mx8_axpby_torch(a, wire, alpha, beta, out_dtype=dst.dtype))
    return dst
