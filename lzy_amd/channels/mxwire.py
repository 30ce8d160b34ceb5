"""Block-scaled wire codecs (OCP MXFP8, MXINT8, MXFP4 and MXFP6; format spec:
docs/mxwire.md).

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

The ``mxi8_*`` functions are the same three layers for MXINT8: same buffer,
same scale byte position, int8 elements (``q * 2^(b-133)``, ``0x80`` is
NaN) — about a third of the error on tensors whose blocks have a narrow
dynamic range.  ``wire_codec(name)`` maps a wire name (``"mxfp8"``,
``"mxint8"``) to its dispatching ``(pack, unpack, axpby)``.

``*_axpby_pack`` / ``*_axpby2_pack`` are the step of a merge-tree node that
forwards its result: the combine and the pack of its output, one kernel
(``lzy_amd.ops.mx8_axpby_pack`` ...) for device tensors, the two torch
functions above for CPU ones.  ``wire_fused(name)`` maps a wire name to them.

The ``mx4_*`` functions are the three layers for MXFP4: e2m1 nibbles, two
per byte, ``uint8[17*nblk]`` (``mx4_nbytes``): half the link bytes of the
8-bit wires at about four times the error of MXFP8.  ``wire_nbytes(name,
numel)`` sizes a buffer of any wire; a forwarding node on this wire is one
kernel too (``lzy_amd.ops.mx4_axpby_pack`` / ``mx4_axpby2_pack``).

The ``mx6_*`` functions are the three layers for MXFP6: 6-bit e2m3 codes,
four in three bytes, ``uint8[25*nblk]`` (``mx6_nbytes``): the error of MXFP8
at 24 % fewer link bytes.  A forwarding node on this wire is one kernel as
well (``lzy_amd.ops.mx6_axpby_pack`` / ``mx6_axpby2_pack``).
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple, Union

import torch

MX_BLOCK = 32
_MX_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def mx8_nbytes(numel: int) -> int:
    return 33 * ((int(numel) + MX_BLOCK - 1) // MX_BLOCK)


def mx4_nbytes(numel: int) -> int:
    return 17 * ((int(numel) + MX_BLOCK - 1) // MX_BLOCK)


def mx6_nbytes(numel: int) -> int:
    return 25 * ((int(numel) + MX_BLOCK - 1) // MX_BLOCK)


def _numel(shape: Sequence[int]) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _blocks(t: torch.Tensor, op: str, block_bytes: int = 33):
    """``t`` as fp32 blocks ``[nblk, 32]`` (the padded tail is 0.0), the raw
    bits of each block's amax over its finite elements (for |x| the integer
    order is the float order), and the empty wire buffer."""
    if t.dtype not in _MX_DTYPES:
        raise ValueError(f"{op}: dtype must be f32/bf16/f16, got {t.dtype}")
    x = t.detach().reshape(-1).to(torch.float32)
    n = x.numel()
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    out = torch.empty(block_bytes * nblk, dtype=torch.uint8, device=x.device)
    if nblk * MX_BLOCK != n:
        x = torch.cat([x, x.new_zeros(nblk * MX_BLOCK - n)])
    x = x.view(nblk, MX_BLOCK)
    mag = x.view(torch.int32) & 0x7FFFFFFF
    mag = torch.where(mag < 0x7F800000, mag, torch.zeros_like(mag))
    return x, mag.amax(dim=1) if n else mag.new_zeros(0), out


def mx8_pack_torch(t: torch.Tensor) -> torch.Tensor:
    """Encode ``t`` (f32/bf16/f16, any device) with torch ops only."""
    x, amax, out = _blocks(t, "mx8_pack")
    nblk = x.shape[0]
    if nblk == 0:
        return out
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


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """fp32 ``2^e`` from int32 ``e`` in [-149, 127], subnormals included."""
    bits = torch.where(e >= -126, (e + 127) << 23,
                       torch.ones_like(e) << (e + 149).clamp(0, 22))
    return bits.to(torch.int32).view(torch.float32)


def mxi8_pack_torch(t: torch.Tensor) -> torch.Tensor:
    """Encode ``t`` (f32/bf16/f16, any device) as MXINT8 with torch ops only."""
    x, amax, out = _blocks(t, "mxi8_pack")
    nblk = x.shape[0]
    if nblk == 0:
        return out
    # smallest b with rne(amax * 2^(133-b)) <= 127: b = E, one more from
    # m = 0x7f0000 on (a subnormal amax: b = 0, one more from 0x7f8000 on)
    b = ((amax + torch.where(amax < 0x00800000, 0x8000, 0x10000)) >> 23).clamp_(max=254)
    # x * 2^(133-b) is exact, but 2^(133-b) is no fp32 for b < 6: two exact
    # multiplies by 2^h and 2^(e-h).  Where the first loses bits to the
    # subnormal range (e < 0 only) the result rounds to zero either way.
    e = 133 - b
    h = e >> 1
    v = (x * _pow2(h)[:, None]) * _pow2(e - h)[:, None]
    v = torch.clamp(v, -127.0, 127.0)  # +-Inf, and the b == 254 cap; NaN stays
    q = torch.where(torch.isnan(v), torch.full_like(v, -128.0), torch.round(v))
    out[: 32 * nblk] = q.to(torch.int8).view(torch.uint8).reshape(-1)
    out[32 * nblk:] = b.to(torch.uint8)
    return out


def mxi8_unpack_torch(buf: torch.Tensor, shape: Union[int, Sequence[int]],
                      dtype: torch.dtype) -> torch.Tensor:
    """Decode an MXINT8 wire buffer into a tensor of ``shape``/``dtype``."""
    if dtype not in _MX_DTYPES:
        raise ValueError(f"mxi8_unpack: dtype must be f32/bf16/f16, got {dtype}")
    shape = (int(shape),) if isinstance(shape, int) else tuple(shape)
    n = _numel(shape)
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    if buf.dtype != torch.uint8 or buf.numel() != 33 * nblk:
        raise ValueError(
            f"mxi8_unpack: buffer must be uint8[{33 * nblk}] for {n} elements, "
            f"got {buf.dtype}[{buf.numel()}]"
        )
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=buf.device)
    buf = buf.reshape(-1)
    q = buf[: 32 * nblk].contiguous().view(torch.int8).view(nblk, MX_BLOCK)
    b = buf[32 * nblk:].to(torch.int32)
    # q * 2^(b-133): exact in fp32 for every b (2^-133 is a subnormal)
    x = q.to(torch.float32) * _pow2(b - 133)[:, None]
    x = torch.where(q == -128, torch.full_like(x, float("nan")), x)
    return x.reshape(-1)[:n].to(dtype).reshape(shape)


def mx4_pack_torch(t: torch.Tensor) -> torch.Tensor:
    """Encode ``t`` (f32/bf16/f16, any device) as MXFP4 with torch ops only."""
    x, amax, out = _blocks(t, "mx4_pack", 17)
    nblk = x.shape[0]
    if nblk == 0:
        return out
    nan = ((x.view(torch.int32) & 0x7FFFFFFF) > 0x7F800000).any(dim=1)
    # smallest 2^(b-127) with amax / 2^(b-127) <= 6 = 1.5 * 2^2: E - 2, one
    # more from m = 0x400001 on (the add carries into the exponent then)
    b = (((amax + 0x3FFFFF) >> 23) - 2).clamp_(min=0)
    v = x * ((254 - b) << 23).view(torch.float32)[:, None]  # exact, or -> 0
    # e2m1 code of |v| on its bits, clamped to 6.0 (moves +-Inf only).  From
    # 1.0 on the code is exponent and top mantissa bit, rounded to nearest
    # even on the 22 bits below (a carry walks into the exponent); below,
    # 0 up to 0.25, 0.5 up to under 0.75, 1.0 from there.
    a = (v.view(torch.int32) & 0x7FFFFFFF).clamp(max=0x40C00000)
    hi = ((a + 0x1FFFFF + ((a >> 22) & 1)) >> 22) - 252
    lo = (a > 0x3E800000).to(torch.int32) + (a >= 0x3F400000).to(torch.int32)
    q = torch.where(a >= 0x3F800000, hi, lo) | ((x.view(torch.int32) >> 28) & 8)
    q = torch.where(nan[:, None], torch.zeros_like(q), q).to(torch.uint8)
    out[: 16 * nblk] = (q[:, 0::2] | (q[:, 1::2] << 4)).reshape(-1)
    out[16 * nblk:] = torch.where(nan, torch.full_like(b, 0xFF), b).to(torch.uint8)
    return out


def mx4_unpack_torch(buf: torch.Tensor, shape: Union[int, Sequence[int]],
                     dtype: torch.dtype) -> torch.Tensor:
    """Decode an MXFP4 wire buffer into a tensor of ``shape``/``dtype``."""
    if dtype not in _MX_DTYPES:
        raise ValueError(f"mx4_unpack: dtype must be f32/bf16/f16, got {dtype}")
    shape = (int(shape),) if isinstance(shape, int) else tuple(shape)
    n = _numel(shape)
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    if buf.dtype != torch.uint8 or buf.numel() != 17 * nblk:
        raise ValueError(
            f"mx4_unpack: buffer must be uint8[{17 * nblk}] for {n} elements, "
            f"got {buf.dtype}[{buf.numel()}]"
        )
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=buf.device)
    buf = buf.reshape(-1)
    p = buf[: 16 * nblk].to(torch.int32)
    q = torch.stack([p & 0xF, p >> 4], dim=1).view(nblk, MX_BLOCK)
    b = buf[16 * nblk:].to(torch.int32)[:, None]
    # |e2m1| as fp32 bits: codes 2..7 are exponent c>>1 (bias 1) and mantissa
    # bit c&1; code 1 is the subnormal 0.5
    c = q & 7
    mag = torch.where(c >= 2, (((c >> 1) + 126) << 23) | ((c & 1) << 22), c * 0x3F000000)
    mult = torch.where(b > 0, b << 23, torch.full_like(b, 0x00400000))
    x = mag.to(torch.int32).view(torch.float32) * mult.to(torch.int32).view(torch.float32)
    bits = x.view(torch.int32) | ((q & 8) << 28)  # the sign, of a zero too
    bits = torch.where(b == 0xFF, torch.full_like(bits, 0x7FC00000), bits)
    return bits.view(torch.float32).reshape(-1)[:n].to(dtype).reshape(shape)


def mx6_pack_torch(t: torch.Tensor) -> torch.Tensor:
    """Encode ``t`` (f32/bf16/f16, any device) as MXFP6 (e2m3) with torch
    ops only."""
    x, amax, out = _blocks(t, "mx6_pack", 25)
    nblk = x.shape[0]
    if nblk == 0:
        return out
    nan = ((x.view(torch.int32) & 0x7FFFFFFF) > 0x7F800000).any(dim=1)
    # smallest 2^(b-127) with amax / 2^(b-127) <= 7.5 = 1.875 * 2^2: E - 2, one
    # more from m = 0x700001 on (the add carries into the exponent then)
    b = (((amax + 0x0FFFFF) >> 23) - 2).clamp_(min=0)
    v = x * ((254 - b) << 23).view(torch.float32)[:, None]  # exact, or -> 0
    # e2m3 code of |v| on its bits, clamped to 7.5 (moves +-Inf only).  From
    # 1.0 on the code is the exponent (rebiased 127 -> 1) and the top three
    # mantissa bits, rounded to nearest even on the 20 bits below (a carry
    # walks into the exponent).  Below 1.0 the grid is k/8: adding 1.5 * 2^23
    # to 8|v| (exact) rounds to an integer by the add's own RNE and leaves it
    # in the low bits of the sum; 8 there is the code of 1.0 all the same.
    a = (v.view(torch.int32) & 0x7FFFFFFF).clamp(max=0x40F00000)
    hi = ((a + 0x7FFFF + ((a >> 20) & 1)) >> 20) - 1008
    lo = (a.view(torch.float32) * 8.0 + 12582912.0).view(torch.int32) & 0xFF
    q = torch.where(a >= 0x3F800000, hi, lo) | ((x.view(torch.int32) >> 26) & 0x20)
    q = torch.where(nan[:, None], torch.zeros_like(q), q).view(nblk, 8, 4)
    # four codes are three bytes, little-endian
    w = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)
    out[: 24 * nblk] = torch.stack(
        [w & 0xFF, (w >> 8) & 0xFF, w >> 16], dim=2).to(torch.uint8).reshape(-1)
    out[24 * nblk:] = torch.where(nan, torch.full_like(b, 0xFF), b).to(torch.uint8)
    return out


def mx6_unpack_torch(buf: torch.Tensor, shape: Union[int, Sequence[int]],
                     dtype: torch.dtype) -> torch.Tensor:
    """Decode an MXFP6 wire buffer into a tensor of ``shape``/``dtype``."""
    if dtype not in _MX_DTYPES:
        raise ValueError(f"mx6_unpack: dtype must be f32/bf16/f16, got {dtype}")
    shape = (int(shape),) if isinstance(shape, int) else tuple(shape)
    n = _numel(shape)
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    if buf.dtype != torch.uint8 or buf.numel() != 25 * nblk:
        raise ValueError(
            f"mx6_unpack: buffer must be uint8[{25 * nblk}] for {n} elements, "
            f"got {buf.dtype}[{buf.numel()}]"
        )
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=buf.device)
    buf = buf.reshape(-1)
    p = buf[: 24 * nblk].to(torch.int32).view(nblk, 8, 3)
    w = p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)
    q = torch.stack([(w >> s) & 0x3F for s in (0, 6, 12, 18)], dim=2).view(nblk, MX_BLOCK)
    b = buf[24 * nblk:].to(torch.int32)[:, None]
    # |e2m3| as fp32 bits: codes from 8 on are exponent c>>3 (bias 1) and
    # mantissa c&7; codes below are the subnormals c/8
    c = q & 0x1F
    mag = torch.where(c >= 8, (((c >> 3) + 126) << 23) | ((c & 7) << 20),
                      (c.to(torch.float32) * 0.125).view(torch.int32))
    mult = torch.where(b > 0, b << 23, torch.full_like(b, 0x00400000))
    x = mag.to(torch.int32).view(torch.float32) * mult.to(torch.int32).view(torch.float32)
    bits = x.view(torch.int32) | ((q & 0x20) << 26)  # the sign, of a zero too
    bits = torch.where(b == 0xFF, torch.full_like(bits, 0x7FC00000), bits)
    return bits.view(torch.float32).reshape(-1)[:n].to(dtype).reshape(shape)


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
    return _axpby_torch("mx8_axpby", mx8_unpack_torch, a, wire, alpha, beta,
                        out_dtype)


def mxi8_axpby_torch(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                     beta: float = 1.0,
                     out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """:func:`mx8_axpby_torch` for an MXINT8 ``wire``."""
    return _axpby_torch("mxi8_axpby", mxi8_unpack_torch, a, wire, alpha, beta,
                        out_dtype)


def mx4_axpby_torch(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """:func:`mx8_axpby_torch` for an MXFP4 ``wire``."""
    return _axpby_torch("mx4_axpby", mx4_unpack_torch, a, wire, alpha, beta,
                        out_dtype)


def mx6_axpby_torch(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """:func:`mx8_axpby_torch` for an MXFP6 ``wire``."""
    return _axpby_torch("mx6_axpby", mx6_unpack_torch, a, wire, alpha, beta,
                        out_dtype)


def _axpby_torch(op, unpack_torch, a, wire, alpha, beta, out_dtype):
    if a.dtype not in _MX_DTYPES:
        raise ValueError(f"{op}: dtype must be f32/bf16/f16, got {a.dtype}")
    out_dtype = a.dtype if out_dtype is None else out_dtype
    if out_dtype not in _MX_DTYPES:
        raise ValueError(
            f"{op}: out dtype must be f32/bf16/f16, got {out_dtype}"
        )
    x = unpack_torch(wire, a.numel(), torch.float32)  # checks the buffer
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


def _pack(op: str, pack_torch: Callable, t: torch.Tensor) -> torch.Tensor:
    if _native(t):
        from lzy_amd import ops

        return getattr(ops, op)(t)
    return pack_torch(t)


def _unpack(op: str, unpack_torch: Callable, buf, shape, dtype) -> torch.Tensor:
    if _native(buf):
        from lzy_amd import ops

        return getattr(ops, op)(buf, shape, dtype)
    return unpack_torch(buf, shape, dtype)


def _axpby(op: str, axpby_torch: Callable, a, wire, alpha, beta, dst):
    if _native(a):
        from lzy_amd import ops

        return getattr(ops, op)(a, wire, alpha, beta, dst=dst)
    if dst is None:
        return axpby_torch(a, wire, alpha, beta)
    if dst.shape != a.shape:
        raise ValueError(
            f"{op}: dst has shape {tuple(dst.shape)}, "
            f"expected {tuple(a.shape)}"
        )
    dst.copy_(axpby_torch(a, wire, alpha, beta, out_dtype=dst.dtype))
    return dst


def mx8_pack(t: torch.Tensor) -> torch.Tensor:
    return _pack("mx8_pack", mx8_pack_torch, t)


def mx8_unpack(buf: torch.Tensor, shape: Union[int, Sequence[int]],
               dtype: torch.dtype) -> torch.Tensor:
    return _unpack("mx8_unpack", mx8_unpack_torch, buf, shape, dtype)


def mx8_axpby(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
              beta: float = 1.0,
              dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dst = alpha*a + beta*decode(wire)``; returns ``dst`` (a new tensor
    like ``a`` when not given; ``dst`` may be ``a``)."""
    return _axpby("mx8_axpby", mx8_axpby_torch, a, wire, alpha, beta, dst)


def mxi8_pack(t: torch.Tensor) -> torch.Tensor:
    return _pack("mxi8_pack", mxi8_pack_torch, t)


def mxi8_unpack(buf: torch.Tensor, shape: Union[int, Sequence[int]],
                dtype: torch.dtype) -> torch.Tensor:
    return _unpack("mxi8_unpack", mxi8_unpack_torch, buf, shape, dtype)


def mxi8_axpby(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
               beta: float = 1.0,
               dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`mx8_axpby` for an MXINT8 ``wire``."""
    return _axpby("mxi8_axpby", mxi8_axpby_torch, a, wire, alpha, beta, dst)


def mx4_pack(t: torch.Tensor) -> torch.Tensor:
    return _pack("mx4_pack", mx4_pack_torch, t)


def mx4_unpack(buf: torch.Tensor, shape: Union[int, Sequence[int]],
               dtype: torch.dtype) -> torch.Tensor:
    return _unpack("mx4_unpack", mx4_unpack_torch, buf, shape, dtype)


def mx4_axpby(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
              beta: float = 1.0,
              dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`mx8_axpby` for an MXFP4 ``wire``."""
    return _axpby("mx4_axpby", mx4_axpby_torch, a, wire, alpha, beta, dst)


def mx6_pack(t: torch.Tensor) -> torch.Tensor:
    return _pack("mx6_pack", mx6_pack_torch, t)


def mx6_unpack(buf: torch.Tensor, shape: Union[int, Sequence[int]],
               dtype: torch.dtype) -> torch.Tensor:
    return _unpack("mx6_unpack", mx6_unpack_torch, buf, shape, dtype)


def mx6_axpby(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
              beta: float = 1.0,
              dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`mx8_axpby` for an MXFP6 ``wire``."""
    return _axpby("mx6_axpby", mx6_axpby_torch, a, wire, alpha, beta, dst)


def _axpby_pack(op: str, combine_torch: Callable, pack_torch: Callable, a, second,
                alpha, beta, dst, wire_out):
    """The step of a forwarding merge-tree node: ``(dst, pack(dst))``.  One
    kernel for device tensors; on CPU the combine and the pack it replaces,
    so the result is theirs bit for bit."""
    if _native(a):
        from lzy_amd import ops

        return getattr(ops, op)(a, second, alpha, beta, dst=dst, wire_out=wire_out)
    r = combine_torch(a, second, alpha, beta, a.dtype if dst is None else dst.dtype)
    if dst is None:
        dst = r
    else:
        if dst.shape != a.shape:
            raise ValueError(
                f"{op}: dst has shape {tuple(dst.shape)}, "
                f"expected {tuple(a.shape)}"
            )
        dst.copy_(r)
    packed = pack_torch(dst)
    if wire_out is None:
        return dst, packed
    wire_out.copy_(packed)
    return dst, wire_out


def _axpby2_torch(a, b, alpha, beta, out_dtype):
    # the combine of an unwired plan step on tensors the kernels do not serve
    return torch.add(a * alpha, b, alpha=beta).to(out_dtype)


def mx8_axpby_pack(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                   beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                   wire_out: Optional[torch.Tensor] = None):
    """``dst = alpha*a + beta*decode(wire)`` and ``wire_out = pack(dst)``;
    returns ``(dst, wire_out)``."""
    return _axpby_pack("mx8_axpby_pack", mx8_axpby_torch, mx8_pack_torch, a, wire,
                       alpha, beta, dst, wire_out)


def mxi8_axpby_pack(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                    wire_out: Optional[torch.Tensor] = None):
    """:func:`mx8_axpby_pack` for MXINT8 buffers."""
    return _axpby_pack("mxi8_axpby_pack", mxi8_axpby_torch, mxi8_pack_torch, a, wire,
                       alpha, beta, dst, wire_out)


def mx8_axpby2_pack(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                    wire_out: Optional[torch.Tensor] = None):
    """``dst = alpha*a + beta*b`` and ``wire_out = pack(dst)``; returns
    ``(dst, wire_out)``."""
    return _axpby_pack("mx8_axpby2_pack", _axpby2_torch, mx8_pack_torch, a, b,
                       alpha, beta, dst, wire_out)


def mxi8_axpby2_pack(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
                     beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                     wire_out: Optional[torch.Tensor] = None):
    """:func:`mx8_axpby2_pack` with an MXINT8 ``wire_out``."""
    return _axpby_pack("mxi8_axpby2_pack", _axpby2_torch, mxi8_pack_torch, a, b,
                       alpha, beta, dst, wire_out)


def mx4_axpby_pack(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                   beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                   wire_out: Optional[torch.Tensor] = None):
    """:func:`mx8_axpby_pack` for MXFP4 buffers."""
    return _axpby_pack("mx4_axpby_pack", mx4_axpby_torch, mx4_pack_torch, a, wire,
                       alpha, beta, dst, wire_out)


def mx4_axpby2_pack(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                    wire_out: Optional[torch.Tensor] = None):
    """:func:`mx8_axpby2_pack` with an MXFP4 ``wire_out``."""
    return _axpby_pack("mx4_axpby2_pack", _axpby2_torch, mx4_pack_torch, a, b,
                       alpha, beta, dst, wire_out)


def mx6_axpby_pack(a: torch.Tensor, wire: torch.Tensor, alpha: float = 1.0,
                   beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                   wire_out: Optional[torch.Tensor] = None):
    """:func:`mx8_axpby_pack` for MXFP6 buffers."""
    return _axpby_pack("mx6_axpby_pack", mx6_axpby_torch, mx6_pack_torch, a, wire,
                       alpha, beta, dst, wire_out)


def mx6_axpby2_pack(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
                    beta: float = 1.0, dst: Optional[torch.Tensor] = None,
                    wire_out: Optional[torch.Tensor] = None):
    """:func:`mx8_axpby2_pack` with an MXFP6 ``wire_out``."""
    return _axpby_pack("mx6_axpby2_pack", _axpby2_torch, mx6_pack_torch, a, b,
                       alpha, beta, dst, wire_out)


# wire name (channel_wire_cast, stream_wire_cast, a plan's "wire") -> the
# dispatching (pack, unpack, axpby), and the size of its buffer
_WIRE_CODECS = {
    "mxfp8": (mx8_pack, mx8_unpack, mx8_axpby),
    "mxint8": (mxi8_pack, mxi8_unpack, mxi8_axpby),
    "mxfp4": (mx4_pack, mx4_unpack, mx4_axpby),
    "mxfp6": (mx6_pack, mx6_unpack, mx6_axpby),
}
_WIRE_NBYTES = {"mxfp8": mx8_nbytes, "mxint8": mx8_nbytes, "mxfp4": mx4_nbytes,
                "mxfp6": mx6_nbytes}
MX_WIRES = tuple(_WIRE_CODECS)
# ... -> the dispatching (axpby_pack, axpby2_pack) of a forwarding node
_WIRE_FUSED = {
    "mxfp8": (mx8_axpby_pack, mx8_axpby2_pack),
    "mxint8": (mxi8_axpby_pack, mxi8_axpby2_pack),
    "mxfp4": (mx4_axpby_pack, mx4_axpby2_pack),
    "mxfp6": (mx6_axpby_pack, mx6_axpby2_pack),
}


def wire_codec(wire: str) -> Tuple[Callable, Callable, Callable]:
    if wire not in _WIRE_CODECS:
        raise ValueError(f"wire must be one of {MX_WIRES}, got {wire!r}")
    return _WIRE_CODECS[wire]


def wire_nbytes(wire: str, numel: int) -> int:
    """Bytes of the wire buffer that carries ``numel`` elements on ``wire``."""
    if wire not in _WIRE_NBYTES:
        raise ValueError(f"wire must be one of {MX_WIRES}, got {wire!r}")
    return _WIRE_NBYTES[wire](numel)


def wire_fused(wire: str) -> Tuple[Callable, Callable]:
    if wire not in _WIRE_FUSED:
        raise ValueError(f"wire must be one of {MX_WIRES}, got {wire!r}")
    return _WIRE_FUSED[wire]
