"""HIP/CDNA4 data-plane kernels (gfx950).

``libhipops.so`` is the in-tree HIP library (lzy_amd/ops/hipops.hip):
vectorized pack/cast and the content-checksum kernels, launched on the
caller's current torch HIP stream via a thin ctypes binding (no torch C++
ABI coupling — tensors are passed as raw device pointers, torch's caching
allocator owns all memory).

On a GPU box the native path is mandatory: ops raise
NativeExtensionMissing instead of silently falling back to eager torch.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

from lzy_amd.exceptions import NativeExtensionMissing

_LIB_PATH = os.path.join(os.path.dirname(__file__), "libhipops.so")

_lib: Optional[ctypes.CDLL] = None
_load_error: Optional[str] = None
_MX8 = False  # libhipops.so exports lz_mx8_pack / lz_mx8_unpack
_MX8_AXPBY = False  # ... and lz_mx8_axpby (the fused decode-combine)
_SEGCOPY = False  # ... and lz_segcopy (the packed-bundle gather/scatter)
# bytes per tile of the segmented copy — LZ_SEG_TILE in hipops.hip
SEGCOPY_TILE = 16384
_SEGCODEC = False  # ... and lz_segcodec (segmented copy-or-MXFP8-codec)
# elements per tile of a coded segment — LZ_SEGCODEC_ELEMS in hipops.hip
SEGCODEC_TILE_ELEMS = 8192
# segment modes of lz_segcodec — LZ_SC_* in hipops.hip; a coded mode is the
# base plus the leaf's dtype code (f32 0, f16 1, bf16 2)
SEGCODEC_RAW = 0
SEGCODEC_ENCODE = 1
SEGCODEC_DECODE = 4


def _try_load() -> Optional[ctypes.CDLL]:
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        _load_error = f"{_LIB_PATH} not built"
        return None
    try:
        # Bind to torch's HIP runtime, not the system one: torch bundles
        # its own libamdhip64.so.7 and two coexisting runtimes make our
        # launches fail with hipErrorNoDevice.  Loading torch (and its
        # runtime, RTLD_GLOBAL) first makes our DT_NEEDED resolve to the
        # same runtime torch uses.
        import torch  # noqa: F401

        torch_hip = os.path.join(
            os.path.dirname(torch.__file__), "lib", "libamdhip64.so"
        )
        if os.path.exists(torch_hip):
            ctypes.CDLL(torch_hip, mode=ctypes.RTLD_GLOBAL)
        lib = ctypes.CDLL(_LIB_PATH)
    except OSError as e:  # e.g. no ROCm runtime on a CPU-only box
        _load_error = str(e)
        return None
    lib.lz_cast_copy.restype = ctypes.c_int
    lib.lz_cast_copy.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int64, ctypes.c_void_p,
    ]
    lib.lz_checksum.restype = ctypes.c_int
    lib.lz_checksum.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.lz_checksum_mfma.restype = ctypes.c_int
    lib.lz_checksum_mfma.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.lz_fill_pattern.restype = ctypes.c_int
    lib.lz_fill_pattern.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p,
    ]
    lib.lz_fill_pattern_masked.restype = ctypes.c_int
    lib.lz_fill_pattern_masked.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64,
        ctypes.c_void_p,
    ]
    lib.lz_stats.restype = ctypes.c_int
    lib.lz_stats.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.lz_stats_variant.restype = ctypes.c_int
    lib.lz_stats_variant.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
    ]
    lib.lz_normalize_apply.restype = ctypes.c_int
    lib.lz_normalize_apply.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
    ]
    lib.lz_scale_shift.restype = ctypes.c_int
    lib.lz_scale_shift.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
    ]
    lib.lz_transpose_cast.restype = ctypes.c_int
    lib.lz_transpose_cast.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
    ]
    lib.lz_axpby.restype = ctypes.c_int
    lib.lz_axpby.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
        ctypes.c_void_p,
    ]
    # newer exports bind optionally: a stale libhipops.so without them must
    # not take the ops above down with it (mx8_* then raise
    # NativeExtensionMissing on use)
    global _MX8
    try:
        lib.lz_mx8_pack.restype = ctypes.c_int
        lib.lz_mx8_pack.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
            ctypes.c_void_p,
        ]
        lib.lz_mx8_unpack.restype = ctypes.c_int
        lib.lz_mx8_unpack.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
            ctypes.c_void_p,
        ]
        _MX8 = True
    except AttributeError:
        _MX8 = False
    global _MX8_AXPBY
    try:
        lib.lz_mx8_axpby.restype = ctypes.c_int
        lib.lz_mx8_axpby.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
            ctypes.c_void_p,
        ]
        _MX8_AXPBY = True
    except AttributeError:
        _MX8_AXPBY = False
    global _SEGCOPY
    try:
        lib.lz_segcopy.restype = ctypes.c_int
        lib.lz_segcopy.argtypes = [
            ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
            ctypes.c_void_p,
        ]
        lib.lz_segcopy_tile.restype = ctypes.c_int
        lib.lz_segcopy_tile.argtypes = []
        # the host builds tile_start for SEGCOPY_TILE: a library compiled
        # for another tile size is as unusable as one without the export
        _SEGCOPY = lib.lz_segcopy_tile() == SEGCOPY_TILE
    except AttributeError:
        _SEGCOPY = False
    global _SEGCODEC
    try:
        lib.lz_segcodec.restype = ctypes.c_int
        lib.lz_segcodec.argtypes = [
            ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
            ctypes.c_void_p,
        ]
        lib.lz_segcodec_tile_elems.restype = ctypes.c_int
        lib.lz_segcodec_tile_elems.argtypes = []
        # raw segments use the segcopy tile, coded ones SEGCODEC_TILE_ELEMS
        _SEGCODEC = _SEGCOPY and \
            lib.lz_segcodec_tile_elems() == SEGCODEC_TILE_ELEMS
    except AttributeError:
        _SEGCODEC = False
    lib.lz_error_name.restype = ctypes.c_char_p
    lib.lz_error_name.argtypes = [ctypes.c_int]
    lib.lz_set_max_blocks.restype = None
    lib.lz_set_max_blocks.argtypes = [ctypes.c_int]
    cap = os.environ.get("LZY_HIP_MAX_BLOCKS")
    if cap:
        lib.lz_set_max_blocks(int(cap))
    _lib = lib
    return lib


NATIVE = _try_load() is not None


def _require_native() -> ctypes.CDLL:
    lib = _try_load()
    if lib is None:
        raise NativeExtensionMissing(
            f"lzy_amd HIP ops not available ({_load_error}); build with "
            f"`python setup.py build_ext --inplace` / __graft_entry__.build() "
            f"(hipcc --offload-arch=gfx950)"
        )
    return lib


def _check(err: int) -> None:
    if err != 0:
        lib = _require_native()
        name = lib.lz_error_name(err).decode()
        raise RuntimeError(f"hipops kernel failed: {name} ({err})")


# dtype codes — must match LzDtype in hipops.hip
def _dtype_code(dtype) -> int:
    import torch

    codes = {
        torch.float32: 0,
        torch.float16: 1,
        torch.bfloat16: 2,
        torch.float8_e4m3fn: 3,
        torch.float8_e5m2: 4,
        torch.uint8: 5,
        torch.int32: 6,
        torch.int64: 7,
        torch.float64: 8,
    }
    if dtype not in codes:
        raise ValueError(f"unsupported dtype for hipops: {dtype}")
    return codes[dtype]


def _current_stream_ptr() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream


def _check_dst(op: str, dst, numel: int, shape=None) -> None:
    """The kernels write ``numel`` elements linearly from ``dst.data_ptr()``:
    anything but a contiguous device tensor of exactly that size would be
    written out of order or out of bounds, so it is rejected up front."""
    if not dst.is_cuda:
        raise ValueError(f"{op}: dst must be a device tensor")
    if not dst.is_contiguous():
        raise ValueError(f"{op}: dst must be contiguous")
    if dst.numel() != numel:
        raise ValueError(
            f"{op}: dst has {dst.numel()} elements, expected {numel}"
        )
    if shape is not None and tuple(dst.shape) != tuple(shape):
        raise ValueError(
            f"{op}: dst has shape {tuple(dst.shape)}, expected {tuple(shape)}"
        )


def cast_copy(src, dst) -> None:
    """dst[i] = cast(src[i]); dst device-contiguous, same numel.

    Fused pack+dtype-cast on the current stream — the channel transport's
    cast-on-the-wire primitive.  Numeric contract: docs/api.md.
    """
    lib = _require_native()
    if src.numel() != dst.numel():
        raise ValueError("cast_copy: numel mismatch")
    if not (src.is_cuda and dst.is_cuda):
        raise ValueError("cast_copy: device tensors required")
    _check_dst("cast_copy", dst, src.numel())
    s = src.detach().contiguous()
    _check(
        lib.lz_cast_copy(
            ctypes.c_void_p(s.data_ptr()),
            _dtype_code(s.dtype),
            ctypes.c_void_p(dst.data_ptr()),
            _dtype_code(dst.dtype),
            s.numel(),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )


def _require_mx8() -> ctypes.CDLL:
    lib = _require_native()
    if not _MX8:
        raise NativeExtensionMissing(
            f"{_LIB_PATH} is stale: it lacks lz_mx8_pack/lz_mx8_unpack; "
            f"rebuild with `python setup.py build_ext --inplace --force`"
        )
    return lib


def mx8_nbytes(numel: int) -> int:
    """Wire bytes of ``numel`` elements in the block-scaled FP8 format:
    32 e4m3 payload bytes + 1 scale byte per 32-element block."""
    return 33 * ((int(numel) + 31) // 32)


def _mx8_check_dtype(dtype, what: str) -> None:
    import torch

    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"{what}: dtype must be f32/bf16/f16, got {dtype}")


def mx8_pack(t, out=None):
    """Pack a device f32/bf16/f16 tensor into the block-scaled FP8 (MXFP8)
    wire format (docs/mxwire.md): one fused amax-reduce + scale + e4m3
    quantize pass on the current stream.  Returns a flat uint8 tensor of
    ``mx8_nbytes(t.numel())`` bytes (``out`` when given)."""
    import torch

    if not t.is_cuda:
        raise ValueError("mx8_pack requires a device tensor")
    _mx8_check_dtype(t.dtype, "mx8_pack")
    lib = _require_mx8()
    s = t.detach().contiguous()
    n = s.numel()
    nbytes = mx8_nbytes(n)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
              and out.numel() == nbytes):
        raise ValueError(
            f"mx8_pack: out must be a contiguous device uint8[{nbytes}]"
        )
    _check(
        lib.lz_mx8_pack(
            ctypes.c_void_p(s.data_ptr()),
            _dtype_code(s.dtype),
            ctypes.c_void_p(out.data_ptr()),
            n,
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return out


def mx8_unpack(buf, numel_or_shape, dtype, out=None):
    """Decode an MXFP8 wire buffer (device uint8) into a tensor of
    ``dtype`` (f32/bf16/f16) and the given numel or shape."""
    import torch

    if isinstance(numel_or_shape, int):
        shape = (numel_or_shape,)
    else:
        shape = tuple(int(d) for d in numel_or_shape)
    n = 1
    for d in shape:
        n *= d
    if not buf.is_cuda:
        raise ValueError("mx8_unpack requires a device buffer")
    _mx8_check_dtype(dtype, "mx8_unpack")
    if buf.dtype != torch.uint8 or not buf.is_contiguous() \
            or buf.numel() != mx8_nbytes(n):
        raise ValueError(
            f"mx8_unpack: buffer must be contiguous uint8[{mx8_nbytes(n)}] "
            f"for {n} elements, got {buf.dtype}[{buf.numel()}]"
        )
    lib = _require_mx8()
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=buf.device)
    elif not (out.is_cuda and out.dtype == dtype and out.is_contiguous()
              and out.numel() == n):
        raise ValueError(
            f"mx8_unpack: out must be a contiguous device {dtype}[{n}]"
        )
    _check(
        lib.lz_mx8_unpack(
            ctypes.c_void_p(buf.data_ptr()),
            ctypes.c_void_p(out.data_ptr()),
            _dtype_code(dtype),
            n,
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return out


def mx8_axpby(a, wire, alpha: float = 1.0, beta: float = 1.0, dst=None):
    """dst = alpha*a + beta*decode(wire): the combine of a wire-cast
    merge-tree edge with the MXFP8 decode fused in (docs/mxwire.md).

    ``a`` is a device f32/bf16/f16 tensor, ``wire`` the contiguous device
    ``uint8[mx8_nbytes(a.numel())]`` buffer of as many elements.  The
    decoded operand enters the fp32 FMA unrounded (it is never cast to a
    16-bit type first).  ``dst`` defaults to a new tensor like ``a``; it
    may be ``a`` itself (in place) and may have another of the three
    dtypes.  Returns ``dst``."""
    import torch

    if not (a.is_cuda and wire.is_cuda):
        raise ValueError("mx8_axpby requires device tensors")
    _mx8_check_dtype(a.dtype, "mx8_axpby")
    n = a.numel()
    if wire.dtype != torch.uint8 or not wire.is_contiguous() \
            or wire.numel() != mx8_nbytes(n):
        raise ValueError(
            f"mx8_axpby: wire must be contiguous uint8[{mx8_nbytes(n)}] "
            f"for {n} elements, got {wire.dtype}[{wire.numel()}]"
        )
    if dst is not None:
        _check_dst("mx8_axpby", dst, n)
        _mx8_check_dtype(dst.dtype, "mx8_axpby dst")
    lib = _require_native()
    if not _MX8_AXPBY:
        raise NativeExtensionMissing(
            f"{_LIB_PATH} is stale: it lacks lz_mx8_axpby; "
            f"rebuild with `python setup.py build_ext --inplace --force`"
        )
    x = a.detach().contiguous()
    if dst is None:
        dst = torch.empty_like(x)
    _check(
        lib.lz_mx8_axpby(
            ctypes.c_void_p(x.data_ptr()),
            _dtype_code(x.dtype),
            ctypes.c_void_p(wire.data_ptr()),
            ctypes.c_void_p(dst.data_ptr()),
            _dtype_code(dst.dtype),
            n,
            ctypes.c_float(alpha),
            ctypes.c_float(beta),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return dst


# ---------------------------------------------------------------------------
# segmented copy: pack / unpack a list of tensors into one uint8 buffer
# (the wire form of a tensor bundle — channels/bundle.py, docs/bundles.md)
# ---------------------------------------------------------------------------

def _require_segcopy() -> ctypes.CDLL:
    lib = _require_native()
    if not _SEGCOPY:
        raise NativeExtensionMissing(
            f"{_LIB_PATH} is stale: it lacks lz_segcopy (tile {SEGCOPY_TILE}); "
            f"rebuild with `python setup.py build_ext --inplace --force`"
        )
    return lib


def _check_align(align: int) -> int:
    align = int(align)
    if align < 1 or align & (align - 1):
        raise ValueError(f"align must be a positive power of two, got {align}")
    return align


def segcopy_layout(sizes, align: int = 128):
    """Byte offsets of segments of ``sizes`` bytes laid out in order, each
    starting at a multiple of ``align``; returns ``(offsets, total)`` with
    ``total`` the end of the last segment rounded up to ``align``.  Pure
    host arithmetic."""
    align = _check_align(align)
    offsets = []
    end = 0
    for n in sizes:
        n = int(n)
        if n < 0:
            raise ValueError(f"negative segment size {n}")
        off = (end + align - 1) // align * align
        offsets.append(off)
        end = off + n
    return offsets, (end + align - 1) // align * align


def segcopy_nbytes(sizes, align: int = 128) -> int:
    """Length of the packed buffer for segments of ``sizes`` bytes."""
    return segcopy_layout(sizes, align)[1]


def segcopy_table(src_addrs, dst_addrs, sizes, tile: int = SEGCOPY_TILE):
    """The kernel's table for ``len(sizes)`` segments, as a flat list of
    ints — ``src_addr[n] + dst_addr[n] + nbytes[n] + tile_start[n + 1]`` —
    and the tile count.  ``tile_start`` is the prefix sum of
    ``ceil(nbytes / tile)``: a zero-length segment owns no tile.  Pure host
    code (no device needed)."""
    sizes = [int(n) for n in sizes]
    if not (len(src_addrs) == len(dst_addrs) == len(sizes)):
        raise ValueError("segcopy_table: length mismatch")
    tile_start = [0]
    for n in sizes:
        if n < 0:
            raise ValueError(f"negative segment size {n}")
        tile_start.append(tile_start[-1] + (n + tile - 1) // tile)
    table = [int(a) for a in src_addrs] + [int(a) for a in dst_addrs] \
        + sizes + tile_start
    return table, tile_start[-1]


def _nbytes_of(t) -> int:
    return t.numel() * t.element_size()


def _byte_view(t):
    """Flat uint8 view of a contiguous tensor (0-dim and empty included)."""
    import torch

    return t.reshape(-1).view(torch.uint8)


def pack_tensors_torch(tensors, out=None, align: int = 128):
    """Torch-only twin of :func:`pack_tensors`, byte-identical to the
    kernel's output: the codec of CPU bundles and the kernel's test oracle
    (the role ``mx8_pack_torch`` has for the MXFP8 kernels)."""
    import torch

    tensors = list(tensors)
    offsets, total = segcopy_layout([_nbytes_of(t) for t in tensors], align)
    if out is None:
        device = tensors[0].device if tensors else None
        out = torch.zeros(total, dtype=torch.uint8, device=device)
    else:
        if out.dtype != torch.uint8 or not out.is_contiguous() \
                or out.numel() != total:
            raise ValueError(
                f"pack_tensors_torch: out must be a contiguous uint8[{total}]"
            )
        out.zero_()
    for t, off in zip(tensors, offsets):
        n = _nbytes_of(t)
        if n:
            out[off: off + n].copy_(_byte_view(t.detach().contiguous()))
    return out, offsets


def _segcopy_upload(table, device):
    """The table in device memory, uploaded on ``device``'s current stream.
    Pinned staging + async H2D: torch's pinned allocator keeps the host
    block until the copy has run, its device allocator keeps the table
    until the kernels launched on the same stream afterwards have."""
    import torch

    host = torch.empty(len(table), dtype=torch.int64, pin_memory=True)
    host.copy_(torch.tensor(table, dtype=torch.int64))
    with torch.cuda.device(device):
        return host.to(device, non_blocking=True)


def _segcopy_run(lib, dev_table, nseg: int, ntiles: int, zero_pad_align: int,
                 device) -> None:
    import torch

    with torch.cuda.device(device):
        _check(
            lib.lz_segcopy(
                ctypes.c_void_p(dev_table.data_ptr()),
                nseg,
                ntiles,
                int(zero_pad_align),
                ctypes.c_void_p(_current_stream_ptr()),
            )
        )


def _segcopy_launch(lib, src_addrs, dst_addrs, sizes, zero_pad_align: int,
                    device) -> None:
    table, ntiles = segcopy_table(src_addrs, dst_addrs, sizes)
    if ntiles == 0:
        return
    dev_table = _segcopy_upload(table, device)
    _segcopy_run(lib, dev_table, len(sizes), ntiles, zero_pad_align, device)


def pack_tensors(tensors, out=None, align: int = 128):
    """Pack device tensors into one contiguous device ``uint8`` buffer with
    a single segmented-copy launch on the current stream.

    Leaves are laid out in order, each at a multiple of ``align`` (128 B: an
    L2 line, and enough for any dtype's view and for 16 B vector access);
    the buffer is ``segcopy_nbytes(sizes, align)`` long and every byte of it
    is defined — leaf data or zero.  Non-contiguous leaves go through
    ``.contiguous()`` first.  Returns ``(buf, offsets)``; ``out`` (device
    ``uint8`` of exactly that length, ``align``-aligned) is filled in place
    when given."""
    import torch

    # (a state_dict has hundreds of leaves: the host work per leaf is kept
    # to the few attribute reads below)
    tensors = [t.detach() if t.requires_grad else t for t in tensors]
    align = _check_align(align)
    if not tensors:
        raise ValueError("pack_tensors: no tensors")
    device = tensors[0].device
    sizes = []
    for t in tensors:
        if not t.is_cuda:
            raise ValueError("pack_tensors requires device tensors")
        if t.device != device:
            raise ValueError(
                f"pack_tensors: leaves on different devices "
                f"({device}, {t.device})"
            )
        sizes.append(t.numel() * t.element_size())
    offsets, total = segcopy_layout(sizes, align)
    if out is not None:
        if not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1
                and out.is_contiguous()):
            raise ValueError("pack_tensors: out must be a contiguous device uint8")
        if out.numel() != total:
            raise ValueError(
                f"pack_tensors: out has {out.numel()} bytes, expected {total}"
            )
        if out.device != device:
            raise ValueError("pack_tensors: out is on another device")
        if out.data_ptr() % align:
            raise ValueError(f"pack_tensors: out must be {align} B-aligned")
    lib = _require_segcopy()
    if out is None:
        # the pad is zeroed by address, so the base must be align-aligned;
        # the allocator's own alignment covers the default
        raw = torch.empty(total + align, dtype=torch.uint8, device=device)
        skew = -raw.data_ptr() % align
        out = raw[skew: skew + total]
    srcs = [t if t.is_contiguous() else t.contiguous() for t in tensors]
    base = out.data_ptr()
    _segcopy_launch(
        lib, [s.data_ptr() for s in srcs], [base + o for o in offsets],
        sizes, align, device,
    )
    return out, offsets


def _numel_of(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def unpack_tensors(buf, offsets, shapes, dtypes, out=None):
    """Leaves of a packed buffer.  With ``out=None`` they are VIEWS into
    ``buf`` (no kernel, no copy; CPU or device).  With ``out`` a list of
    contiguous device tensors of the leaves' shapes and dtypes the bytes
    are scattered into them by the segmented-copy kernel (the
    ``load_state_dict``-style "copy into my parameters" case) and ``out``
    is returned."""
    import torch

    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError("unpack_tensors: buf must be a contiguous 1-D uint8")
    if not (len(offsets) == len(shapes) == len(dtypes)):
        raise ValueError("unpack_tensors: offsets/shapes/dtypes differ in length")
    shapes = [tuple(int(d) for d in s) for s in shapes]
    sizes = [
        _numel_of(s) * torch.empty(0, dtype=dt).element_size()
        for s, dt in zip(shapes, dtypes)
    ]
    for off, n in zip(offsets, sizes):
        if off < 0 or off + n > buf.numel():
            raise ValueError(
                f"unpack_tensors: segment [{off}, {off + n}) outside the "
                f"{buf.numel()}-byte buffer"
            )
    if out is None:
        return [
            buf[off: off + n].view(dt).view(s)
            for off, n, s, dt in zip(offsets, sizes, shapes, dtypes)
        ]
    out = list(out)
    if not buf.is_cuda:
        raise ValueError("unpack_tensors: scatter requires a device buffer")
    if len(out) != len(offsets):
        raise ValueError("unpack_tensors: out has the wrong number of tensors")
    for o, s, dt in zip(out, shapes, dtypes):
        if not o.is_cuda or o.device != buf.device:
            raise ValueError("unpack_tensors: out tensors must be on buf's device")
        if not o.is_contiguous():
            raise ValueError("unpack_tensors: out tensors must be contiguous")
        if o.dtype != dt or tuple(o.shape) != s:
            raise ValueError(
                f"unpack_tensors: out tensor is {o.dtype}{tuple(o.shape)}, "
                f"expected {dt}{s}"
            )
    lib = _require_segcopy()
    base = buf.data_ptr()
    _segcopy_launch(
        lib, [base + o for o in offsets], [o.data_ptr() for o in out],
        sizes, 0, buf.device,
    )
    return out


# ---------------------------------------------------------------------------
# segmented copy-or-codec: a packed buffer whose flagged ("wired") float
# leaves are MXFP8 segments (docs/mxwire.md layout) and whose other leaves
# are raw bytes — the wire form of a bundle under ``bundle_wire_cast``
# ---------------------------------------------------------------------------

def _require_segcodec() -> ctypes.CDLL:
    lib = _require_native()
    if not _SEGCODEC:
        raise NativeExtensionMissing(
            f"{_LIB_PATH} is stale: it lacks lz_segcodec (tile "
            f"{SEGCODEC_TILE_ELEMS} elements); "
            f"rebuild with `python setup.py build_ext --inplace --force`"
        )
    return lib


def segcodec_table(src_addrs, dst_addrs, counts, modes,
                   tile: int = SEGCOPY_TILE,
                   tile_elems: int = SEGCODEC_TILE_ELEMS):
    """The table of ``lz_segcodec`` as a flat list of ints —
    ``src_addr[n] + dst_addr[n] + count[n] + mode[n] + tile_start[n + 1]`` —
    and the tile count.  ``count`` is bytes for a ``SEGCODEC_RAW`` segment
    (tiles of ``tile`` bytes) and elements for a coded one (tiles of
    ``tile_elems`` elements); a zero-count segment owns no tile.  Pure host
    code (no device needed)."""
    counts = [int(n) for n in counts]
    modes = [int(m) for m in modes]
    if not (len(src_addrs) == len(dst_addrs) == len(counts) == len(modes)):
        raise ValueError("segcodec_table: length mismatch")
    tile_start = [0]
    for n, m in zip(counts, modes):
        if n < 0:
            raise ValueError(f"negative segment count {n}")
        if not SEGCODEC_RAW <= m < SEGCODEC_DECODE + 3:
            raise ValueError(f"unknown segment mode {m}")
        per = tile if m == SEGCODEC_RAW else tile_elems
        tile_start.append(tile_start[-1] + (n + per - 1) // per)
    table = [int(a) for a in src_addrs] + [int(a) for a in dst_addrs] \
        + counts + modes + tile_start
    return table, tile_start[-1]


def _segcodec_launch(lib, src_addrs, dst_addrs, counts, modes,
                     zero_pad_align: int, device) -> None:
    import torch

    table, ntiles = segcodec_table(src_addrs, dst_addrs, counts, modes)
    if ntiles == 0:
        return
    dev_table = _segcopy_upload(table, device)
    with torch.cuda.device(device):
        _check(
            lib.lz_segcodec(
                ctypes.c_void_p(dev_table.data_ptr()),
                len(counts),
                ntiles,
                int(zero_pad_align),
                ctypes.c_void_p(_current_stream_ptr()),
            )
        )


def _wire_sizes(numels, itemsizes, wired):
    return [
        mx8_nbytes(n) if w else n * isz
        for n, isz, w in zip(numels, itemsizes, wired)
    ]


def _check_wired(op: str, wired, dtypes) -> list:
    wired = [bool(w) for w in wired]
    if len(wired) != len(dtypes):
        raise ValueError(f"{op}: wired flags and leaves differ in length")
    for w, dt in zip(wired, dtypes):
        if w:
            _mx8_check_dtype(dt, f"{op}: a wired leaf")
    return wired


def _check_packed_out(op: str, out, total: int, align: int, device) -> None:
    import torch

    if not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1
            and out.is_contiguous()):
        raise ValueError(f"{op}: out must be a contiguous device uint8")
    if out.numel() != total:
        raise ValueError(f"{op}: out has {out.numel()} bytes, expected {total}")
    if out.device != device:
        raise ValueError(f"{op}: out is on another device")
    if out.data_ptr() % align:
        raise ValueError(f"{op}: out must be {align} B-aligned")


def _aligned_empty(total: int, align: int, device):
    import torch

    raw = torch.empty(total + align, dtype=torch.uint8, device=device)
    skew = -raw.data_ptr() % align
    return raw[skew: skew + total]


def pack_tensors_wire_torch(tensors, wired, out=None, align: int = 128):
    """Torch-only twin of :func:`pack_tensors_wire`: the codec of CPU
    bundles and the kernel's oracle.  A wired segment is
    ``mx8_pack_torch(leaf)``, every other byte as ``pack_tensors_torch``."""
    import torch

    from lzy_amd.channels.mxwire import mx8_pack_torch

    tensors = [t.detach() for t in tensors]
    wired = _check_wired("pack_tensors_wire_torch", wired,
                         [t.dtype for t in tensors])
    sizes = _wire_sizes([t.numel() for t in tensors],
                        [t.element_size() for t in tensors], wired)
    offsets, total = segcopy_layout(sizes, align)
    if out is None:
        device = tensors[0].device if tensors else None
        out = torch.zeros(total, dtype=torch.uint8, device=device)
    else:
        if out.dtype != torch.uint8 or not out.is_contiguous() \
                or out.numel() != total:
            raise ValueError(
                f"pack_tensors_wire_torch: out must be a contiguous uint8[{total}]"
            )
        out.zero_()
    for t, w, off, n in zip(tensors, wired, offsets, sizes):
        if n:
            seg = mx8_pack_torch(t) if w else _byte_view(t.contiguous())
            out[off: off + n].copy_(seg)
    return out, offsets


def unpack_tensors_wire_torch(wire_buf, wired, shapes, dtypes, out=None,
                              align: int = 128):
    """Torch-only twin of :func:`unpack_tensors_wire`: the exact-layout
    buffer (``pack_tensors_torch`` of the decoded leaves) and its offsets."""
    import torch

    from lzy_amd.channels.mxwire import mx8_unpack_torch

    shapes = [tuple(int(d) for d in s) for s in shapes]
    wired = _check_wired("unpack_tensors_wire_torch", wired, dtypes)
    numels = [_numel_of(s) for s in shapes]
    itemsizes = [torch.empty(0, dtype=dt).element_size() for dt in dtypes]
    wsizes = _wire_sizes(numels, itemsizes, wired)
    woffs, wtotal = segcopy_layout(wsizes, align)
    if wire_buf.dtype != torch.uint8 or wire_buf.dim() != 1 \
            or wire_buf.numel() != wtotal:
        raise ValueError(
            f"unpack_tensors_wire_torch: wire buffer must be uint8[{wtotal}]"
        )
    leaves = []
    for w, off, n, s, dt in zip(wired, woffs, wsizes, shapes, dtypes):
        seg = wire_buf[off: off + n]
        leaves.append(mx8_unpack_torch(seg, s, dt) if w
                      else seg.clone().view(dt).view(s))
    if not leaves:
        return torch.zeros(0, dtype=torch.uint8, device=wire_buf.device), []
    return pack_tensors_torch(leaves, out=out, align=align)


def pack_tensors_wire(tensors, wired, out=None, align: int = 128):
    """:func:`pack_tensors` with the leaves flagged in ``wired`` (f32 / bf16
    / f16 only) MXFP8-encoded on the way: ONE segmented copy-or-codec launch
    on the current stream.  A wired leaf occupies ``mx8_nbytes(numel)``
    bytes, exactly what :func:`mx8_pack` writes for it; the other leaves,
    the layout rule (``segcopy_layout`` of the wire sizes), the zeroed gaps
    and ``out`` are as for :func:`pack_tensors`.  Returns
    ``(buf, offsets)``."""
    import torch

    tensors = [t.detach() if t.requires_grad else t for t in tensors]
    align = _check_align(align)
    if not tensors:
        raise ValueError("pack_tensors_wire: no tensors")
    wired = _check_wired("pack_tensors_wire", wired,
                         [t.dtype for t in tensors])
    device = tensors[0].device
    for t in tensors:
        if not t.is_cuda:
            raise ValueError("pack_tensors_wire requires device tensors")
        if t.device != device:
            raise ValueError(
                f"pack_tensors_wire: leaves on different devices "
                f"({device}, {t.device})"
            )
    numels = [t.numel() for t in tensors]
    sizes = _wire_sizes(numels, [t.element_size() for t in tensors], wired)
    offsets, total = segcopy_layout(sizes, align)
    if out is not None:
        _check_packed_out("pack_tensors_wire", out, total, align, device)
    lib = _require_segcodec()
    if out is None:
        out = _aligned_empty(total, align, device)
    srcs = [t if t.is_contiguous() else t.contiguous() for t in tensors]
    base = out.data_ptr()
    _segcodec_launch(
        lib, [s.data_ptr() for s in srcs], [base + o for o in offsets],
        [n if w else sz for n, sz, w in zip(numels, sizes, wired)],
        [SEGCODEC_ENCODE + _dtype_code(t.dtype) if w else SEGCODEC_RAW
         for t, w in zip(tensors, wired)],
        align, device,
    )
    return out, offsets


def unpack_tensors_wire(wire_buf, wired, shapes, dtypes, out=None,
                        align: int = 128):
    """Decode a :func:`pack_tensors_wire` buffer into the EXACT packed
    layout (what :func:`pack_tensors` of the decoded leaves would give,
    every byte defined) with one launch; returns ``(buf, offsets)``, so the
    leaves are ``unpack_tensors(buf, offsets, shapes, dtypes)`` views of one
    allocation.  ``out``: as for :func:`pack_tensors`."""
    import torch

    align = _check_align(align)
    shapes = [tuple(int(d) for d in s) for s in shapes]
    wired = _check_wired("unpack_tensors_wire", wired, dtypes)
    if len(shapes) != len(wired):
        raise ValueError("unpack_tensors_wire: shapes/dtypes differ in length")
    if not shapes:
        raise ValueError("unpack_tensors_wire: no tensors")
    if not (wire_buf.is_cuda and wire_buf.dtype == torch.uint8
            and wire_buf.dim() == 1 and wire_buf.is_contiguous()):
        raise ValueError(
            "unpack_tensors_wire: wire buffer must be a contiguous device uint8"
        )
    numels = [_numel_of(s) for s in shapes]
    itemsizes = [torch.empty(0, dtype=dt).element_size() for dt in dtypes]
    wsizes = _wire_sizes(numels, itemsizes, wired)
    woffs, wtotal = segcopy_layout(wsizes, align)
    if wire_buf.numel() != wtotal:
        raise ValueError(
            f"unpack_tensors_wire: wire buffer has {wire_buf.numel()} bytes, "
            f"expected {wtotal}"
        )
    sizes = [n * isz for n, isz in zip(numels, itemsizes)]
    offsets, total = segcopy_layout(sizes, align)
    device = wire_buf.device
    if out is not None:
        _check_packed_out("unpack_tensors_wire", out, total, align, device)
    lib = _require_segcodec()
    if out is None:
        out = _aligned_empty(total, align, device)
    sbase, dbase = wire_buf.data_ptr(), out.data_ptr()
    _segcodec_launch(
        lib, [sbase + o for o in woffs], [dbase + o for o in offsets],
        [n if w else sz for n, sz, w in zip(numels, sizes, wired)],
        [SEGCODEC_DECODE + _dtype_code(dt) if w else SEGCODEC_RAW
         for dt, w in zip(dtypes, wired)],
        align, device,
    )
    return out, offsets


def device_checksum(t, method: str = "auto") -> int:
    """64-bit content hash of a device tensor, computed on-GPU (no PCIe
    round-trip for the data; 8 bytes come back).

    method: "mfma" routes the mixing through the i8 matrix cores (the
    default for buffers >= 64 KiB — VALU stays free, bandwidth-bound),
    "valu" is the splitmix64 kernel, "auto" picks by size.  The two
    digests are different hash functions (both stable across runs).
    """
    import torch

    lib = _require_native()
    if not t.is_cuda:
        raise ValueError("device_checksum requires a device tensor")
    flat = t.detach().contiguous().view(torch.uint8) if t.dtype != torch.uint8 \
        else t.detach().contiguous()
    nbytes = flat.numel() * flat.element_size()
    if method == "auto":
        method = "mfma" if nbytes >= (64 << 10) else "valu"
    fn = lib.lz_checksum_mfma if method == "mfma" else lib.lz_checksum
    out = torch.zeros(1, dtype=torch.int64, device=t.device)
    _check(
        fn(
            ctypes.c_void_p(flat.data_ptr()),
            nbytes,
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return int(out.item()) & 0xFFFFFFFFFFFFFFFF


def stats(t, use_abs: bool = False):
    """One-pass (sum, sumsq) — or (sum|x|, sumsq) — of a device tensor.
    Returns a device float64[2] tensor; no host sync."""
    import torch

    lib = _require_native()
    if not t.is_cuda:
        raise ValueError("stats requires a device tensor")
    flat = t.detach().contiguous()
    out = torch.empty(2, dtype=torch.float64, device=t.device)
    _check(
        lib.lz_stats(
            ctypes.c_void_p(flat.data_ptr()),
            _dtype_code(flat.dtype),
            flat.numel(),
            1 if use_abs else 0,
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return out


def stats_variant(t, variant: int, use_abs: bool = False):
    """Sweep-only: run a (V, U) load-shape variant of the stats kernel
    (benchmarks/kernel_sweep.py picks the default)."""
    import torch

    lib = _require_native()
    flat = t.detach().contiguous()
    out = torch.empty(2, dtype=torch.float64, device=t.device)
    _check(
        lib.lz_stats_variant(
            ctypes.c_void_p(flat.data_ptr()),
            _dtype_code(flat.dtype),
            flat.numel(),
            1 if use_abs else 0,
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(_current_stream_ptr()),
            int(variant),
        )
    )
    return out


def abs_mean(t) -> float:
    """Fused mean(|x|) — one read of the buffer, 8 bytes back to host.
    (torch chain `t.float().abs().mean()` moves ~9x the bytes.)"""
    s = stats(t, use_abs=True)
    return float(s[0].item()) / max(1, t.numel())


def mean_std(t, unbiased: bool = False):
    """(mean, std) from the one-pass stats kernel; two scalars back."""
    import math

    s = stats(t, use_abs=False)
    n = t.numel()
    vals = s.cpu()
    mean = float(vals[0]) / n
    var = float(vals[1]) / n - mean * mean
    if unbiased and n > 1:
        var *= n / (n - 1)
    return mean, math.sqrt(max(var, 0.0))


def normalize(src, dst=None, eps: float = 1e-6):
    """dst = (src - mean(src)) / (std(src) + ~eps), fused two-pass on
    device (stats kernel + apply kernel, stats handed over in HBM — no
    host round-trip).  dst defaults to a new tensor of src's dtype."""
    import torch

    lib = _require_native()
    if not src.is_cuda:
        raise ValueError("normalize requires a device tensor")
    s = src.detach().contiguous()
    if dst is None:
        dst = torch.empty_like(s)
    else:
        _check_dst("normalize", dst, s.numel())
    st = stats(s, use_abs=False)
    _check(
        lib.lz_normalize_apply(
            ctypes.c_void_p(s.data_ptr()),
            _dtype_code(s.dtype),
            ctypes.c_void_p(dst.data_ptr()),
            _dtype_code(dst.dtype),
            s.numel(),
            ctypes.c_void_p(st.data_ptr()),
            ctypes.c_float(eps),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return dst


def scale_shift(src, a: float, b: float, dst=None):
    """dst = src * a + b (fused single-FMA elementwise; in-place when
    dst is src)."""
    import torch

    lib = _require_native()
    if not src.is_cuda:
        raise ValueError("scale_shift requires a device tensor")
    s = src.detach().contiguous()
    if dst is None:
        dst = torch.empty_like(s)
    else:
        _check_dst("scale_shift", dst, s.numel())
    _check(
        lib.lz_scale_shift(
            ctypes.c_void_p(s.data_ptr()),
            _dtype_code(s.dtype),
            ctypes.c_void_p(dst.data_ptr()),
            _dtype_code(dst.dtype),
            s.numel(),
            ctypes.c_float(a),
            ctypes.c_float(b),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return dst


def axpby(a, b, alpha: float = 1.0, beta: float = 1.0, dst=None):
    """dst = alpha*a + beta*b, fused (the tree-merge primitive: one read
    of each input, one write, vs 4+ passes for the torch float() chain)."""
    import torch

    lib = _require_native()
    if not (a.is_cuda and b.is_cuda):
        raise ValueError("axpby requires device tensors")
    if a.numel() != b.numel() or a.dtype != b.dtype:
        raise ValueError("axpby: shape/dtype mismatch")
    x = a.detach().contiguous()
    y = b.detach().contiguous()
    if dst is None:
        dst = torch.empty_like(x)
    else:
        _check_dst("axpby", dst, x.numel())
    _check(
        lib.lz_axpby(
            ctypes.c_void_p(x.data_ptr()),
            ctypes.c_void_p(y.data_ptr()),
            _dtype_code(x.dtype),
            ctypes.c_void_p(dst.data_ptr()),
            _dtype_code(dst.dtype),
            x.numel(),
            ctypes.c_float(alpha),
            ctypes.c_float(beta),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return dst


def transpose_cast(src, dst=None, dtype=None):
    """dst = src.T (2-D), optionally casting — LDS-staged 64x64 tiles so
    both the gather and the scatter side stay coalesced (the pack path
    for transposed tensors; a naive strided copy runs at ~1/8 HBM rate)."""
    import torch

    lib = _require_native()
    if not src.is_cuda or src.dim() != 2:
        raise ValueError("transpose_cast requires a 2-D device tensor")
    s = src.detach().contiguous()
    rows, cols = s.shape
    out_dtype = dtype or s.dtype
    if dst is None:
        dst = torch.empty(cols, rows, dtype=out_dtype, device=s.device)
    else:
        _check_dst("transpose_cast", dst, rows * cols, shape=(cols, rows))
    _check(
        lib.lz_transpose_cast(
            ctypes.c_void_p(s.data_ptr()),
            _dtype_code(s.dtype),
            ctypes.c_void_p(dst.data_ptr()),
            _dtype_code(dst.dtype),
            rows,
            cols,
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
    return dst


def fill_pattern(t, seed: int = 0, mask16: int = 0) -> None:
    """Deterministic device-side fill (tests / synthetic data).

    ``mask16``: AND every 16-bit lane with this mask in the same pass —
    e.g. 0x3FFF makes a bf16 buffer finite positive synthetic data
    without a second read+write over HBM.

    Byte ``8*i + k`` is byte ``k`` of ``splitmix64(seed ^ i) & mask``,
    trailing ``nbytes % 8`` bytes included.  ``t`` is written in place, so
    it must be a contiguous device tensor."""
    lib = _require_native()
    if not t.is_cuda:
        raise ValueError("fill_pattern requires a device tensor")
    if not t.is_contiguous():
        raise ValueError("fill_pattern: tensor must be contiguous")
    flat = t.detach()
    nbytes = flat.numel() * flat.element_size()
    if mask16:
        _check(
            lib.lz_fill_pattern_masked(
                ctypes.c_void_p(flat.data_ptr()),
                nbytes,
                ctypes.c_uint64(seed),
                ctypes.c_uint64(mask16),
                ctypes.c_void_p(_current_stream_ptr()),
            )
        )
        return
    _check(
        lib.lz_fill_pattern(
            ctypes.c_void_p(flat.data_ptr()),
            nbytes,
            ctypes.c_uint64(seed),
            ctypes.c_void_p(_current_stream_ptr()),
        )
    )
