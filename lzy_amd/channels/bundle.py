"""Packed tensor bundles: containers of tensors as a first-class entry kind.

A *bundle* is a nest of ``dict`` / ``OrderedDict`` / ``list`` / ``tuple``
whose tensor leaves all live on one device — ``model.state_dict()``,
``(features, labels)``, a list of shards, a dict of gradients.  Instead of
being pickled (a D2H copy of every leaf at op completion, a host-only
transfer, leaves landing on the *sender's* device index) it travels as

  * one contiguous ``uint8`` buffer, packed by a single segmented-copy
    launch (``ops.pack_tensors``; a torch codec for CPU leaves),
  * a layout table ``[[offset, dtype, shape], ...]``, and
  * a pickled *skeleton*: the container with every tensor leaf replaced by
    an index placeholder (non-tensor leaves stay in it).

The receiver rebuilds the container with leaves that are views into the
receive buffer on its own device — no unpack pass.  Rules, layout and the
one difference from pickling (views sharing storage are packed by value):
docs/bundles.md.

With ``bundle_wire_cast="mxfp8"`` (the driver's decision, per transfer) the
large float leaves cross the link block-scaled FP8: ``pack_bundle(value,
wire)`` builds the wire buffer of ``bundle_wire_layout`` in one
copy-or-codec launch, ``unpack_bundle_wire`` decodes it in one launch into
the exact layout above and rebuilds the container from that.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, List, Optional, Tuple

import torch

BUNDLE_MIN_BYTES = 64 << 10
BUNDLE_ALIGN = 128

_CONTAINERS = (dict, OrderedDict, list, tuple)
# non-tensor leaves (and dict keys) a bundle may carry in its skeleton:
# plain immutable scalars only, so the spec needs no device work, stays
# small and cannot hide a tensor
_SCALARS = (type(None), bool, int, float, complex, str, bytes,
            torch.dtype, torch.device, torch.Size)


class _Leaf:
    """Skeleton placeholder for tensor leaf ``i`` (pickled by reference)."""

    __slots__ = ("i",)

    def __init__(self, i: int) -> None:
        self.i = i

    def __reduce__(self):
        return (_Leaf, (self.i,))


class _NotBundle(Exception):
    pass


def _leaf_ok(t: torch.Tensor) -> bool:
    return (
        type(t) is torch.Tensor
        and t.layout == torch.strided
        and not t.requires_grad
        and not t.is_meta
        and not t.is_sparse
        and not t.is_quantized
        and not t.is_nested
        and not t.is_conj()
        and not t.is_neg()
    )


def _analyze(value: Any) -> Optional[Tuple[Any, List[torch.Tensor]]]:
    """(skeleton object, tensor leaves in layout order) or None when the
    value is not a bundle.  Touches shapes, dtypes and devices only."""
    if type(value) not in _CONTAINERS:
        return None
    leaves: List[torch.Tensor] = []
    index = {}  # id(tensor) -> leaf index: one object, one segment
    seen = set()  # container ids: shared or cyclic containers stay pickled

    def walk(v):
        if isinstance(v, torch.Tensor):
            i = index.get(id(v))
            if i is None:
                if not _leaf_ok(v):
                    raise _NotBundle
                if leaves and v.device != leaves[0].device:
                    raise _NotBundle
                i = index[id(v)] = len(leaves)
                leaves.append(v)
            return _Leaf(i)
        tv = type(v)
        if tv in _SCALARS:
            return v
        if tv not in _CONTAINERS:
            raise _NotBundle
        if tv is tuple:  # immutable: sharing one is unobservable
            return tuple(walk(x) for x in v)
        if id(v) in seen:
            raise _NotBundle
        seen.add(id(v))
        if tv is list:
            return [walk(x) for x in v]
        if any(type(k) not in _SCALARS for k in v):
            raise _NotBundle
        out = tv((k, walk(x)) for k, x in v.items())
        attrs = getattr(v, "__dict__", None)
        if attrs:
            # an OrderedDict may carry attributes (state_dict()'s
            # ``_metadata``); they travel like one more nested dict
            out.__dict__.update(walk(dict(attrs)))
        return out

    try:
        skeleton = walk(value)
    except (_NotBundle, RecursionError):
        return None
    if not leaves or leaves[0].device.type not in ("cpu", "cuda"):
        return None
    total = sum(t.numel() * t.element_size() for t in leaves)
    if total < BUNDLE_MIN_BYTES:
        return None
    return skeleton, leaves


def is_bundle(value: Any) -> bool:
    """True when ``value`` travels as a packed bundle (docs/bundles.md):
    a dict / OrderedDict / list / tuple nest (exact types) with at least
    one tensor leaf, every tensor leaf a plain dense ``torch.Tensor``
    without ``requires_grad``, all on one device, ``BUNDLE_MIN_BYTES`` or
    more of tensor data, and only plain scalars as other leaves."""
    return _analyze(value) is not None


def bundle_device(value: Any) -> Optional[torch.device]:
    """Device of a bundle's leaves; None when ``value`` is not a bundle."""
    if type(value) not in _CONTAINERS:
        return None
    got = _analyze(value)
    return None if got is None else got[1][0].device


def _dtype_name(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def _spec_of(skeleton: Any, leaves: List[torch.Tensor]) -> dict:
    import cloudpickle

    from lzy_amd.ops import segcopy_layout

    offsets, nbytes = segcopy_layout(
        [t.numel() * t.element_size() for t in leaves], BUNDLE_ALIGN
    )
    return {
        "skeleton": cloudpickle.dumps(skeleton),
        "segs": [
            [off, _dtype_name(t.dtype), [int(d) for d in t.shape]]
            for off, t in zip(offsets, leaves)
        ],
        "nbytes": nbytes,
    }


def try_bundle_spec(value: Any) -> Optional[dict]:
    """``bundle_spec(value)``, or None when ``value`` is not a bundle."""
    got = _analyze(value)
    return None if got is None else _spec_of(*got)


def bundle_spec(value: Any) -> dict:
    """``{"skeleton": bytes, "segs": [[offset, dtype, shape], ...],
    "nbytes": int}`` — computed from shapes and dtypes alone (no device
    work, no packing).  The same tensor object appearing twice is one
    segment."""
    spec = try_bundle_spec(value)
    if spec is None:
        raise ValueError("value is not a tensor bundle")
    return spec


BUNDLE_WIRES = ("", "mxfp8")
_WIRE_DTYPE_NAMES = ("float32", "bfloat16", "float16")


def _check_wire(wire: str) -> str:
    if wire not in BUNDLE_WIRES:
        raise ValueError(
            f"bundle wire must be \"\" or \"mxfp8\", got {wire!r}"
        )
    return wire


def _wired_flags(dtype_names, numels, wire: str) -> List[bool]:
    """Leaf ``i`` is wired when its dtype is f32/bf16/f16 and it has at
    least ``transport._WIRE_MIN_ELEMS`` elements, the threshold of every
    other wire cast; biases, norms and every other dtype stay exact."""
    from lzy_amd.channels.transport import _WIRE_MIN_ELEMS

    if not _check_wire(wire):
        return [False] * len(numels)
    return [
        name in _WIRE_DTYPE_NAMES and n >= _WIRE_MIN_ELEMS
        for name, n in zip(dtype_names, numels)
    ]


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def bundle_wire_layout(spec: dict, wire: str) -> Optional[dict]:
    """Wire form of the bundle ``spec`` under the lossy wire ``wire``:
    ``{"wired": [bool, ...], "offsets": [int, ...], "wire_nbytes": int}``,
    or None when ``wire`` is ``""`` or no leaf is wired — the bundle then
    travels exact, byte for byte.  A wired leaf occupies
    ``mx8_nbytes(numel)`` bytes (payload, then scale bytes:
    docs/mxwire.md), an exact leaf its raw bytes; segments follow
    ``ops.segcopy_layout(sizes, BUNDLE_ALIGN)`` in leaf order.  Reads shapes
    and dtypes only."""
    from lzy_amd.ops import mx8_nbytes, segcopy_layout

    segs = spec["segs"]
    numels = [_numel(s[2]) for s in segs]
    wired = _wired_flags([s[1] for s in segs], numels, wire)
    if not any(wired):
        return None
    sizes = [
        mx8_nbytes(n) if w
        else n * torch.empty(0, dtype=getattr(torch, s[1])).element_size()
        for s, n, w in zip(segs, numels, wired)
    ]
    offsets, total = segcopy_layout(sizes, BUNDLE_ALIGN)
    return {"wired": wired, "offsets": offsets, "wire_nbytes": total}


def pack_bundle(value: Any, wire: str = "") -> torch.Tensor:
    """The bundle's packed ``uint8`` buffer, on the leaves' device: one
    segmented-copy launch for device leaves (a missing kernel is an error,
    never a silent torch fallback), the torch codec for CPU leaves.

    With ``wire="mxfp8"`` the result is the WIRE buffer of
    :func:`bundle_wire_layout` — large float leaves MXFP8-encoded, packed
    by one copy-or-codec launch (``ops.pack_tensors_wire``); when no leaf
    is wired it is the exact buffer."""
    got = _analyze(value)
    if got is None:
        raise ValueError("value is not a tensor bundle")
    leaves = got[1]
    from lzy_amd import ops

    wired = _wired_flags([_dtype_name(t.dtype) for t in leaves],
                         [t.numel() for t in leaves], wire)
    if any(wired):
        if leaves[0].is_cuda:
            return ops.pack_tensors_wire(leaves, wired, align=BUNDLE_ALIGN)[0]
        return ops.pack_tensors_wire_torch(leaves, wired, align=BUNDLE_ALIGN)[0]
    if leaves[0].is_cuda:
        return ops.pack_tensors(leaves, align=BUNDLE_ALIGN)[0]
    return ops.pack_tensors_torch(leaves, align=BUNDLE_ALIGN)[0]


def unpack_bundle_wire(wire_buf: torch.Tensor, spec: dict, wire: str) -> Any:
    """Rebuild the container from a ``pack_bundle(value, wire)`` buffer:
    one decode launch (the torch codec on the CPU) into a fresh buffer of
    ``spec["nbytes"]`` in the exact layout, every byte defined, then
    :func:`unpack_bundle` of that — leaves are views of one allocation on
    ``wire_buf``'s device, the wire buffer is dropped."""
    from lzy_amd import ops

    layout = bundle_wire_layout(spec, wire)
    if layout is None:
        return unpack_bundle(wire_buf, spec)
    if wire_buf.numel() != layout["wire_nbytes"]:
        raise ValueError(
            f"bundle wire buffer has {wire_buf.numel()} bytes, "
            f"layout says {layout['wire_nbytes']}"
        )
    segs = spec["segs"]
    shapes = [s[2] for s in segs]
    dtypes = [getattr(torch, s[1]) for s in segs]
    decode = ops.unpack_tensors_wire if wire_buf.is_cuda \
        else ops.unpack_tensors_wire_torch
    buf, offsets = decode(wire_buf, layout["wired"], shapes, dtypes,
                          align=BUNDLE_ALIGN)
    assert offsets == [s[0] for s in segs] and buf.numel() == spec["nbytes"]
    return unpack_bundle(buf, spec)


def unpack_bundle(buf: torch.Tensor, spec: dict) -> Any:
    """Rebuild the container around views of ``buf`` (on whatever device
    ``buf`` is): container types, key order and non-tensor leaves as
    sent."""
    import cloudpickle

    from lzy_amd import ops

    segs = spec["segs"]
    if buf.numel() != spec["nbytes"]:
        raise ValueError(
            f"bundle buffer has {buf.numel()} bytes, spec says {spec['nbytes']}"
        )
    leaves = ops.unpack_tensors(
        buf,
        [s[0] for s in segs],
        [s[2] for s in segs],
        [getattr(torch, s[1]) for s in segs],
    )

    def fill(v):
        tv = type(v)
        if tv is _Leaf:
            return leaves[v.i]
        if tv is list:
            return [fill(x) for x in v]
        if tv is tuple:
            return tuple(fill(x) for x in v)
        if tv is dict or tv is OrderedDict:
            out = tv((k, fill(x)) for k, x in v.items())
            attrs = getattr(v, "__dict__", None)
            if attrs:
                out.__dict__.update(fill(dict(attrs)))
            return out
        return v

    return fill(cloudpickle.loads(spec["skeleton"]))
