"""Value transport between GPU workers.

Re-design of the reference's slot/channel data path (reference: lzy/slots
InputSlot/OutputSlot gRPC chunk streams + S3 fail-over,
slots/InputSlot.java:118-190, transfers/SlotInputTransfer.java:55-63):
on one MI355X node a channel edge is

  * same-rank            -> no-op (the value is a store reference);
  * device tensor, cross -> RCCL point-to-point over xGMI
                            (torch.distributed isend/irecv on the data
                            process group; "nccl" IS RCCL on ROCm);
  * container of tensors -> one packed uint8 buffer over the same tensor
                            path, leaves rebuilt as views of it
                            (channels/bundle.py, docs/bundles.md);
  * anything else        -> cloudpickle bytes over gloo isend/irecv.

Ordering discipline: RCCL matches p2p by (src, dst) issue order, not tags,
so the driver assigns every transfer a global sequence number and each
rank issues its sends/recvs in that global order (its command queue is a
subsequence of the global order) — pairwise-consistent, cycle-free, no
p2p deadlock.  All transfer ops are NON-blocking (isend/irecv); executor
threads wait on the returned handles, the serve loop never blocks.
"""
from __future__ import annotations

import io
import logging
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

_LOG = logging.getLogger("lzy_amd.transport")

KIND_TENSOR = "tensor"
KIND_BYTES = "bytes"
KIND_BUNDLE = "bundle"  # container of tensors, packed (channels/bundle.py)


@dataclass
class EntryMeta:
    """Driver-side location + shape record of one entry value."""

    entry_id: str
    owners: set = field(default_factory=set)
    kind: str = KIND_BYTES
    shape: Tuple[int, ...] = ()
    dtype: str = ""
    device_type: str = "cpu"  # "cuda" -> lives in HBM on the owner
    nbytes: int = 0
    ipc_handle: Optional[bytes] = None  # driver-side cache; never on the wire
    bundle: Optional[dict] = None  # KIND_BUNDLE only: bundle.bundle_spec()

    def to_wire(self) -> dict:
        wire = {
            "entry_id": self.entry_id,
            "kind": self.kind,
            "shape": list(self.shape),
            "dtype": self.dtype,
            "device_type": self.device_type,
            "nbytes": self.nbytes,
        }
        if self.kind == KIND_BUNDLE:
            wire["bundle"] = self.bundle
        return wire

    @staticmethod
    def from_wire(d: dict) -> "EntryMeta":
        return EntryMeta(
            entry_id=d["entry_id"],
            kind=d["kind"],
            shape=tuple(d["shape"]),
            dtype=d["dtype"],
            device_type=d["device_type"],
            nbytes=d["nbytes"],
            bundle=d.get("bundle"),
        )


def bundles_enabled() -> bool:
    from lzy_amd.config import get_config

    return get_config().channel_bundles


def _bundle_meta(entry_id: str, value: Any) -> Optional[EntryMeta]:
    """Bundle meta of an eligible container (no pickling, no device
    work); None for everything else or with ``channel_bundles`` off."""
    from lzy_amd.channels import bundle as _bundle

    if type(value) not in _bundle._CONTAINERS or not bundles_enabled():
        return None
    got = _bundle._analyze(value)
    if got is None:
        return None
    spec = _bundle._spec_of(*got)
    return EntryMeta(
        entry_id=entry_id,
        kind=KIND_BUNDLE,
        device_type=got[1][0].device.type,
        nbytes=spec["nbytes"],
        bundle=spec,
    )


def describe_value(entry_id: str, value: Any) -> EntryMeta:
    if isinstance(value, torch.Tensor):
        return EntryMeta(
            entry_id=entry_id,
            kind=KIND_TENSOR,
            shape=tuple(value.shape),
            dtype=str(value.dtype).replace("torch.", ""),
            device_type=value.device.type,
            nbytes=value.numel() * value.element_size(),
        )
    bm = _bundle_meta(entry_id, value)
    if bm is not None:
        return bm
    data = pickle_value(value)
    return EntryMeta(entry_id=entry_id, kind=KIND_BYTES, nbytes=len(data))


def pickle_value(value: Any) -> bytes:
    import cloudpickle

    return cloudpickle.dumps(value)


def unpickle_value(data: bytes) -> Any:
    import cloudpickle

    return cloudpickle.loads(data)


# ---------------------------------------------------------------------------
# hipIpc zero-copy path (same node, cross process)
# ---------------------------------------------------------------------------
#
# torch's CUDA-IPC reduction shares the tensor's HBM allocation itself
# (hipIpcGetMemHandle under the hood; dmabuf mode with
# HSA_ENABLE_IPC_MODE_LEGACY=0): the consumer maps the producer's memory
# with NO copy at all when it reads on the same GPU, or issues exactly one
# xGMI DMA (`.to(device)`) when it lives on another GPU.  torch's
# ref-counter files keep the producer allocation alive until every
# consumer releases its view.  Selected with LZY_CHANNEL_TRANSPORT=ipc;
# RCCL p2p is the default.

def export_ipc(tensor: torch.Tensor) -> bytes:
    from torch.multiprocessing.reductions import reduce_tensor

    import cloudpickle

    func, args = reduce_tensor(tensor)
    return cloudpickle.dumps((func, args))


def import_ipc(data: bytes, device: Optional[torch.device]) -> torch.Tensor:
    import cloudpickle

    func, args = cloudpickle.loads(data)
    t = func(*args)
    if device is not None and t.device != device:
        t = t.to(device)  # one DMA over xGMI
    return t


def ipc_enabled() -> bool:
    from lzy_amd.config import get_config

    return get_config().channel_transport == "ipc"


# ---------------------------------------------------------------------------
# cast-on-the-wire (BASELINE north star: the slot serializer's pack/unpack
# + dtype-cast as a CDNA4 HIP kernel).  Opt-in (lossy): float tensors are
# cast to a narrower wire dtype by the producer's cast kernel, halving (or
# quartering) the bytes crossing xGMI, and cast back on the consumer.
# Both sides derive the decision from (meta.dtype, config) — deterministic.
# The plain fp8 casts are unscaled (small-magnitude tensors come back all
# zero); the 8-bit format for real tensors is block-scaled "mxfp8" below.
# ---------------------------------------------------------------------------

_WIRE_DTYPES = {
    "fp16": torch.float16,
    "bf16": torch.bfloat16,
    "fp8e4m3": torch.float8_e4m3fn,
    "fp8e5m2": torch.float8_e5m2,
}
_WIRE_CASTABLE = (torch.float32, torch.bfloat16, torch.float16)
_WIRE_MIN_ELEMS = 1 << 16
# wire dtypes the gloo path can carry: float8 isend/irecv raises on gloo,
# so fp8 wire-cast is RCCL-device-path only
_GLOO_WIRE_OK = (torch.float16, torch.bfloat16)


def wire_cast_dtype() -> Optional[torch.dtype]:
    from lzy_amd.config import get_config

    return _WIRE_DTYPES.get(get_config().channel_wire_cast)


def _should_wirecast(dtype: torch.dtype, numel: int, wire) -> bool:
    return (
        wire is not None
        and dtype in _WIRE_CASTABLE
        and dtype != wire
        and torch.empty(0, dtype=wire).element_size()
        < torch.empty(0, dtype=dtype).element_size()
        and numel >= _WIRE_MIN_ELEMS
    )


# "mxfp8" is not a torch dtype: block-scaled FP8 (channels/mxwire.py) packs
# into a flat uint8 buffer, which every path carries — RCCL device, the
# host-staged fallback and CPU tensors over gloo.
_MX_WIRE = "mxfp8"


def wire_cast_mx() -> bool:
    from lzy_amd.config import get_config

    return get_config().channel_wire_cast == _MX_WIRE


def _should_mxcast(dtype: torch.dtype, numel: int, enabled: bool) -> bool:
    return enabled and dtype in _WIRE_CASTABLE and numel >= _WIRE_MIN_ELEMS


def _pack_contiguous(t: torch.Tensor) -> torch.Tensor:
    """Contiguous pack for the wire.  Transposed 2-D device views go
    through the LDS-tiled transpose kernel (coalesced both sides);
    everything else falls back to torch's copy."""
    if (
        t.is_cuda
        and t.dim() == 2
        and t.stride(0) == 1
        and t.stride(1) == t.shape[0]
    ):
        from lzy_amd import ops as _ops

        if _ops.NATIVE and t.dtype in (
            torch.float32, torch.float16, torch.bfloat16
        ):
            return _ops.transpose_cast(t.t())
    return t.contiguous()


def wire_pack(t: torch.Tensor, wire: torch.dtype) -> torch.Tensor:
    """Producer-side pack: cast to the wire dtype (HIP cast kernel on
    device, torch cast on host)."""
    out = torch.empty(t.shape, dtype=wire, device=t.device)
    if t.is_cuda:
        from lzy_amd import ops

        if ops.NATIVE:
            ops.cast_copy(t, out)
            return out
    return out.copy_(t.to(wire))


def wire_unpack(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Consumer-side unpack: cast back to the declared dtype."""
    out = torch.empty(w.shape, dtype=dtype, device=w.device)
    if w.is_cuda:
        from lzy_amd import ops

        if ops.NATIVE:
            ops.cast_copy(w, out)
            return out
    return out.copy_(w.to(dtype))


class Transport:
    """Per-rank transfer engine over a dedicated data process group.

    ``cuda_p2p``: device tensors go directly over RCCL/xGMI.  When ranks
    outnumber physical GPUs (test harnesses; oversubscribed pools) RCCL
    cannot build a comm, so device tensors are staged through pinned host
    memory and gloo — every rank computes the same predicate, so sender
    and receiver always agree on the wire format.
    """

    def __init__(self, pg: Optional[dist.ProcessGroup], device: Optional[torch.device],
                 world: int = 1):
        self._pg = pg
        self._device = device
        self._cuda_p2p = (
            device is not None
            and torch.cuda.is_available()
            and torch.cuda.device_count() >= world
        )
        # config read once: chunk size is fixed for the transport's life
        # (get_config() re-fingerprints the env — too hot per transfer)
        from lzy_amd.config import get_config

        self._chunk_bytes = get_config().channel_chunk_mb << 20
        self._wire = wire_cast_dtype()
        self._mx = wire_cast_mx()

    def _wire_allowed(self, producer_cuda: bool) -> bool:
        """May the configured wire dtype be used for this transfer?  The
        RCCL device path carries anything; the gloo path (CPU values,
        host-staged device tensors) only fp16/bf16."""
        if self._wire is None:
            return False
        if producer_cuda and self._cuda_p2p:
            return True
        return self._wire in _GLOO_WIRE_OK

    # -- chunking ------------------------------------------------------------
    #
    # Large values go over the wire as a sequence of fixed-size chunks
    # (reference: slots' offset-resumable chunked `Read` streams,
    # slots-api.proto:33-46, SlotInputTransfer.java:43-99).  Benefits here:
    # the host-staged fallback never materializes more than one chunk's
    # staging buffer ahead of the link, and a retried transfer can resume
    # from the first incomplete chunk (`offset_chunks`) instead of
    # resending the whole tensor.  Chunks of one transfer are issued
    # back-to-back on the (src,dst) pair, so RCCL/gloo order-matching
    # pairs them 1:1 with the receiver's chunk recvs.

    def _chunk_elems(self, elem_size: int) -> int:
        return max(1, self._chunk_bytes // max(1, elem_size))

    @staticmethod
    def _chunks(flat: torch.Tensor, per: int, offset_chunks: int):
        n = flat.numel()
        starts = range(offset_chunks * per, n, per)
        return [flat[s: min(s + per, n)] for s in starts]

    # -- op builders ---------------------------------------------------------
    #
    # send_ops/recv_ops return (P2POp list, keepalive/finalize) WITHOUT
    # issuing — callers group ops from several transfers into ONE
    # dist.batch_isend_irecv (ncclGroupStart/End under RCCL), so
    # transfers to/from *distinct peers* progress in parallel across
    # their xGMI links instead of serializing on the comm stream.

    def send_ops(self, value: Any, prepickled: Optional[bytes], dst: int,
                 offset_chunks: int = 0, tag: int = 0,
                 kind: Optional[str] = None, wire: str = ""):
        """Build send P2POps; returns (ops, keepalive).

        ``kind``: the entry's ``EntryMeta.kind`` when the caller knows it —
        the receiver follows the meta, so a sender told the kind never
        re-derives it.  Without it a container is sent as a bundle exactly
        when ``describe_value`` would have said so (no stored pickle, an
        eligible value, ``channel_bundles`` on).

        ``offset_chunks`` resumes a partially completed transfer: the
        first ``offset_chunks`` chunks are assumed delivered and skipped.
        ``tag``: driver-assigned per-transfer tag.  gloo matches p2p by
        (pair, tag, order); unique tags mean the stale posted recvs of a
        FAILED transfer can never swallow a later transfer's chunks.
        NCCL/RCCL ignores tags — that path keeps the strict
        driver-sequenced issue-order discipline instead.

        ``wire``: lossy wire format of a BUNDLE transfer ("" or "mxfp8"),
        decided by the driver per transfer (``bundle_wire_cast``) and handed
        to both endpoints; this rank's own config is not consulted.
        """
        as_bundle = kind == KIND_BUNDLE or (
            kind is None
            and prepickled is None
            and not isinstance(value, torch.Tensor)
            and _bundle_meta("", value) is not None
        )
        if as_bundle:
            from lzy_amd.channels import bundle as _bundle

            # one segmented-copy launch (torch codec for CPU leaves); the
            # packed uint8 buffer then rides the tensor path below as it
            # is: channel_wire_cast never applies to bundles (uint8 is not
            # a castable dtype, and the receiver never casts this kind).
            # With ``wire`` (bundle_wire_cast, the driver's decision) the
            # same launch MXFP8-encodes the large float leaves, where the
            # leaves live: only wire bytes are staged through the host.
            # The wire buffer is deterministic, so a resumed transfer's
            # re-pack reproduces the chunks already delivered.
            value = _bundle.pack_bundle(value, wire=wire)
        if isinstance(value, torch.Tensor):
            t = value.detach()
            if not t.is_contiguous():
                t = _pack_contiguous(t)
            # wire-cast decision must be symmetric with recv_ops: both
            # sides derive it from (producer device, _cuda_p2p, config).
            # fp8 wire dtypes are RCCL-device-path only — gloo (CPU
            # tensors, host-staged fallback) cannot carry float8.
            # mxfp8 packs to flat uint8 BEFORE host staging (a host-staged
            # device tensor is packed by the kernel) and rides every path.
            if _should_mxcast(t.dtype, t.numel(), self._mx):
                from lzy_amd.channels import mxwire

                t = mxwire.mx8_pack(t)
            elif self._wire_allowed(t.is_cuda) and _should_wirecast(
                t.dtype, t.numel(), self._wire
            ):
                t = wire_pack(t, self._wire)  # cast kernel on device
            if t.is_cuda and not self._cuda_p2p:
                t = t.cpu()
            per = self._chunk_elems(t.element_size())
            if t.numel() <= per and offset_chunks == 0:
                chunks = [t]
            else:
                chunks = self._chunks(t.view(-1), per, offset_chunks)
            # tags are a GLOO matching feature; the NCCL/RCCL path is
            # matched by issue order and torch documents tags as
            # unsupported there — pass 0 so no backend can object
            eff = 0 if t.is_cuda else tag
            ops = [dist.P2POp(dist.isend, c, dst, group=self._pg, tag=eff)
                   for c in chunks]
            return ops, t
        data = prepickled if prepickled is not None else pickle_value(value)
        buf = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        per = self._chunk_elems(1)
        if buf.numel() <= per and offset_chunks == 0:
            chunks = [buf]
        else:
            chunks = self._chunks(buf, per, offset_chunks)
        ops = [dist.P2POp(dist.isend, c, dst, group=self._pg, tag=tag)
               for c in chunks]
        return ops, buf

    def recv_ops(self, meta: EntryMeta, src: int, offset_chunks: int = 0,
                 into: Optional[torch.Tensor] = None, tag: int = 0,
                 wire: str = ""):
        """Build recv P2POps; returns (ops, finalize) where finalize() ->
        the received value (call after the issued works complete).

        ``offset_chunks``/``into`` resume into an existing buffer that
        already holds the first ``offset_chunks`` chunks (for a wired
        bundle: of the WIRE buffer).  ``wire``: see :meth:`send_ops`."""
        if meta.kind == KIND_BUNDLE:
            # the sender's packed uint8 buffer over the tensor path (same
            # chunking, staging and tag rules, never cast); the leaves are
            # views of this one buffer on OUR device.  Follows meta.kind
            # alone — the local channel_bundles setting is not consulted.
            # With ``wire`` the buffer on the link is the wire form; one
            # decode launch on arrival turns it into the exact layout.
            from lzy_amd.channels import bundle as _bundle

            spec = meta.bundle
            layout = _bundle.bundle_wire_layout(spec, wire)
            want_cuda = meta.device_type == "cuda" and self._device is not None
            on_device = want_cuda and self._cuda_p2p
            buf = into if into is not None else torch.empty(
                spec["nbytes"] if layout is None else layout["wire_nbytes"],
                dtype=torch.uint8,
                device=self._device if on_device else None,
            )
            per = self._chunk_elems(1)
            if buf.numel() <= per and offset_chunks == 0:
                chunks = [buf]
            else:
                chunks = self._chunks(buf, per, offset_chunks)
            eff = 0 if buf.is_cuda else tag  # mirror of the sender rule
            ops = [dist.P2POp(dist.irecv, c, src, group=self._pg, tag=eff)
                   for c in chunks]

            def finalize_bundle():
                out = buf
                if want_cuda and not on_device:
                    out = out.to(self._device, non_blocking=False)
                if layout is not None:
                    return _bundle.unpack_bundle_wire(out, spec, wire)
                return _bundle.unpack_bundle(out, spec)

            return ops, finalize_bundle
        if meta.kind == KIND_TENSOR:
            dtype = getattr(torch, meta.dtype)
            wire_dtype = dtype
            numel = 1
            for s in meta.shape:
                numel *= s
            want_cuda = meta.device_type == "cuda" and self._device is not None
            on_device = want_cuda and self._cuda_p2p
            # mirror of the sender's decision (same predicate, same inputs)
            casted = self._wire_allowed(
                meta.device_type == "cuda"
            ) and _should_wirecast(dtype, numel, self._wire)
            if casted:
                wire_dtype = self._wire
            mx = _should_mxcast(dtype, numel, self._mx)
            dev = self._device if on_device else None
            if mx:
                from lzy_amd.channels import mxwire

                wire_dtype = torch.uint8
                wire_shape: Tuple[int, ...] = (mxwire.mx8_nbytes(numel),)
            else:
                wire_shape = meta.shape
            per = self._chunk_elems(
                torch.empty(0, dtype=wire_dtype).element_size()
            )
            buf = into if into is not None else torch.empty(
                wire_shape, dtype=wire_dtype, device=dev
            )
            if buf.numel() <= per and offset_chunks == 0:
                chunks = [buf]
            else:
                chunks = self._chunks(buf.view(-1), per, offset_chunks)
            eff = 0 if buf.is_cuda else tag  # mirror of the sender rule
            ops = [dist.P2POp(dist.irecv, c, src, group=self._pg, tag=eff)
                   for c in chunks]

            def finalize():
                out = buf
                if want_cuda and not on_device:
                    out = out.to(self._device, non_blocking=False)
                if mx:
                    out = mxwire.mx8_unpack(out, meta.shape, dtype)
                elif casted:
                    out = wire_unpack(out, dtype)
                return out

            return ops, finalize
        per = self._chunk_elems(1)
        buf = into if into is not None else torch.empty(meta.nbytes, dtype=torch.uint8)
        if buf.numel() <= per and offset_chunks == 0:
            chunks = [buf]
        else:
            chunks = self._chunks(buf, per, offset_chunks)
        ops = [dist.P2POp(dist.irecv, c, src, group=self._pg, tag=tag)
               for c in chunks]
        return ops, (lambda: unpickle_value(buf.numpy().tobytes()))

    @staticmethod
    def _batch(ops: list) -> list:
        """batch_isend_irecv normalized to ONE work PER OP.

        Critical NCCL/RCCL behavior: with a coalescing backend the call
        returns a SINGLE work for the whole group (cm.works from
        _coalescing_manager), not one per op.  Callers here slice works
        per entry/chunk (settle waits, resume offsets); naive slicing
        would leave later entries with EMPTY work lists — no stream wait
        before their buffers are read.  Replicating the group work per
        op keeps every wait correct (waiting the same work repeatedly is
        idempotent).  gloo returns per-op works and passes through."""
        works = dist.batch_isend_irecv(ops)
        if len(works) == len(ops):
            return works
        if len(works) == 1:
            return [works[0]] * len(ops)

        class _AllOf:  # unexpected shape: conservative wait-them-all
            def __init__(self, ws):
                self._ws = ws

            def wait(self, *a, **k):
                for w in self._ws:
                    w.wait(*a, **k)
                return True

            def is_completed(self):
                return all(w.is_completed() for w in self._ws)

        return [_AllOf(works)] * len(ops)

    @staticmethod
    def issue(ops: list) -> list:
        """Issue a group of P2POps; returns one work per op, in order.

        Device and host ops are batched SEPARATELY: on the composite
        backend (cuda:nccl + cpu:gloo) a mixed batch would coalesce two
        different backends in one group — splitting is always safe
        because matching happens per backend, and both endpoints derive
        the same split from the same item order."""
        if not ops:
            return []
        cuda_ops = [op for op in ops if op.tensor.is_cuda]
        cpu_ops = [op for op in ops if not op.tensor.is_cuda]
        if not cuda_ops or not cpu_ops:
            return Transport._batch(ops)
        works_by_id = {}
        for group in (cuda_ops, cpu_ops):
            for op, w in zip(group, Transport._batch(group)):
                works_by_id[id(op)] = w
        return [works_by_id[id(op)] for op in ops]

    # -- single-transfer conveniences ----------------------------------------

    def isend_value(self, value: Any, prepickled: Optional[bytes], dst: int,
                    offset_chunks: int = 0, tag: int = 0,
                    kind: Optional[str] = None, wire: str = ""):
        """Issue non-blocking send(s); returns (works, keepalive)."""
        ops, keep = self.send_ops(value, prepickled, dst, offset_chunks, tag,
                                  kind, wire)
        return self.issue(ops), keep

    def irecv_value(self, meta: EntryMeta, src: int, offset_chunks: int = 0,
                    into: Optional[torch.Tensor] = None, tag: int = 0,
                    wire: str = ""):
        """Issue non-blocking recv; returns (works, finalize)."""
        ops, fin = self.recv_ops(meta, src, offset_chunks, into, tag, wire)
        return self.issue(ops), fin

    @staticmethod
    def completed_chunks(works: list) -> int:
        """Number of leading completed chunk transfers — the resume offset
        for a retry (reference: slots Read offset resume)."""
        done = 0
        for w in works:
            if w is not None and w.is_completed():
                done += 1
            else:
                break
        return done
