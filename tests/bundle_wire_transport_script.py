"""A wired tensor bundle over the chunked, offset-resumable transport —
world_size 2 on gloo, modelled on tests/chunked_transport_script.py.  Run
under torch.distributed.run by tests/test_bundle_wire.py; prints
BUNDLE-WIRE-TRANSPORT-OK on rank 0.

At ``channel_chunk_mb=1`` the wire buffer (about 1.2 MiB of MXFP8 segments
plus 1 MiB of exact int64) spans three chunks.  The second transfer resumes
with ``offset_chunks=1`` into a buffer that holds the first chunk: the wire
buffer is deterministic, so the sender's re-pack reproduces it.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels import bundle
from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch
from lzy_amd.channels.transport import KIND_BUNDLE, Transport, describe_value
from lzy_amd.config import Config


def _value(scale: float):
    g = torch.Generator().manual_seed(5)
    return {
        "w": torch.randn(1000, 1100, generator=g) * scale,            # wired
        "h": torch.randn(65536 + 7, generator=g).to(torch.bfloat16),  # wired
        "ids": torch.arange(1 << 17, dtype=torch.int64),              # exact
        "b": torch.randn(200, generator=g),                           # exact
        "step": 9,
    }


def _check(got, value) -> None:
    assert list(got) == list(value) and got["step"] == 9
    for k in ("w", "h"):
        t = value[k]
        want = mx8_unpack_torch(mx8_pack_torch(t), t.shape, t.dtype)
        assert got[k].dtype == t.dtype and torch.equal(got[k], want), k
    assert torch.equal(got["ids"], value["ids"])
    assert torch.equal(got["b"], value["b"])


def main() -> None:
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    Config.reset(channel_chunk_mb=1)
    tr = Transport(None, None, world=dist.get_world_size())
    per = tr._chunk_elems(1)

    value = _value(1.0)
    meta = describe_value("e1", value)
    assert meta.kind == KIND_BUNDLE
    layout = bundle.bundle_wire_layout(meta.bundle, "mxfp8")
    nchunks = -(-layout["wire_nbytes"] // per)
    assert nchunks >= 3, nchunks
    assert layout["wire_nbytes"] < meta.nbytes

    # --- whole transfer --------------------------------------------------
    if rank == 0:
        works, keep = tr.isend_value(value, None, dst=1, kind=KIND_BUNDLE,
                                     wire="mxfp8")
        assert keep.numel() == layout["wire_nbytes"]  # wire bytes on the link
        assert len(works) == nchunks, len(works)
        for w in works:
            w.wait()
    else:
        works, fin = tr.irecv_value(meta, src=0, wire="mxfp8")
        assert len(works) == nchunks, len(works)
        for w in works:
            w.wait()
        _check(fin(), value)

    dist.barrier()

    # --- offset resume: chunk 0 of the WIRE buffer already delivered ----
    value2 = _value(3e-3)
    meta2 = describe_value("e2", value2)
    if rank == 0:
        works, keep = tr.isend_value(value2, None, dst=1, offset_chunks=1,
                                     kind=KIND_BUNDLE, wire="mxfp8")
        assert len(works) == nchunks - 1
        for w in works:
            w.wait()
    else:
        whole = bundle.pack_bundle(value2, wire="mxfp8")
        buf = torch.zeros_like(whole)
        buf[:per] = whole[:per]  # chunk 0 survived the failed attempt
        works, fin = tr.irecv_value(meta2, src=0, offset_chunks=1, into=buf,
                                    wire="mxfp8")
        assert len(works) == nchunks - 1
        for w in works:
            w.wait()
        assert torch.equal(buf, whole)
        _check(fin(), value2)

    dist.barrier()

    # --- wire="" is the exact path, byte for byte ------------------------
    if rank == 0:
        works, keep = tr.isend_value(value, None, dst=1, kind=KIND_BUNDLE)
        assert torch.equal(keep, bundle.pack_bundle(value))
        for w in works:
            w.wait()
    else:
        works, fin = tr.irecv_value(meta, src=0)
        for w in works:
            w.wait()
        got = fin()
        for k in ("w", "h", "ids", "b"):
            assert torch.equal(got[k], value[k]), k

    dist.barrier()
    if rank == 0:
        print("BUNDLE-WIRE-TRANSPORT-OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
