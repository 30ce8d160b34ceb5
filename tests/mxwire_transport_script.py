"""channel_wire_cast="mxfp8" through the transport — world_size 2 on gloo.

Run under torch.distributed.run by tests/test_mxwire.py (CPU tensors) and
tests/test_gpu_mxwire.py (MXWIRE_DEVICE=cuda: device tensors, host-staged
because both ranks share one GPU); prints MXWIRE-TRANSPORT-OK on rank 0.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels.mxwire import mx8_nbytes, mx8_pack_torch, mx8_unpack_torch
from lzy_amd.channels.transport import Transport, describe_value
from lzy_amd.config import Config
from mxwire_util import assert_within_bound


def _wait(works):
    for w in works:
        w.wait()


def cpu_scenario(rank: int) -> None:
    Config.reset(channel_chunk_mb=1, channel_wire_cast="mxfp8")
    tr = Transport(None, None, world=dist.get_world_size())
    n = (1 << 20) + 77
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, generator=g) * 1e-4  # same values on both ranks
    wire = mx8_pack_torch(x)
    want = mx8_unpack_torch(wire, x.shape, torch.float32)

    # --- f32 CPU tensor travels as uint8[mx8_nbytes], chunked ------------
    if rank == 0:
        works, keep = tr.isend_value(x, None, dst=1, tag=11)
        assert keep.dtype == torch.uint8, keep.dtype
        assert keep.numel() == mx8_nbytes(n), keep.numel()
        assert torch.equal(keep, wire)
        assert len(works) >= 2, len(works)
        _wait(works)
    else:
        meta = describe_value("m1", torch.empty(n, dtype=torch.float32))
        works, fin = tr.irecv_value(meta, src=0, tag=11)
        assert len(works) >= 2, len(works)
        _wait(works)
        got = fin()
        assert got.dtype == torch.float32 and got.shape == (n,)
        rel = assert_within_bound(got, x, torch.float32)
        assert rel < 0.04, rel
        assert torch.equal(got, want)
    dist.barrier()

    # --- offset resume: chunk 0 of the wire buffer already delivered -----
    per = tr._chunk_elems(1)
    if rank == 0:
        works, keep = tr.isend_value(x, None, dst=1, offset_chunks=1, tag=12)
        assert len(works) == len(range(per, mx8_nbytes(n), per))
        _wait(works)
    else:
        buf = torch.zeros(mx8_nbytes(n), dtype=torch.uint8)
        buf[:per] = wire[:per]  # survived the failed attempt
        meta = describe_value("m2", torch.empty(n, dtype=torch.float32))
        works, fin = tr.irecv_value(meta, src=0, offset_chunks=1, into=buf, tag=12)
        _wait(works)
        assert torch.equal(buf, wire)
        assert torch.equal(fin(), want)
    dist.barrier()

    # --- below the size threshold / not a float dtype: uncast ------------
    small = torch.randn(1000, generator=g) * 1e-4
    ints = torch.arange(1 << 17, dtype=torch.int64) * 7919 - 12345
    for i, t in enumerate((small, ints)):
        if rank == 0:
            works, keep = tr.isend_value(t, None, dst=1, tag=20 + i)
            assert keep.dtype == t.dtype
            _wait(works)
        else:
            meta = describe_value(f"m3{i}", torch.empty_like(t))
            works, fin = tr.irecv_value(meta, src=0, tag=20 + i)
            _wait(works)
            got = fin()
            assert got.dtype == t.dtype and torch.equal(got, t)
        dist.barrier()


def cuda_scenario(rank: int) -> None:
    """Device bf16 tensor, 2 ranks on one GPU: packed by the HIP kernel,
    staged through the host, unpacked by the HIP kernel on arrival."""
    import lzy_amd.ops as ops

    assert ops.NATIVE, "HIP ops must be built+loadable on a GPU box"
    Config.reset(channel_chunk_mb=1, channel_wire_cast="mxfp8")
    dev = torch.device("cuda", 0)
    tr = Transport(None, dev, world=dist.get_world_size())
    assert not tr._cuda_p2p  # ranks outnumber GPUs -> host staging
    n = (1 << 17) + 9
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(n, generator=g) * 1e-4).to(torch.bfloat16)
    if rank == 0:
        works, keep = tr.isend_value(x.to(dev), None, dst=1, tag=31)
        assert keep.dtype == torch.uint8 and not keep.is_cuda
        assert keep.numel() == mx8_nbytes(n)
        _wait(works)
    else:
        meta = describe_value("g1", torch.empty(n, dtype=torch.bfloat16, device=dev))
        works, fin = tr.irecv_value(meta, src=0, tag=31)
        _wait(works)
        got = fin()
        torch.cuda.synchronize()
        assert got.is_cuda and got.dtype == torch.bfloat16 and got.shape == (n,)
        rel = assert_within_bound(got, x, torch.bfloat16)
        assert rel < 0.04, rel
    dist.barrier()


def main() -> None:
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    if os.environ.get("MXWIRE_DEVICE") == "cuda":
        cuda_scenario(rank)
    else:
        cpu_scenario(rank)
    if rank == 0:
        print("MXWIRE-TRANSPORT-OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
