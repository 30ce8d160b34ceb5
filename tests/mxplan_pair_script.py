"""streamed_reduce_pair(..., wire="mxfp8") — world_size 2 on gloo, CPU
tensors: both sides are the torch codec, so the receiver's result must
equal the host emulation (pack per 256-multiple chunk, fused
decode-combine) bit for bit.  Prints MXPLAN-PAIR-OK on rank 0.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels.mxwire import mx8_axpby_torch, mx8_pack_torch
from lzy_amd.channels.streaming import streamed_reduce_pair


def main() -> None:
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    n = 3 * 25000 + 13           # chunk_bytes below: 25000 -> 25088 elements
    per = 25088
    xs = [torch.randn(n, generator=torch.Generator().manual_seed(40 + r)) * 3e3
          for r in (0, 1)]
    for dtype in (torch.float32, torch.bfloat16):
        mine = xs[rank].to(dtype)
        out = streamed_reduce_pair(
            mine, peer=1 - rank, is_receiver=(rank == 0), alpha=0.75,
            beta=-1.5, chunk_bytes=25000 * mine.element_size(), wire="mxfp8",
        )
        if rank == 0:
            theirs = xs[1].to(dtype)
            want = torch.empty_like(mine)
            for s in range(0, n, per):
                e = min(s + per, n)
                want[s:e] = mx8_axpby_torch(
                    mine[s:e], mx8_pack_torch(theirs[s:e]), 0.75, -1.5
                )
            assert out.dtype == dtype and out.shape == mine.shape
            assert torch.equal(out, want), dtype
            exact = (mine.double() * 0.75 - theirs.double() * 1.5).to(dtype)
            assert not torch.equal(out, exact)
        else:
            assert out is None
        dist.barrier()
    # unknown wire names are refused on both sides, before any traffic
    try:
        streamed_reduce_pair(xs[rank], peer=1 - rank, is_receiver=(rank == 0),
                             wire="fp8")
        raise AssertionError("wire='fp8' was accepted")
    except ValueError:
        pass
    if rank == 0:
        print("MXPLAN-PAIR-OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
