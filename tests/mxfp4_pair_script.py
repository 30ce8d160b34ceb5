"""streamed_reduce_pair(..., wire="mxfp4"), world 2 on gloo, the tensors on
MXFP4_DEVICE (cuda: both ranks on one GPU, kernel pack, packed bytes staged
through the host, kernel decode-combine).  The receiver's result must equal
the torch codec on the same inputs (mx4_pack_torch per 256-multiple chunk,
mx4_axpby_torch) bit for bit.  Prints MXFP4-PAIR-OK on rank 0.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels.mxwire import mx4_axpby_torch, mx4_pack_torch
from lzy_amd.channels.streaming import streamed_reduce_pair

ALPHA, BETA = 0.5, -1.5      # dyadic: the fp32 FMA and the float64 host sum agree


def main() -> None:
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    device = os.environ.get("MXFP4_DEVICE", "cpu")
    n, per = 3 * 25000 + 13, 25088      # chunk_bytes below: 25000 -> 25088 elements
    xs = [torch.randn(n, generator=torch.Generator().manual_seed(70 + r)) * 3e3
          for r in (0, 1)]
    for dtype in (torch.float32, torch.bfloat16):
        mine = xs[rank].to(dtype)
        out = streamed_reduce_pair(
            mine.to(device), peer=1 - rank, is_receiver=(rank == 0), alpha=ALPHA,
            beta=BETA, chunk_bytes=25000 * mine.element_size(), wire="mxfp4",
        )
        if rank == 0:
            theirs = xs[1].to(dtype)
            want = torch.empty_like(mine)
            for s in range(0, n, per):
                e = min(s + per, n)
                want[s:e] = mx4_axpby_torch(mine[s:e], mx4_pack_torch(theirs[s:e]),
                                            ALPHA, BETA)
            assert out.dtype == dtype and out.device.type == device
            assert torch.equal(out.cpu(), want), dtype
            assert not torch.equal(want, (mine.double() * ALPHA + theirs.double() * BETA).to(dtype))
        else:
            assert out is None
        dist.barrier()
    if rank == 0:
        print("MXFP4-PAIR-OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
