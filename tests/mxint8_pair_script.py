"""streamed_reduce_pair(..., wire="mxint8") — world_size 2 on gloo.  With
CPU tensors both sides are the torch codec; with MXINT8_DEVICE=cuda the
tensors live on the device, the kernels pack and combine, and the packed
bytes are staged through the host.  Either way the receiver's result must
equal the host emulation (mxi8_pack_torch per 256-multiple chunk,
mxi8_axpby_torch) bit for bit, and stay inside the one-hop error bound of
docs/mxwire.md.  Prints MXINT8-PAIR-OK on rank 0.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels.mxwire import mxi8_axpby_torch, mxi8_pack_torch
from lzy_amd.channels.streaming import streamed_reduce_pair

ALPHA, BETA = 0.5, -1.5      # dyadic: the fp32 FMA and the float64 host sum agree


def main() -> None:
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    device = os.environ.get("MXINT8_DEVICE", "cpu")
    n = 3 * 25000 + 13           # chunk_bytes below: 25000 -> 25088 elements
    per = 25088
    xs = [torch.randn(n, generator=torch.Generator().manual_seed(60 + r)) * 3e3
          for r in (0, 1)]
    for dtype in (torch.float32, torch.bfloat16):
        mine = xs[rank].to(dtype)
        out = streamed_reduce_pair(
            mine.to(device), peer=1 - rank, is_receiver=(rank == 0), alpha=ALPHA,
            beta=BETA, chunk_bytes=25000 * mine.element_size(), wire="mxint8",
        )
        if rank == 0:
            theirs = xs[1].to(dtype)
            want = torch.empty_like(mine)
            for s in range(0, n, per):
                e = min(s + per, n)
                want[s:e] = mxi8_axpby_torch(
                    mine[s:e], mxi8_pack_torch(theirs[s:e]), ALPHA, BETA
                )
            assert out.dtype == dtype and out.shape == mine.shape
            assert out.device.type == device
            assert torch.equal(out.cpu(), want), dtype
            # one hop: |x^ - x| <= amax_block * 2^-7 * 256/255 on the remote
            # operand, scaled by |beta|, plus the accumulator's own rounding
            exact = mine.double() * ALPHA + theirs.double() * BETA
            pad = torch.zeros(-n % 32, dtype=torch.float64)
            amax = torch.cat([theirs.double(), pad]).view(-1, 32).abs().amax(1)
            bound = (amax * 2.0 ** -7 * 256 / 255 * abs(BETA)).repeat_interleave(32)[:n]
            bound = bound + exact.abs() * (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23)
            err = (out.cpu().double() - exact).abs()
            assert bool((err <= bound).all()), float((err - bound).max())
            assert float(err.max()) > 0
        else:
            assert out is None
        dist.barrier()
    if rank == 0:
        print("MXINT8-PAIR-OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
