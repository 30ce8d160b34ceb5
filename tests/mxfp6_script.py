"""The MXFP6 wire under torchrun, world 2 on gloo: streamed_reduce_pair with the
tensors on MXFP6_DEVICE, then (CPU only) the four-leaf plan of
tests/mxfp4_plan_script.py, whose rank 1 forwards.  Every result must equal
the torch codec applied edge by edge and chunk by chunk, bit for bit.  Prints
MXFP6-PAIR-OK and MXFP6-PLAN-OK on rank 0.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels.mxwire import mx6_axpby_torch, mx6_nbytes, mx6_pack_torch
from lzy_amd.channels.streaming import streamed_reduce_pair
from lzy_amd.channels.treeplan import build_plan, find_components, run_stream_plan
from mxfp4_plan_script import Store
from mxplan_util import FakeCall, chunk_bounds, tensor_meta

ALPHA, BETA = 0.5, -1.5      # dyadic: the fp32 FMA and the float64 host sum agree


def hop(a, b, bounds):
    out = torch.empty_like(a)
    for s, e in bounds:
        out[s:e] = mx6_axpby_torch(a[s:e], mx6_pack_torch(b[s:e]), ALPHA, BETA)
    return out


def pair(rank, device):
    n, per = 3 * 25000 + 13, 25088      # chunk_bytes below: 25000 -> 25088 elements
    xs = [torch.randn(n, generator=torch.Generator().manual_seed(70 + r)) * 3e3 for r in (0, 1)]
    for dtype in (torch.float32, torch.bfloat16):
        mine, theirs = xs[rank].to(dtype), xs[1 - rank].to(dtype)
        out = streamed_reduce_pair(
            mine.to(device), peer=1 - rank, is_receiver=(rank == 0), alpha=ALPHA,
            beta=BETA, chunk_bytes=25000 * mine.element_size(), wire="mxfp6")
        if rank == 0:
            want = hop(mine, theirs, [(s, min(s + per, n)) for s in range(0, n, per)])
            assert out.dtype == dtype and out.device.type == device
            assert torch.equal(out.cpu(), want), dtype
        dist.barrier()


def plan(rank):
    n = 65536 + 40               # 5 chunks of 16384; the last ends in a block of 8
    leaves = {f"leaf{i}": torch.randn(n, generator=torch.Generator().manual_seed(40 + i))
              for i in range(4)}
    owners = {"leaf0": 0, "leaf1": 1, "leaf2": 1, "leaf3": 0}
    c1, c2 = (FakeCall(pair, pair_reduce=(ALPHA, BETA))
              for pair in (["leaf0", "leaf1"], ["leaf2", "leaf3"]))
    calls = {"t0": c1, "t1": c2,
             "t2": FakeCall([c1.entry_ids[0], c2.entry_ids[0]], pair_reduce=(ALPHA, BETA))}
    metas = {e: tensor_meta(e, owner=o, shape=(n,)) for e, o in owners.items()}
    box = [build_plan("p", find_components(calls)[0], calls, metas.get, chunk_bytes=1 << 16,
                      cuda_p2p=False, wire="mxfp6")]
    dist.broadcast_object_list(box, src=0)     # rank 0's entry ids
    steps = {int(r): s for r, s in box[0]["steps_by_rank"].items()}
    assert box[0]["wire"] == "mxfp6" and box[0]["chunk_elems"] == 16384
    [fwd] = [s for s in steps[1] if s["op"] == "node"]
    assert fwd["send_to"] and fwd["remote_src"] == 0, "no forwarding node"
    store = Store({e: leaves[e] for e, o in owners.items() if o == rank})
    results = run_stream_plan(box[0], steps[rank], store, None, None)
    bounds = chunk_bounds(box[0])
    m01, m23 = (hop(leaves[a], leaves[b], bounds) for a, b in (("leaf0", "leaf1"), ("leaf2", "leaf3")))
    want = [m01, hop(m01, m23, bounds)] if rank == 0 else [m23]
    nodes = [s for s in steps[rank] if s["op"] == "node"]
    assert len(nodes) == len(want)
    for st, w in zip(nodes, want):
        assert torch.equal(store[st["out"]], w), f"rank {rank} {st['out']}: not bit-identical"
    # rank 0 sends one edge (a leaf), rank 1 two (a leaf, the forwarded output)
    edge = sum(mx6_nbytes(e - s) for s, e in bounds)
    assert edge == 25 * -(-n // 32) and results[0]["plan_stats"]["wire_bytes"] == (1 + rank) * edge
    dist.barrier()


if __name__ == "__main__":
    dist.init_process_group("gloo")
    rank, device = dist.get_rank(), os.environ.get("MXFP6_DEVICE", "cpu")
    pair(rank, device)
    if device == "cpu":
        plan(rank)
    if rank == 0:
        print("MXFP6-PAIR-OK" + (" MXFP6-PLAN-OK" if device == "cpu" else ""), flush=True)
    dist.destroy_process_group()
