"""A wired plan on the MXFP4 wire, world 2 over gloo, CPU tensors: a
four-leaf tree whose ranks each combine a leaf of their own with one of the
other's; rank 1 FORWARDS its result (the two-step wire_fused path) and rank
0 combines the two.  Every output must equal the torch codec applied edge by
edge, bit for bit, and each rank's plan_stats["wire_bytes"] the mx4 sizes of
what it sent.  Prints MXFP4-PLAN-OK on rank 0.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from lzy_amd.channels.mxwire import mx4_axpby_torch, mx4_nbytes, mx4_pack_torch
from lzy_amd.channels.treeplan import build_plan, find_components, run_stream_plan
from mxplan_util import FakeCall, chunk_bounds, tensor_meta

N = 65536 + 40               # 5 chunks of 16384; the last ends in a block of 8
ALPHA, BETA = 0.5, -1.5


class Store(dict):
    has = dict.__contains__
    put = dict.__setitem__

    def wait_present(self, eid, timeout):
        return eid in self


def main() -> None:
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    leaves = {f"leaf{i}": torch.randn(N, generator=torch.Generator().manual_seed(40 + i))
              for i in range(4)}
    owners = {"leaf0": 0, "leaf1": 1, "leaf2": 1, "leaf3": 0}
    box = [None]
    if rank == 0:
        c1 = FakeCall(["leaf0", "leaf1"], pair_reduce=(ALPHA, BETA))
        c2 = FakeCall(["leaf2", "leaf3"], pair_reduce=(ALPHA, BETA))
        c3 = FakeCall([c1.entry_ids[0], c2.entry_ids[0]], pair_reduce=(ALPHA, BETA))
        calls = {"t0": c1, "t1": c2, "t2": c3}
        metas = {e: tensor_meta(e, owner=o, shape=(N,)) for e, o in owners.items()}
        [order] = find_components(calls)
        box[0] = build_plan("p", order, calls, metas.get, chunk_bytes=1 << 16,
                            cuda_p2p=False, wire="mxfp4")
    dist.broadcast_object_list(box, src=0)
    plan = box[0]
    steps = {int(r): s for r, s in plan["steps_by_rank"].items()}
    assert plan["wire"] == "mxfp4" and plan["chunk_elems"] == 16384
    [fwd] = [s for s in steps[1] if s["op"] == "node"]
    assert fwd["send_to"] and fwd["remote_src"] == 0, "no forwarding node"

    store = Store({e: leaves[e] for e, o in owners.items() if o == rank})
    results = run_stream_plan(plan, steps[rank], store, None, None)

    def hop(a, b):
        out = torch.empty_like(a)
        for s, e in chunk_bounds(plan):
            out[s:e] = mx4_axpby_torch(a[s:e], mx4_pack_torch(b[s:e]), ALPHA, BETA)
        return out

    m01 = hop(leaves["leaf0"], leaves["leaf1"])
    m23 = hop(leaves["leaf2"], leaves["leaf3"])
    want = [m01, hop(m01, m23)] if rank == 0 else [m23]
    nodes = [s for s in steps[rank] if s["op"] == "node"]
    assert len(nodes) == len(want)
    for st, w in zip(nodes, want):
        assert torch.equal(store[st["out"]], w), f"rank {rank} {st['out']}: not bit-identical"
    # rank 0 sends one edge (a leaf), rank 1 two (a leaf, the forwarded output)
    edge = sum(mx4_nbytes(e - s) for s, e in chunk_bounds(plan))
    assert edge == 17 * -(-N // 32)
    assert results[0]["plan_stats"]["wire_bytes"] == (1 + rank) * edge
    dist.barrier()
    if rank == 0:
        print("MXFP4-PLAN-OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
