"""Wired streamed merge-tree plans (stream_wire_cast="mxfp8"), world 4
over gloo: the remote edges of a pair_reduce tree cross the link as MXFP8
chunks and are combined by the fused decode (channels/treeplan.py,
docs/mxwire.md).

The driver records every plan it builds and replays it on the host with
the torch codec (tests/mxplan_util.py).  With CPU leaves both sides of
every edge ARE the torch codec, so root and interior outputs must equal
that replay bit for bit; with device leaves (MXPLAN_DEVICE=cuda, all
ranks on one GPU: kernel pack, host staging, kernel decode-combine) the
hardware e4m3 rounding may differ in rare elements, so the check is the
propagated per-hop error bound instead.
"""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import lzy_amd.channels.treeplan as treeplan
from lzy_amd import Lzy, op
from lzy_amd.config import Config
from lzy_amd.proxy import get_proxy_entry_id, materialize
from lzy_amd.runtime.pool import GpuPool, GpuPoolRuntime
from lzy_amd.utils.metrics import METRICS
from mxplan_util import (
    edge_wire_bytes,
    emulate_plan,
    exact_and_bound,
    plan_nodes,
    remote_edges,
)

N = (1 << 20) + 40  # 4 chunks of 262400; the last ends in a block of 8
ON_DEVICE = os.environ.get("MXPLAN_DEVICE") == "cuda"


def leaf(i: int) -> torch.Tensor:
    return torch.randn(N, generator=torch.Generator().manual_seed(1000 + i))


@op
def make_shard(i: int) -> torch.Tensor:
    t = leaf(i)
    return t.cuda() if ON_DEVICE else t


@op(pair_reduce=(0.5, 0.5))
def merge(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a + b) * 0.5


@op(pair_reduce=(1.0, -1.0))
def diff(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a - b


@op
def fetch(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu()


RECORDED = []
_build_plan = treeplan.build_plan


def _recording_build_plan(*args, **kwargs):
    plan = _build_plan(*args, **kwargs)
    if plan is not None:
        RECORDED.append(copy.deepcopy(plan))
    return plan


def host(v) -> torch.Tensor:
    return materialize(fetch(v)).detach().cpu().reshape(-1)


def run_tree(lzy):
    """4-leaf merge(0.5, 0.5) tree; returns (plan, leaf values by entry
    id, {out entry id: tensor} for the root and both interior nodes)."""
    RECORDED.clear()
    with lzy.workflow("mxplan-tree") as wf:
        shards = [make_shard(i) for i in range(4)]
        wf.barrier()
        m01 = merge(shards[0], shards[1])
        m23 = merge(shards[2], shards[3])
        root = merge(m01, m23)
        got = {get_proxy_entry_id(v): host(v) for v in (m01, m23, root)}
        leaves = {get_proxy_entry_id(s): leaf(i) for i, s in enumerate(shards)}
    assert len(RECORDED) == 1, f"tree was not folded into one plan: {len(RECORDED)}"
    return RECORDED[0], leaves, got


def run_chain(lzy):
    """(1.0, -1.0) chain, the accumulator passed first (local-first)."""
    RECORDED.clear()
    with lzy.workflow("mxplan-chain") as wf:
        shards = [make_shard(i) for i in range(3)]
        # leaves first: a component launches as soon as its ENTRY members
        # are ready (d01 here), and folds only if every leaf it reaches
        # (the third shard too) has a confirmed owner by then
        wf.barrier()
        d01 = diff(shards[0], shards[1])
        d = diff(d01, shards[2])
        got = {get_proxy_entry_id(v): host(v) for v in (d01, d)}
        leaves = {get_proxy_entry_id(s): leaf(i) for i, s in enumerate(shards)}
    assert len(RECORDED) == 1, f"chain was not folded into one plan: {len(RECORDED)}"
    return RECORDED[0], leaves, got


def check_wired(name, plan, leaves, got, wire_bytes):
    assert plan["wire"] == "mxfp8", plan["wire"]
    assert plan["chunk_elems"] == 262400, plan["chunk_elems"]
    assert plan["numel"] == N
    edges = remote_edges(plan)
    assert edges >= 1, "no cross-rank edge: the wire was never used"
    unwired = dict(plan, wire="")
    exact = emulate_plan(unwired, leaves)
    # bytes handed to isend, summed over ranks: one MXFP8 buffer per chunk
    want_bytes = edges * edge_wire_bytes(plan)
    assert wire_bytes == want_bytes, (wire_bytes, want_bytes)
    ratio = want_bytes / (edges * edge_wire_bytes(unwired))
    assert abs(ratio - 33 / 128) < 1e-4, ratio
    if ON_DEVICE:
        for eid, (ex, bound) in exact_and_bound(plan, leaves).items():
            err = (got[eid].double() - ex).abs()
            worst = (err - bound).max().item()
            print(f"MXPLAN {name} {eid}: max err {err.max().item():.3e}, "
                  f"max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}",
                  flush=True)
            assert worst <= 0, f"{name} {eid}: bound exceeded by {worst}"
    else:
        want = emulate_plan(plan, leaves)
        for eid, w in want.items():
            assert torch.equal(got[eid], w), f"{name} {eid}: not bit-identical"
    # every output downstream of a wired edge must show it
    wired_outs = set()
    for n in plan_nodes(plan):
        if n["remote"] is not None or n["local"] in wired_outs \
                or n["local2"] in wired_outs:
            wired_outs.add(n["out"])
    assert plan_nodes(plan)[-1]["out"] in wired_outs
    for eid in wired_outs:
        assert not torch.equal(got[eid], exact[eid]), f"{name} {eid}: exact?"


def main() -> None:
    GpuPool.get()
    treeplan.build_plan = _recording_build_plan
    lzy = Lzy(runtime=GpuPoolRuntime())

    Config.reset(stream_wire_cast="mxfp8")
    for name, run in (("tree", run_tree), ("chain", run_chain)):
        plans0 = METRICS.counter_value("lzy_stream_plans")
        bytes0 = METRICS.counter_value("lzy_stream_wire_bytes")
        xfer0 = METRICS.counter_value("lzy_transfer_bytes")
        plan, leaves, got = run(lzy)
        assert METRICS.counter_value("lzy_stream_plans") - plans0 >= 1
        sent = METRICS.counter_value("lzy_stream_wire_bytes") - bytes0
        check_wired(name, plan, leaves, got, sent)
        # the driver's transfer accounting shows the real wire bytes
        assert METRICS.counter_value("lzy_transfer_bytes") - xfer0 == sent
    print("MXPLAN-WIRED-OK", flush=True)

    # the field unset: plans stay exact, as before
    Config.reset()
    bytes0 = METRICS.counter_value("lzy_stream_wire_bytes")
    plan, leaves, got = run_tree(lzy)
    assert plan["wire"] == "" and plan["chunk_elems"] == (N + 3) // 4
    want = emulate_plan(plan, leaves)
    for eid, w in want.items():
        assert torch.equal(got[eid], w), f"unwired {eid}"
    sent = METRICS.counter_value("lzy_stream_wire_bytes") - bytes0
    assert sent == remote_edges(plan) * N * 4, sent

    # a value the scheduler must refuse
    Config.reset(stream_wire_cast="fp8")
    try:
        with lzy.workflow("mxplan-bad"):
            float(materialize(merge(make_shard(0), make_shard(1))).sum())
        raised = False
    except ValueError:
        raised = True
    assert raised, "stream_wire_cast='fp8' was accepted"
    print("MXPLAN-OK", flush=True)
    os._exit(0)


if __name__ == "__main__":
    main()
