"""Shared helpers of the wired (MXFP8) streamed-plan tests: the fake DAG
calls of the plan-builder unit tests, a host emulation of a recorded plan
through the torch codec, and the error bound a wired plan must keep."""
import math

import torch

from lzy_amd.channels.mxwire import (
    mx8_axpby_torch,
    mx8_nbytes,
    mx8_pack_torch,
)
from lzy_amd.channels.transport import EntryMeta
from mxwire_util import block_amax


class FakeCall:
    _n = 0

    def __init__(self, inputs, outputs=1, pair_reduce=None, kwargs=None):
        FakeCall._n += 1
        self.pair_reduce = pair_reduce
        self._inputs = tuple(inputs)
        self.entry_ids = tuple(f"out{FakeCall._n}_{i}" for i in range(outputs))
        self.kwarg_entry_ids = dict(kwargs or {})

    def input_entry_ids(self):
        return self._inputs + tuple(self.kwarg_entry_ids.values())


def tensor_meta(eid, owner, shape=(1024,), dtype="float32", device="cpu"):
    return EntryMeta(
        entry_id=eid, owners={owner}, kind="tensor", shape=shape,
        dtype=dtype, device_type=device,
        nbytes=4 * math.prod(shape),
    )


def make_tree(width, shape=(1024,), dtype="float32"):
    """width leaves (leaf i on rank i) -> pairwise merge tree."""
    FakeCall._n = 0
    calls = {}
    leaves = [f"leaf{i}" for i in range(width)]
    metas = {
        e: tensor_meta(e, owner=i, shape=shape, dtype=dtype)
        for i, e in enumerate(leaves)
    }
    layer = leaves[:]
    while len(layer) > 1:
        nxt = []
        for i in range(0, len(layer) - 1, 2):
            c = FakeCall([layer[i], layer[i + 1]], pair_reduce=(0.5, 0.5))
            calls[f"t{len(calls)}"] = c
            nxt.append(c.entry_ids[0])
        if len(layer) % 2:
            nxt.append(layer[-1])
        layer = nxt
    return calls, metas


# ---------------------------------------------------------------------------
# a recorded plan (build_plan's return value, steps_by_rank included)
# ---------------------------------------------------------------------------

def plan_nodes(plan):
    """The plan's node steps in topo order, each with the entry id of its
    remote operand resolved (``remote``: None for a local-local node)."""
    steps = {int(r): sts for r, sts in plan["steps_by_rank"].items()}
    nodes = []
    for rank, sts in steps.items():
        for st in sts:
            if st["op"] != "node":
                continue
            remote = None
            if st["remote_src"] is not None:
                for o in steps[st["remote_src"]]:
                    if (o["op"] == "leaf_send" and o["topo"] == st["topo"]
                            and o["dst"] == rank):
                        remote = o["entry"]
                    elif o["op"] == "node" and any(
                        d == rank and t == st["topo"] for d, t in o["send_to"]
                    ):
                        remote = o["out"]
                assert remote is not None, st
            nodes.append({**st, "rank": rank, "remote": remote})
    nodes.sort(key=lambda s: s["topo"])
    return nodes


def chunk_bounds(plan):
    per, numel = plan["chunk_elems"], plan["numel"]
    return [(s, min(s + per, numel)) for s in range(0, numel, per)]


def edge_wire_bytes(plan):
    """Bytes one cross-rank edge of the plan hands to isend."""
    if plan.get("wire"):
        return sum(mx8_nbytes(e - s) for s, e in chunk_bounds(plan))
    elem = torch.empty(0, dtype=getattr(torch, plan["dtype"])).element_size()
    return plan["numel"] * elem


def remote_edges(plan):
    return sum(1 for n in plan_nodes(plan) if n["remote"] is not None)


def emulate_plan(plan, values):
    """Run the plan on the host.  ``values``: leaf entry id -> flat CPU
    tensor of the plan dtype.  A remote operand of a wired plan crosses as
    mx8_pack_torch per chunk and enters through mx8_axpby_torch; everything
    else is the executor's plain host combine.  Returns out entry id ->
    tensor, every interior node included."""
    vals = dict(values)
    for n in plan_nodes(plan):
        a = vals[n["local"]]
        alpha, beta = n["alpha"], n["beta"]
        out = torch.empty_like(a)
        if n["remote"] is None:
            torch.add(a * alpha, vals[n["local2"]], alpha=beta, out=out)
        elif plan.get("wire"):
            b = vals[n["remote"]]
            for s, e in chunk_bounds(plan):
                out[s:e] = mx8_axpby_torch(
                    a[s:e], mx8_pack_torch(b[s:e]), alpha, beta
                )
        else:
            torch.add(a * alpha, vals[n["remote"]], alpha=beta, out=out)
        vals[n["out"]] = out
    return {n["out"]: vals[n["out"]] for n in plan_nodes(plan)}


def exact_and_bound(plan, values):
    """Per node output: (exact float64 value, element-wise error bound) of
    a wired plan whose packs and combines may run on either codec.

    A remote operand x~ that already carries an error <= B (|x~ - E| <= B
    for its exact value E) picks up one hop of docs/mxwire.md:
    ``2^-4 |x~| + amax_block(x~) 2^-17`` (+ ``2^-8 |x~|`` when the decode
    feeds a 16-bit accumulator), with |x~| <= |E| + B.  Chunks are whole
    32-blocks, so the wire's blocks are the flat tensor's.  The combine
    scales the operands' bounds by |alpha|, |beta| and adds its own
    rounding: the fp32 product and the final rounding to the plan dtype,
    each at most one unit roundoff of the magnitudes involved."""
    dtype = getattr(torch, plan["dtype"])
    u_out = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9,
             torch.float16: 2.0 ** -11}[dtype]
    exact = {k: v.double() for k, v in values.items()}
    bound = {k: torch.zeros_like(v, dtype=torch.float64)
             for k, v in values.items()}
    for n in plan_nodes(plan):
        alpha, beta = abs(n["alpha"]), abs(n["beta"])
        e_l, b_l = exact[n["local"]], bound[n["local"]]
        other = n["remote"] if n["remote"] is not None else n["local2"]
        e_r, b_r = exact[other], bound[other]
        if n["remote"] is not None and plan.get("wire"):
            mag = e_r.abs() + b_r
            hop = mag * 2.0 ** -4 + block_amax(mag.float()).double() * (
                2.0 ** -17) * (1 + 2.0 ** -20)  # amax taken via fp32
            if dtype != torch.float32:
                hop = hop + mag * 2.0 ** -8
            b_r = b_r + hop
        e_o = e_l * n["alpha"] + e_r * n["beta"]
        mag_o = alpha * (e_l.abs() + b_l) + beta * (e_r.abs() + b_r)
        exact[n["out"]] = e_o
        bound[n["out"]] = (alpha * b_l + beta * b_r
                           + mag_o * (2.0 ** -24 + u_out))
    return {n["out"]: (exact[n["out"]], bound[n["out"]])
            for n in plan_nodes(plan)}
