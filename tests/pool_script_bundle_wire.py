"""Tensor bundles on the MXFP8 wire for a 2-rank pool — run under
torch.distributed.run by tests/test_bundle_wire.py (CPU leaves over gloo)
and tests/test_gpu_bundle_wire.py (BUNDLE_DEVICE=cuda: device leaves, both
ranks on one GPU, the host-staged path).

The placement is that of tests/pool_script_bundle.py: producer ``i`` runs
beside anchor ``i``, consumer ``i`` beside the next anchor, so at least two
consumers receive a cross-rank bundle transfer.

With LZY_BUNDLE_WIRE_CAST=mxfp8 (the driver's setting; the worker never
reads it) a cross-rank consumer, and the driver-side read of a value made
on the other rank, see the large float leaves after one MXFP8 round trip —
on the CPU exactly the torch codec's decode, on a device within the
docs/mxwire.md bound — and every other leaf bit-exact; a same-rank consumer
sees the exact object; ``lzy_transfers_bundle_wired >= 1``.  With the key
unset every value is bit-exact and the counter stays 0.

Prints BUNDLE-WIRE-SCRIPT-OK on success (rank 0).
"""
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from lzy_amd import Lzy, op
from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch
from lzy_amd.proxy import get_proxy_entry_id, materialize
from lzy_amd.runtime.pool import GpuPool, GpuPoolRuntime
from lzy_amd.utils.metrics import METRICS
from mxwire_util import assert_within_bound

DEVICE = os.environ.get("BUNDLE_DEVICE", "cpu")
WIRE = os.environ.get("LZY_BUNDLE_WIRE_CAST", "")
N_PAIRS = 4
WIRED_KEYS = ("w", "h")


def reference(i: int) -> "OrderedDict":
    """The producer's value with CPU leaves, rebuilt from the seed alone."""
    g = torch.Generator().manual_seed(2000 + i)
    sd = OrderedDict()
    sd["w"] = torch.randn(300, 257, generator=g)                      # wired
    sd["h"] = (torch.randn(65536 + 7, generator=g) * 1e-3).to(torch.bfloat16)
    sd["b"] = torch.randn(200, generator=g)                           # small
    sd["steps"] = torch.arange(7 + i, dtype=torch.int64)
    sd["mask"] = torch.rand(33, generator=g) > 0.5
    sd["epoch"] = 3 + i
    sd["note"] = f"run-{i}"
    return sd


def _bytes(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def _check(got, i: int, quantized: bool) -> None:
    want = reference(i)
    want["rank"] = got["rank"]
    assert type(got) is OrderedDict
    assert list(got.keys()) == list(want.keys()), list(got.keys())
    for k, w in want.items():
        g = got[k]
        if not isinstance(w, torch.Tensor):
            assert type(g) is type(w) and g == w, (k, g, w)
            continue
        assert type(g) is torch.Tensor and g.dtype == w.dtype \
            and g.shape == w.shape, (k, g.dtype, g.shape)
        if quantized and k in WIRED_KEYS:
            if DEVICE == "cuda":
                # the sender's kernel rounds with the hardware convert
                assert_within_bound(g, w, w.dtype)
                assert not torch.equal(_bytes(g), _bytes(w)), f"{k} not wired"
            else:
                oracle = mx8_unpack_torch(mx8_pack_torch(w), w.shape, w.dtype)
                assert torch.equal(_bytes(g), _bytes(oracle)), f"leaf {k}"
        else:
            assert torch.equal(_bytes(g), _bytes(w)), f"leaf {k} differs"


@op
def anchor(i: int) -> torch.Tensor:
    return torch.full((256,), float(i))


@op
def produce(a: torch.Tensor, i: int) -> OrderedDict:
    sd = reference(i)
    if DEVICE == "cuda":
        for k, v in list(sd.items()):
            if isinstance(v, torch.Tensor):
                sd[k] = v.to("cuda")
    sd["rank"] = int(os.environ.get("RANK", "0"))
    return sd


@op
def consume(sd: OrderedDict, place: torch.Tensor, i: int) -> dict:
    my_rank = int(os.environ.get("RANK", "0"))
    crossed = sd["rank"] != my_rank
    _check(sd, i, quantized=crossed and WIRE == "mxfp8")
    leaves = [v for v in sd.values() if isinstance(v, torch.Tensor)]
    one_alloc = len({v.untyped_storage().data_ptr() for v in leaves}) == 1
    if DEVICE == "cuda":
        cur = torch.device("cuda", torch.cuda.current_device())
        assert all(v.device == cur for v in leaves), [v.device for v in leaves]
    else:
        assert all(v.device.type == "cpu" for v in leaves)
    return {"producer": sd["rank"], "consumer": my_rank, "crossed": crossed,
            "one_alloc": one_alloc}


def main() -> None:
    GpuPool.get()  # workers serve here and never return
    lzy = Lzy(runtime=GpuPoolRuntime())

    with lzy.workflow("bundle-wire-wf") as wf:
        anchors = [anchor(i) for i in range(N_PAIRS)]
        sds = [produce(anchors[i], i) for i in range(N_PAIRS)]
        outs = [consume(sds[i], anchors[(i + 1) % N_PAIRS], i)
                for i in range(N_PAIRS)]
        outs = [dict(materialize(o)) for o in outs]
        metas = [wf._entry_meta[get_proxy_entry_id(s)] for s in sds]
        # the driver-side read: rank 0's copy — the exact object when the
        # producer ran here, a transferred (quantized) copy otherwise
        for i, s in enumerate(sds):
            got = materialize(s)
            _check(got, i, quantized=got["rank"] != 0 and WIRE == "mxfp8")

    print("outs", outs, flush=True)
    crossed = [o for o in outs if o["crossed"]]
    assert crossed, f"no producer ran on the other rank: {outs}"
    for o, meta in zip(outs, metas):
        assert meta.kind == "bundle", meta.kind
        if o["crossed"]:
            assert o["one_alloc"], o
    n = METRICS.counter_value("lzy_transfers_bundle")
    wired = METRICS.counter_value("lzy_transfers_bundle_wired")
    assert n >= len(crossed) >= 1, (n, crossed)
    if WIRE == "mxfp8":
        assert wired >= len(crossed) >= 1, (wired, crossed)
    else:
        assert wired == 0, wired
    print("BUNDLE-WIRE-SCRIPT-OK", flush=True)


if __name__ == "__main__":
    main()
