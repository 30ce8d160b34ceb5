"""Tensor-bundle scenario for a 2-rank pool — run under torch.distributed.run
by tests/test_bundle.py (CPU leaves over gloo) and tests/test_gpu_bundle.py
(BUNDLE_DEVICE=cuda: device leaves, both ranks on one GPU, the host-staged
path).

Producers return an ``OrderedDict`` of tensors plus scalars; each runs on
the rank that holds its anchor tensor (data affinity), the four anchors
spread over both ranks.  Consumer ``i`` is placed by the NEXT anchor
(cyclically), so wherever the anchors landed at least two consumers sit on
the other rank than their producer and receive a cross-rank bundle
transfer.  An inspector op then runs beside each producer and looks into
that rank's store.

BUNDLE_EXPECT=bundle: the entry's kind is ``bundle``, the producer's store
holds no pickle of it, ``lzy_transfers_bundle >= 1``, received leaves are
views of one allocation on the consumer's own device.
BUNDLE_EXPECT=bytes (LZY_CHANNEL_BUNDLES=0): the parent path — the same
values arrive equal, pickled.

Prints BUNDLE-SCRIPT-OK on success (rank 0).
"""
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from lzy_amd import Lzy, op
from lzy_amd.proxy import get_proxy_entry_id, materialize
from lzy_amd.runtime.pool import GpuPool, GpuPoolRuntime
from lzy_amd.utils.metrics import METRICS

DEVICE = os.environ.get("BUNDLE_DEVICE", "cpu")
EXPECT = os.environ.get("BUNDLE_EXPECT", "bundle")
N_PAIRS = 4


def reference(i: int) -> "OrderedDict":
    """The producer's value with CPU leaves, rebuilt from the seed alone
    (a private generator: ops of one rank run on concurrent threads)."""
    g = torch.Generator().manual_seed(1000 + i)
    if DEVICE == "cuda":
        from lzy_amd.models.transformer import TransformerLM

        model = TransformerLM(vocab=64, d_model=64, n_layers=2, n_heads=4,
                              max_seq=16)
        sd = model.state_dict()
        for v in sd.values():
            v.copy_(torch.randn(v.shape, generator=g))
    else:
        sd = OrderedDict()
        sd["w"] = torch.randn(96, 200, generator=g)
        sd["b"] = torch.randn(200, generator=g).to(torch.bfloat16)
        sd["steps"] = torch.arange(7, dtype=torch.int64)
        sd["mask"] = torch.rand(33, generator=g) > 0.5
        sd["scalar"] = torch.tensor(2.5, dtype=torch.float64)
        sd["empty"] = torch.empty(0, 4)
    sd["epoch"] = 3 + i
    sd["note"] = f"run-{i}"
    return sd


def _same(got, want) -> None:
    assert type(got) is type(want), (type(got), type(want))
    assert list(got.keys()) == list(want.keys()), list(got.keys())
    for k, w in want.items():
        g = got[k]
        if isinstance(w, torch.Tensor):
            assert type(g) is torch.Tensor and g.dtype == w.dtype \
                and g.shape == w.shape, (k, g.dtype, g.shape)
            gb = g.detach().cpu().contiguous().reshape(-1).view(torch.uint8)
            wb = w.contiguous().reshape(-1).view(torch.uint8)
            assert torch.equal(gb, wb), f"leaf {k} differs"
        else:
            assert type(g) is type(w) and g == w, (k, g, w)


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
    want = reference(i)
    want["rank"] = sd["rank"]
    _same(sd, want)
    leaves = [v for v in sd.values() if isinstance(v, torch.Tensor)]
    my_rank = int(os.environ.get("RANK", "0"))
    crossed = sd["rank"] != my_rank
    one_alloc = len({v.untyped_storage().data_ptr() for v in leaves}) == 1
    if DEVICE == "cuda":
        cur = torch.device("cuda", torch.cuda.current_device())
        assert all(v.device == cur for v in leaves), [v.device for v in leaves]
    else:
        assert all(v.device.type == "cpu" for v in leaves)
    return {"producer": sd["rank"], "consumer": my_rank, "crossed": crossed,
            "one_alloc": one_alloc}


@op
def inspect_store(a: torch.Tensor, after: dict, i: int) -> dict:
    """Runs beside producer ``i`` (same anchor): is its output pickled?"""
    store = GpuPool._instance.agent.store
    found = pickled = 0
    for eid, v in list(store.values.items()):
        if type(v) is OrderedDict and v.get("note") == f"run-{i}":
            found += 1
            pickled += eid in store.pickled
    return {"rank": int(os.environ.get("RANK", "0")), "found": found,
            "pickled": pickled}


def main() -> None:
    GpuPool.get()  # workers serve here and never return
    lzy = Lzy(runtime=GpuPoolRuntime())

    with lzy.workflow("bundle-wf") as wf:
        anchors = [anchor(i) for i in range(N_PAIRS)]
        sds = [produce(anchors[i], i) for i in range(N_PAIRS)]
        outs = [consume(sds[i], anchors[(i + 1) % N_PAIRS], i)
                for i in range(N_PAIRS)]
        looks = [inspect_store(anchors[i], outs[i], i)
                 for i in range(N_PAIRS)]
        outs = [dict(materialize(o)) for o in outs]
        looks = [dict(materialize(x)) for x in looks]
        metas = [wf._entry_meta[get_proxy_entry_id(s)] for s in sds]
        # the driver-side read: fetched to rank 0 where it is not there yet
        for i, s in enumerate(sds):
            got = materialize(s)
            want = reference(i)
            want["rank"] = got["rank"]
            _same(got, want)

    print("outs", outs, "looks", looks, flush=True)
    crossed = [o for o in outs if o["crossed"]]
    assert crossed, f"no producer ran on the other rank: {outs}"
    for o, look, meta in zip(outs, looks, metas):
        assert look["rank"] == o["producer"] and look["found"] >= 1, (o, look)
        if EXPECT == "bundle":
            assert meta.kind == "bundle", meta.kind
            assert look["pickled"] == 0, look
            if o["crossed"]:
                assert o["one_alloc"], o
        else:
            assert meta.kind == "bytes", meta.kind
            assert look["pickled"] == look["found"], look
    n = METRICS.counter_value("lzy_transfers_bundle")
    if EXPECT == "bundle":
        assert n >= len(crossed) >= 1, (n, crossed)
    else:
        assert n == 0, n
    print("BUNDLE-SCRIPT-OK", flush=True)


if __name__ == "__main__":
    main()
