"""Packed tensor bundles on the CPU: eligibility, spec, the torch codec
(the segmented-copy kernel's oracle), the host-side table builder, the meta
wire format, the config switch, and a two-rank gloo pool
(tests/pool_script_bundle.py).  The kernel itself: tests/test_gpu_bundle.py.
"""
import os
import socket
import subprocess
import sys
from collections import OrderedDict
from dataclasses import dataclass
from pathlib import Path

import pytest
import torch

from lzy_amd import ops
from lzy_amd.channels import bundle
from lzy_amd.channels.transport import (
    KIND_BUNDLE, KIND_BYTES, KIND_TENSOR, EntryMeta, describe_value,
)
from lzy_amd.config import Config

ROOT = Path(__file__).resolve().parent.parent
T = ops.SEGCOPY_TILE
# the byte lengths every pack test covers: around the vector widths, the
# layout alignment and the kernel's tile
SIZES = [0, 1, 2, 15, 16, 17, 127, 128, 129, T - 1, T, T + 1, 2 * T + 3]


def _big(n=20000):
    return torch.arange(n, dtype=torch.float32)  # 80 kB > BUNDLE_MIN_BYTES


# ---------------------------------------------------------------------------
# eligibility
# ---------------------------------------------------------------------------

@dataclass
class _Holder:
    w: torch.Tensor


@pytest.mark.parametrize("make", [
    lambda: {"w": _big()},
    lambda: OrderedDict(w=_big(), n=3, s="x", none=None),
    lambda: [_big(), _big(10)],
    lambda: (_big(), {"inner": [torch.zeros(3), (torch.ones(2),)]}),
    lambda: {"w": _big().reshape(100, 200).t()},  # dense, non-contiguous
    lambda: {"w": torch.zeros(bundle.BUNDLE_MIN_BYTES, dtype=torch.uint8)},
], ids=["dict", "ordered+scalars", "list", "nested", "transposed", "floor"])
def test_is_bundle_accepts(make):
    assert bundle.is_bundle(make())


class _MyDict(dict):
    pass


@pytest.mark.parametrize("make", [
    lambda: {"w": torch.nn.Parameter(_big())},
    lambda: {"w": _big().requires_grad_()},
    lambda: {"a": _big(), "b": torch.empty(4, device="meta")},
    lambda: _Holder(_big()),
    lambda: {"h": _Holder(_big()), "w": _big()},
    lambda: {"w": torch.zeros(bundle.BUNDLE_MIN_BYTES - 1, dtype=torch.uint8)},
    lambda: {"a": 1, "b": [2, "x"], "c": (None,)},
    lambda: _MyDict(w=_big()),
    lambda: {"w": _big().to_sparse()},
    lambda: _big(),
], ids=["parameter", "requires_grad", "mixed-devices", "dataclass",
        "dataclass-leaf", "under-64k", "no-tensor", "dict-subclass", "sparse",
        "bare-tensor"])
def test_is_bundle_rejects(make):
    v = make()
    assert not bundle.is_bundle(v)
    if not isinstance(v, torch.Tensor):
        assert describe_value("e", v).kind == KIND_BYTES  # pickled, as before


def test_shared_or_cyclic_containers_stay_pickled():
    inner = [_big()]
    assert not bundle.is_bundle({"a": inner, "b": inner})
    loop = [_big()]
    loop.append(loop)
    assert not bundle.is_bundle(loop)


# ---------------------------------------------------------------------------
# layout helpers and the kernel's table, against brute force
# ---------------------------------------------------------------------------

def test_segcopy_layout_and_nbytes():
    offs, total = ops.segcopy_layout(SIZES, 128)
    end = 0
    for n, off in zip(SIZES, offs):
        assert off % 128 == 0 and off >= end and off - end < 128
        end = off + n
    assert total % 128 == 0 and 0 <= total - end < 128
    assert ops.segcopy_nbytes(SIZES, 128) == total
    assert ops.segcopy_nbytes([], 128) == 0
    assert ops.segcopy_nbytes([0, 0], 128) == 0
    assert ops.segcopy_layout([5, 5], 1) == ([0, 5], 10)
    with pytest.raises(ValueError):
        ops.segcopy_layout([1], 48)
    with pytest.raises(ValueError):
        ops.segcopy_layout([-1], 128)


@pytest.mark.parametrize("sizes", [SIZES, SIZES[::-1], [0, 0, 0], [], [5 * T]],
                         ids=["sizes", "reversed", "all-empty", "none", "5T"])
def test_segcopy_table_matches_tile_enumeration(sizes):
    n = len(sizes)
    srcs = [1000 + 7 * i for i in range(n)]
    dsts = [5000 + 128 * i for i in range(n)]
    table, ntiles = ops.segcopy_table(srcs, dsts, sizes)
    assert len(table) == 4 * n + 1
    assert table[:n] == srcs and table[n:2 * n] == dsts
    assert table[2 * n:3 * n] == list(sizes)
    tile_start = table[3 * n:]
    # brute force: walk every segment's bytes in tile-sized steps
    tiles = []  # (segment, byte offset, length)
    for s, nb in enumerate(sizes):
        off = 0
        while off < nb:
            tiles.append((s, off, min(T, nb - off)))
            off += T
    assert ntiles == len(tiles)
    assert tile_start[0] == 0 and tile_start[-1] == ntiles
    for t, (s, off, ln) in enumerate(tiles):
        # the kernel's search: the largest s with tile_start[s] <= t
        lo = max(i for i in range(n) if tile_start[i] <= t)
        assert lo == s
        assert (t - tile_start[lo]) * T == off
        assert min(T, sizes[lo] - off) == ln
    covered = [sum(ln for s, _, ln in tiles if s == i) for i in range(n)]
    assert covered == list(sizes)


# ---------------------------------------------------------------------------
# spec
# ---------------------------------------------------------------------------

def _rich_value():
    g = torch.Generator().manual_seed(7)
    shared = torch.randn(33, generator=g)
    inner = OrderedDict()
    inner["z_last_key_first"] = torch.randn(300, 70, generator=g)
    inner["bf16"] = torch.randn(17, generator=g).to(torch.bfloat16)
    inner["f16"] = torch.randn(5, 3, generator=g).to(torch.float16)
    inner["a_key"] = shared
    value = OrderedDict()
    value["model"] = inner
    value["list"] = [
        torch.tensor(3.5, dtype=torch.float64),           # 0-dim
        torch.empty(0, 4),                                # 0 elements
        torch.rand(9, generator=g) > 0.5,                 # bool
        torch.randint(0, 255, (129,), generator=g, dtype=torch.uint8),
        torch.randint(-9, 9, (4, 2), generator=g, dtype=torch.int64),
        torch.randn(64, generator=g).to(torch.float8_e4m3fn),
        "a string", 12, None, 2.5,
    ]
    value["tuple"] = (torch.randn(40, 30, generator=g).t(), shared, ())
    value["epoch"] = 4
    return value, shared


def _nb(t):
    return t.numel() * t.element_size()


def test_bundle_spec_is_deterministic_and_needs_no_data():
    value, _ = _rich_value()
    spec = bundle.bundle_spec(value)
    assert spec == bundle.bundle_spec(value)
    assert spec == bundle.bundle_spec(_rich_value()[0])
    assert isinstance(spec["skeleton"], bytes)
    assert all(off % 128 == 0 for off, _, _ in spec["segs"])
    sizes = [
        _nb(torch.empty(shape, dtype=getattr(torch, dt)))
        for _, dt, shape in spec["segs"]
    ]
    assert spec["nbytes"] == ops.segcopy_nbytes(sizes, 128)
    assert [off for off, _, _ in spec["segs"]] == ops.segcopy_layout(sizes, 128)[0]
    # shapes and dtypes alone: same-shaped garbage gives the same spec
    other = {"w": torch.empty(20000)}
    assert bundle.bundle_spec(other) == bundle.bundle_spec({"w": _big()})
    # the repeated object is one segment: 12 tensor slots, 11 distinct leaves
    assert len(spec["segs"]) == 11
    with pytest.raises(ValueError):
        bundle.bundle_spec({"small": torch.zeros(3)})


# ---------------------------------------------------------------------------
# torch codec round trip
# ---------------------------------------------------------------------------

def _assert_same(got, want):
    assert type(got) is type(want), (type(got), type(want))
    if isinstance(want, torch.Tensor):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(
            got.contiguous().reshape(-1).view(torch.uint8),
            want.contiguous().reshape(-1).view(torch.uint8),
        )
    elif isinstance(want, dict):
        assert list(got.keys()) == list(want.keys())
        for k in want:
            _assert_same(got[k], want[k])
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            _assert_same(g, w)
    else:
        assert got == want


def test_round_trip_bit_exact_with_structure():
    value, _ = _rich_value()
    spec = bundle.bundle_spec(value)
    buf = bundle.pack_bundle(value)
    assert buf.dtype == torch.uint8 and buf.numel() == spec["nbytes"]
    got = bundle.unpack_bundle(buf, spec)
    _assert_same(got, value)
    # the repeated object comes back as one object
    assert got["model"]["a_key"] is got["tuple"][1]
    # leaves are views of the one buffer, at their offsets
    leaves = [got["model"]["z_last_key_first"], got["model"]["bf16"]]
    for leaf, (off, _, _) in zip(leaves, spec["segs"]):
        assert leaf.data_ptr() == buf.data_ptr() + off
    # every byte outside the leaves is zero
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for off, dt, shape in spec["segs"]:
        mask[off: off + _nb(torch.empty(shape, dtype=getattr(torch, dt)))] = False
    assert mask.any() and not buf[mask].any()


def test_state_dict_round_trip_keeps_metadata():
    model = torch.nn.Sequential(torch.nn.Linear(200, 100), torch.nn.BatchNorm1d(100))
    sd = model.state_dict()
    assert bundle.is_bundle(sd)
    got = bundle.unpack_bundle(bundle.pack_bundle(sd), bundle.bundle_spec(sd))
    _assert_same(got, sd)
    assert got._metadata == sd._metadata
    torch.nn.Sequential(
        torch.nn.Linear(200, 100), torch.nn.BatchNorm1d(100)
    ).load_state_dict(got)


def test_pack_tensors_torch_layout_and_pad():
    g = torch.Generator().manual_seed(3)
    leaves = [torch.randint(1, 255, (n,), generator=g, dtype=torch.uint8)
              for n in SIZES]
    buf, offs = ops.pack_tensors_torch(leaves)
    assert offs == ops.segcopy_layout(SIZES, 128)[0]
    assert buf.numel() == ops.segcopy_nbytes(SIZES, 128)
    want = torch.zeros_like(buf)
    for t, off in zip(leaves, offs):
        want[off: off + t.numel()] = t
    assert torch.equal(buf, want)
    # out= is overwritten entirely, stale bytes included
    out = torch.full_like(buf, 0xAB)
    assert ops.pack_tensors_torch(leaves, out=out)[0] is out
    assert torch.equal(out, want)
    views = ops.unpack_tensors(buf, offs, [t.shape for t in leaves],
                               [t.dtype for t in leaves])
    for v, t, off in zip(views, leaves, offs):
        assert torch.equal(v, t) and v.storage_offset() == off
        if t.numel():  # torch reports a null data_ptr for empty tensors
            assert v.data_ptr() == buf.data_ptr() + off
    with pytest.raises(ValueError):
        ops.pack_tensors_torch(leaves, out=torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError):  # a segment past the end of the buffer
        ops.unpack_tensors(buf[:128], [128], [(1,)], [torch.uint8])


def test_pack_tensors_rejects_cpu_leaves():
    with pytest.raises(ValueError):
        ops.pack_tensors([torch.zeros(4)])
    with pytest.raises(ValueError):
        ops.pack_tensors([])


# ---------------------------------------------------------------------------
# meta wire format, describe_value, config
# ---------------------------------------------------------------------------

_PARENT_KEYS = {"entry_id", "kind", "shape", "dtype", "device_type", "nbytes"}


def test_wire_dicts_of_other_kinds_are_unchanged():
    t = describe_value("e1", torch.zeros(4, 2))
    b = describe_value("e2", {"x": 1})
    assert t.kind == KIND_TENSOR and b.kind == KIND_BYTES
    assert set(t.to_wire()) == _PARENT_KEYS
    assert set(b.to_wire()) == _PARENT_KEYS
    back = EntryMeta.from_wire(t.to_wire())  # no "bundle" key: accepted
    assert back.bundle is None and back.shape == (4, 2)


def test_bundle_meta_survives_the_wire():
    value, _ = _rich_value()
    meta = describe_value("e3", value)
    assert meta.kind == KIND_BUNDLE and meta.device_type == "cpu"
    assert meta.bundle == bundle.bundle_spec(value)
    assert meta.nbytes == meta.bundle["nbytes"]
    wire = meta.to_wire()
    assert set(wire) == _PARENT_KEYS | {"bundle"}
    back = EntryMeta.from_wire(wire)
    assert back.kind == KIND_BUNDLE and back.bundle == meta.bundle
    assert back.nbytes == meta.nbytes and back.device_type == "cpu"
    _assert_same(
        bundle.unpack_bundle(bundle.pack_bundle(value), back.bundle), value
    )


def test_describe_value_does_not_pickle_a_bundle(monkeypatch):
    from lzy_amd.channels import transport

    def boom(_):
        raise AssertionError("bundle was pickled")

    monkeypatch.setattr(transport, "pickle_value", boom)
    assert describe_value("e", {"w": _big()}).kind == KIND_BUNDLE


def test_channel_bundles_off_gives_bytes(monkeypatch):
    value = {"w": _big()}
    try:
        Config.reset(channel_bundles=False)
        assert describe_value("e", value).kind == KIND_BYTES
    finally:
        Config.reset()
    assert describe_value("e", value).kind == KIND_BUNDLE
    monkeypatch.setenv("LZY_CHANNEL_BUNDLES", "0")
    assert describe_value("e", value).kind == KIND_BYTES


def test_cpu_bundle_records_no_stream_event():
    from lzy_amd.runtime.streams import _device_of

    assert _device_of({"w": _big()}) is None
    assert _device_of({"a": 1}) is None


# ---------------------------------------------------------------------------
# transport over a real (1-process-per-rank) gloo pool
# ---------------------------------------------------------------------------

def _run_pool(tmp_path, extra_env):
    env = dict(os.environ)
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    env["MASTER_ADDR"] = "127.0.0.1"
    env["BUNDLE_DEVICE"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LZY_CHANNEL_BUNDLES"):
        env.pop(k, None)
    env.update(extra_env)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    res = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node=2",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            "tests/pool_script_bundle.py",
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=180,
    )
    if res.returncode != 0:
        print("STDOUT:", res.stdout[-4000:])
        print("STDERR:", res.stderr[-4000:])
    assert res.returncode == 0
    assert "BUNDLE-SCRIPT-OK" in res.stdout


def test_pool_two_ranks_bundle(tmp_path):
    _run_pool(tmp_path, {"BUNDLE_EXPECT": "bundle"})


def test_pool_two_ranks_bundles_off_is_the_parent_path(tmp_path):
    _run_pool(tmp_path, {"BUNDLE_EXPECT": "bytes", "LZY_CHANNEL_BUNDLES": "0"})
