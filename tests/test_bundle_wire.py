"""Tensor bundles on the MXFP8 wire (``bundle_wire_cast``), host side: the
wire layout, the table of the segmented copy-or-codec kernel, the torch
codec (the kernel's oracle), the driver's config check, a two-rank gloo pool
(tests/pool_script_bundle_wire.py) and a chunked, resumed transport
(tests/bundle_wire_transport_script.py).  The kernel itself:
tests/test_gpu_bundle_wire.py.
"""
import os
import socket
import subprocess
import sys
from collections import OrderedDict
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from lzy_amd import ops
from lzy_amd.channels import bundle, transport
from lzy_amd.channels.mxwire import mx8_nbytes, mx8_pack_torch, mx8_unpack_torch
from lzy_amd.channels.transport import KIND_BUNDLE, describe_value
from lzy_amd.config import Config
from mxwire_util import assert_within_bound

ROOT = Path(__file__).resolve().parent.parent
T = ops.SEGCOPY_TILE
E = ops.SEGCODEC_TILE_ELEMS
MIN = transport._WIRE_MIN_ELEMS


def _up(n, a=128):
    return (n + a - 1) // a * a


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------

def test_threshold_is_the_projects():
    assert MIN == 65536 and E % 2048 == 0


def test_wire_layout_against_hand_arithmetic():
    value = OrderedDict(
        w=torch.zeros(300, 257),                        # 77100 f32: wired
        b=torch.zeros(65536 + 7, dtype=torch.bfloat16),  # wired
        small=torch.zeros(200),                         # float, too small
        steps=torch.zeros(70000, dtype=torch.int64),    # large, not float
        h=torch.zeros(65536, dtype=torch.float16),      # wired, at the edge
        mask=torch.zeros(33, dtype=torch.bool),
    )
    spec = bundle.bundle_spec(value)
    lay = bundle.bundle_wire_layout(spec, "mxfp8")
    assert lay["wired"] == [True, True, False, False, True, False]
    # 33 bytes per block of 32 elements, each segment at a multiple of 128
    s0 = 33 * ((77100 + 31) // 32)   # 2410 blocks -> 79530
    s1 = 33 * ((65543 + 31) // 32)   # 2049 blocks -> 67617
    s4 = 33 * 2048                   # 67584
    assert (s0, s1, s4) == (79530, 67617, 67584)
    assert s0 == mx8_nbytes(77100) == ops.mx8_nbytes(77100)
    o0 = 0
    o1 = _up(o0 + s0)
    o2 = _up(o1 + s1)
    o3 = _up(o2 + 200 * 4)
    o4 = _up(o3 + 70000 * 8)
    o5 = _up(o4 + s4)
    assert lay["offsets"] == [o0, o1, o2, o3, o4, o5]
    assert lay["wire_nbytes"] == _up(o5 + 33)
    sizes = [s0, s1, 800, 560000, s4, 33]
    assert (lay["offsets"], lay["wire_nbytes"]) == ops.segcopy_layout(sizes, 128)
    assert lay["wire_nbytes"] < spec["nbytes"]
    assert lay == bundle.bundle_wire_layout(spec, "mxfp8")  # deterministic


def test_wire_layout_none_when_off_or_nothing_wired():
    big = {"w": torch.zeros(70000)}
    assert bundle.bundle_wire_layout(bundle.bundle_spec(big), "") is None
    small = {"a": torch.zeros(65535), "i": torch.zeros(70000, dtype=torch.int64),
             "d": torch.zeros(70000, dtype=torch.float64)}
    assert bundle.bundle_wire_layout(bundle.bundle_spec(small), "mxfp8") is None
    with pytest.raises(ValueError):
        bundle.bundle_wire_layout(bundle.bundle_spec(big), "fp8")
    # unwired: pack_bundle(value, wire) is the exact buffer, byte for byte
    g = torch.Generator().manual_seed(1)
    v = {"a": torch.randn(65535, generator=g)}
    assert torch.equal(bundle.pack_bundle(v, wire="mxfp8"), bundle.pack_bundle(v))
    assert torch.equal(bundle.pack_bundle(v, wire=""), bundle.pack_bundle(v))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_threshold_edge(dtype):
    below = bundle.bundle_spec({"w": torch.zeros(MIN - 1, dtype=dtype)})
    at = bundle.bundle_spec({"w": torch.zeros(MIN, dtype=dtype)})
    assert bundle.bundle_wire_layout(below, "mxfp8") is None
    lay = bundle.bundle_wire_layout(at, "mxfp8")
    assert lay == {"wired": [True], "offsets": [0],
                   "wire_nbytes": _up(33 * (MIN // 32))}


# ---------------------------------------------------------------------------
# the kernel's table, against brute force
# ---------------------------------------------------------------------------

_RAW, _ENC, _DEC = ops.SEGCODEC_RAW, ops.SEGCODEC_ENCODE, ops.SEGCODEC_DECODE
_TABLE_CASES = {
    "mixed": ([0, 1, T - 1, T, T + 1, 2 * T + 3, 0, 1, 31, 32, E - 1, E, E + 1,
               2 * E + 37, 5, 3 * E],
              [_RAW] * 6 + [_ENC, _ENC + 1, _ENC + 2, _DEC, _DEC + 1, _DEC + 2,
                            _ENC, _DEC, _RAW, _ENC + 2]),
    "all-empty": ([0, 0, 0], [_RAW, _ENC, _DEC + 2]),
    "none": ([], []),
    "coded-only": ([5 * E, 1], [_DEC, _ENC]),
}


@pytest.mark.parametrize("case", list(_TABLE_CASES), ids=list(_TABLE_CASES))
def test_segcodec_table_matches_tile_enumeration(case):
    counts, modes = _TABLE_CASES[case]
    n = len(counts)
    srcs = [1000 + 7 * i for i in range(n)]
    dsts = [5000 + 128 * i for i in range(n)]
    table, ntiles = ops.segcodec_table(srcs, dsts, counts, modes)
    assert len(table) == 5 * n + 1
    assert table[:n] == srcs and table[n:2 * n] == dsts
    assert table[2 * n:3 * n] == list(counts)
    assert table[3 * n:4 * n] == list(modes)
    tile_start = table[4 * n:]
    # brute force: walk every segment in steps of its own tile unit
    tiles = []  # (segment, offset in the segment's unit, length)
    for s, (cnt, m) in enumerate(zip(counts, modes)):
        per = T if m == _RAW else E
        off = 0
        while off < cnt:
            tiles.append((s, off, min(per, cnt - off)))
            off += per
    assert ntiles == len(tiles)
    assert tile_start[0] == 0 and tile_start[-1] == ntiles
    for t, (s, off, ln) in enumerate(tiles):
        lo = max(i for i in range(n) if tile_start[i] <= t)  # the kernel's search
        per = T if modes[lo] == _RAW else E
        assert lo == s
        assert (t - tile_start[lo]) * per == off
        assert min(per, counts[lo] - off) == ln
    covered = [sum(ln for s, _, ln in tiles if s == i) for i in range(n)]
    assert covered == list(counts)


def test_segcodec_table_rejects_bad_input():
    with pytest.raises(ValueError):
        ops.segcodec_table([0], [0], [4], [7])
    with pytest.raises(ValueError):
        ops.segcodec_table([0], [0], [-1], [0])
    with pytest.raises(ValueError):
        ops.segcodec_table([0], [0, 1], [4], [0])


# ---------------------------------------------------------------------------
# torch codec
# ---------------------------------------------------------------------------

def _value(seed=7):
    g = torch.Generator().manual_seed(seed)
    shared = torch.randn(300, 257, generator=g)
    inner = OrderedDict()
    inner["z_first"] = shared
    inner["bf16"] = (torch.randn(MIN + 7, generator=g) * 1e-4).to(torch.bfloat16)
    inner["f16"] = (torch.randn(MIN, generator=g) * 30).to(torch.float16)
    inner["bias"] = torch.randn(200, generator=g)
    inner._metadata = OrderedDict([("", {"version": 2})])
    value = OrderedDict()
    value["model"] = inner
    value["rest"] = (
        torch.arange(70000, dtype=torch.int64),
        torch.rand(33, generator=g) > 0.5,
        torch.tensor(2.5, dtype=torch.float64),
        torch.empty(0, 4),
        shared,
        "a string", 12, None, 2.5,
    )
    value["epoch"] = 4
    return value


def _leaves(value):
    m, r = value["model"], value["rest"]
    return [m["z_first"], m["bf16"], m["f16"], m["bias"], r[0], r[1], r[2], r[3]]


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def test_torch_codec_round_trip_of_a_nested_container():
    value = _value()
    spec = bundle.bundle_spec(value)
    lay = bundle.bundle_wire_layout(spec, "mxfp8")
    assert lay["wired"] == [True, True, True] + [False] * 5
    wire = bundle.pack_bundle(value, wire="mxfp8")
    assert wire.dtype == torch.uint8 and wire.numel() == lay["wire_nbytes"]
    assert torch.equal(wire, bundle.pack_bundle(_value(), wire="mxfp8"))
    src = _leaves(value)
    # a wired segment is an ordinary MXFP8 buffer; gaps are zero
    mask = torch.ones(wire.numel(), dtype=torch.bool)
    for t, w, off in zip(src, lay["wired"], lay["offsets"]):
        n = mx8_nbytes(t.numel()) if w else t.numel() * t.element_size()
        want = mx8_pack_torch(t) if w else _bytes(t)
        assert torch.equal(wire[off: off + n], want)
        mask[off: off + n] = False
    assert mask.any() and not wire[mask].any()

    got = bundle.unpack_bundle_wire(wire, spec, "mxfp8")
    assert type(got) is OrderedDict and list(got) == ["model", "rest", "epoch"]
    assert type(got["model"]) is OrderedDict and type(got["rest"]) is tuple
    assert list(got["model"]) == ["z_first", "bf16", "f16", "bias"]
    assert got["model"]._metadata == value["model"]._metadata
    assert got["rest"][5:] == ("a string", 12, None, 2.5) and got["epoch"] == 4
    assert got["rest"][4] is got["model"]["z_first"]  # one object, one segment
    dec = _leaves(got)
    for g, t, w in zip(dec, src, lay["wired"]):
        assert g.dtype == t.dtype and g.shape == t.shape
        if w:
            want = mx8_unpack_torch(mx8_pack_torch(t), t.shape, t.dtype)
            assert torch.equal(_bytes(g), _bytes(want))
            assert_within_bound(g, t, t.dtype)
        else:
            assert torch.equal(_bytes(g), _bytes(t))
    # views of one allocation, which is the exact-layout buffer
    ptrs = {g.untyped_storage().data_ptr() for g in dec}
    assert len(ptrs) == 1
    exact, offs = ops.pack_tensors_torch(dec)
    assert offs == [s[0] for s in spec["segs"]]
    assert exact.numel() == spec["nbytes"]
    root = dec[0]
    whole = torch.empty(0, dtype=torch.uint8).set_(
        root.untyped_storage(), 0, (spec["nbytes"],))
    assert torch.equal(whole, exact)
    # the ops twins agree with the bundle codec
    buf, offs2 = ops.unpack_tensors_wire_torch(
        wire, lay["wired"], [t.shape for t in src], [t.dtype for t in src])
    assert offs2 == offs and torch.equal(buf, exact)
    out = torch.full_like(wire, 0xAB)
    assert ops.pack_tensors_wire_torch(src, lay["wired"], out=out)[0] is out
    assert torch.equal(out, wire)


def test_torch_twins_reject_bad_arguments():
    with pytest.raises(ValueError):  # a wired int leaf
        ops.pack_tensors_wire_torch([torch.arange(100)], [True])
    with pytest.raises(ValueError):
        ops.pack_tensors_wire_torch([torch.zeros(4)], [True, False])
    with pytest.raises(ValueError):  # wrong wire size
        ops.unpack_tensors_wire_torch(torch.zeros(128, dtype=torch.uint8), [True],
                                      [(100,)], [torch.float32])
    with pytest.raises(ValueError):  # device entry points take device leaves
        ops.pack_tensors_wire([torch.zeros(100)], [True])
    spec = bundle.bundle_spec({"w": torch.zeros(MIN)})
    with pytest.raises(ValueError):
        bundle.unpack_bundle_wire(torch.zeros(128, dtype=torch.uint8), spec, "mxfp8")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16],
                         ids=["f32", "bf16", "f16"])
def test_second_hop_reencodes_to_the_same_values(dtype):
    """A receiver that serves a later transfer re-encodes decoded leaves:
    decode(encode(decode(encode(x)))) == decode(encode(x)) bit for bit on
    these inputs (observed, not proven; the wire bytes may differ)."""
    tiny = 1e-6 if dtype is torch.float16 else 1e-30
    for k, mag in enumerate((1.0, 1e-4, 3e3, tiny)):
        g = torch.Generator().manual_seed(40 + k)
        x = (torch.randn(70000, generator=g) * mag).to(dtype)
        value = {"x": x, "step": k}
        spec = bundle.bundle_spec(value)
        hop1 = bundle.unpack_bundle_wire(
            bundle.pack_bundle(value, wire="mxfp8"), spec, "mxfp8")
        hop2 = bundle.unpack_bundle_wire(
            bundle.pack_bundle(hop1, wire="mxfp8"), spec, "mxfp8")
        assert torch.equal(_bytes(hop2["x"]), _bytes(hop1["x"])), (dtype, mag)
        assert hop2["step"] == k


# ---------------------------------------------------------------------------
# meta, config, driver
# ---------------------------------------------------------------------------

def test_entry_meta_wire_dict_of_a_bundle_is_unchanged():
    meta = describe_value("e", _value())
    assert meta.kind == KIND_BUNDLE
    wire = meta.to_wire()
    assert set(wire) == {"entry_id", "kind", "shape", "dtype", "device_type",
                         "nbytes", "bundle"}
    assert wire["nbytes"] == meta.bundle["nbytes"]
    assert set(wire["bundle"]) == {"skeleton", "segs", "nbytes"}


def test_config_bundle_wire_cast(monkeypatch):
    monkeypatch.delenv("LZY_BUNDLE_WIRE_CAST", raising=False)
    try:
        assert Config.reset().bundle_wire_cast == ""
        monkeypatch.setenv("LZY_BUNDLE_WIRE_CAST", "mxfp8")
        cfg = Config.reset()
        assert cfg.bundle_wire_cast == "mxfp8"
        assert cfg.channel_wire_cast == "" and cfg.stream_wire_cast == ""
    finally:
        monkeypatch.delenv("LZY_BUNDLE_WIRE_CAST", raising=False)
        Config.reset()


def test_scheduler_rejects_bad_bundle_wire_cast():
    from lzy_amd.runtime.pool import _DriverScheduler

    try:
        Config.reset(bundle_wire_cast="fp8")
        with pytest.raises(ValueError, match="bundle_wire_cast"):
            _DriverScheduler(SimpleNamespace(world=1), SimpleNamespace(), [], None)
    finally:
        Config.reset()


def test_driver_marks_both_items_and_counts_wire_bytes():
    from lzy_amd.runtime.pool import _wire_bundle_items
    from lzy_amd.utils.metrics import METRICS

    meta = describe_value("e", _value())
    before = meta.to_wire()
    n0 = METRICS.counter_value("lzy_transfers_bundle_wired")
    send, recv = {"entry": "e"}, {"entry": "e"}
    nbytes = _wire_bundle_items(meta, "mxfp8", send, recv)
    lay = bundle.bundle_wire_layout(meta.bundle, "mxfp8")
    assert send["wire"] == recv["wire"] == "mxfp8"
    assert nbytes == lay["wire_nbytes"] < meta.nbytes
    assert METRICS.counter_value("lzy_transfers_bundle_wired") == n0 + 1
    assert meta.to_wire() == before
    # off, an unwirable bundle, or another kind: untouched items, exact bytes
    for m, wire in ((meta, ""),
                    (describe_value("s", {"w": torch.zeros(20000)}), "mxfp8"),
                    (describe_value("t", torch.zeros(MIN)), "mxfp8")):
        send, recv = {}, {}
        assert _wire_bundle_items(m, wire, send, recv) == m.nbytes
        assert send == {} and recv == {}
    assert METRICS.counter_value("lzy_transfers_bundle_wired") == n0 + 1


# ---------------------------------------------------------------------------
# gloo runs
# ---------------------------------------------------------------------------

def _torchrun(script, tmp_path, extra_env, marker, timeout=180):
    env = dict(os.environ)
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    env["MASTER_ADDR"] = "127.0.0.1"
    env["BUNDLE_DEVICE"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LZY_CHANNEL_BUNDLES", "LZY_BUNDLE_WIRE_CAST"):
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
            script,
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout,
    )
    if res.returncode != 0:
        print("STDOUT:", res.stdout[-4000:])
        print("STDERR:", res.stderr[-4000:])
    assert res.returncode == 0
    assert marker in res.stdout


def test_pool_two_ranks_bundle_wired(tmp_path):
    _torchrun("tests/pool_script_bundle_wire.py", tmp_path,
              {"LZY_BUNDLE_WIRE_CAST": "mxfp8"}, "BUNDLE-WIRE-SCRIPT-OK")


def test_pool_two_ranks_key_unset_is_bit_exact(tmp_path):
    _torchrun("tests/pool_script_bundle_wire.py", tmp_path, {},
              "BUNDLE-WIRE-SCRIPT-OK")


def test_wired_bundle_chunked_and_resumed(tmp_path):
    _torchrun("tests/bundle_wire_transport_script.py", tmp_path, {},
              "BUNDLE-WIRE-TRANSPORT-OK")
