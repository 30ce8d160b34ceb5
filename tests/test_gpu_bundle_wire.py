"""The segmented copy-or-codec kernel (ops.pack_tensors_wire /
unpack_tensors_wire) on MI355X (gfx950), and a wired tensor bundle carried
between two pool ranks on one GPU.

Yardsticks, none of them the code under test: a wired segment is held byte
for byte to the existing single-tensor kernel ``ops.mx8_pack`` and to the
torch codec; raw segments, gaps and the whole decode direction are held
byte for byte to the torch twins run on the CPU.  Host-side parts:
tests/test_bundle_wire.py.
"""
import os
import random
import socket
import subprocess
import sys
from contextlib import contextmanager
from pathlib import Path

import pytest
import torch

from lzy_amd import ops
from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch
from lzy_amd.exceptions import NativeExtensionMissing
from mxwire_util import assert_wire_equal, check_special_decode, special_vector

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROOT = Path(__file__).resolve().parent.parent
E = ops.SEGCODEC_TILE_ELEMS
T = ops.SEGCOPY_TILE
NUMELS = [1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049,
          E - 1, E, E + 1, 2 * E + 37]
RAW_SIZES = [0, 1, 2, 15, 16, 17, 127, 128, 129, T - 1, T, T + 1, 2 * T + 3]
RAW_DTYPES = [torch.bool, torch.uint8, torch.int64, torch.bfloat16,
              torch.float16, torch.float32, torch.float64, torch.float8_e4m3fn]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
MAGS = [1e-4, 1.0, 3e3]


def _input(n, dtype, seed=0):
    """CPU tensor whose three thirds sit at the three magnitudes."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(n, generator=g)
    mag = torch.tensor(MAGS)[(torch.arange(n) * 3) // max(n, 1)]
    return (x * mag).to(dtype)


def _raw_leaf(nbytes, dtype, g):
    if dtype is torch.bool:
        return torch.rand(nbytes, generator=g) > 0.5
    raw = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)
    return raw.view(dtype)


def _raw_leaves(sizes, g):
    """One raw leaf per byte length, every dtype of RAW_DTYPES used."""
    wide = {0: torch.int64, 16: torch.float32, 128: torch.float64,
            T: torch.bfloat16, 2: torch.float16}
    narrow = [torch.bool, torch.uint8, torch.float8_e4m3fn]
    return [_raw_leaf(n, wide.get(n, narrow[j % 3]), g)
            for j, n in enumerate(sizes)]


def _interleaved(dtype, seed):
    """Coded leaves of every size in NUMELS with raw leaves of every byte
    length in RAW_SIZES between them; (cpu leaves, wired flags)."""
    g = torch.Generator().manual_seed(seed)
    sizes = list(RAW_SIZES)
    random.Random(seed).shuffle(sizes)
    raw = _raw_leaves(sizes, g)
    assert {t.dtype for t in raw} == set(RAW_DTYPES)
    leaves, wired = [], []
    for j, n in enumerate(NUMELS):
        leaves.append(_input(n, dtype, seed=n))
        wired.append(True)
        if j < len(raw):
            leaves.append(raw[j])
            wired.append(False)
    return leaves, wired


_CASES = {}


def _case(dtype):
    """The interleaved leaves of ``dtype`` and their CPU references,
    computed once and shared (never modified)."""
    if dtype not in _CASES:
        leaves, wired = _interleaved(dtype, 21 + DTYPES.index(dtype))
        wire, woffs = ops.pack_tensors_wire_torch(leaves, wired)
        exact, offs = ops.unpack_tensors_wire_torch(
            wire, wired, [t.shape for t in leaves], [t.dtype for t in leaves])
        _CASES[dtype] = (leaves, wired, wire, woffs, exact, offs)
    return _CASES[dtype]


@contextmanager
def _capped(k):
    lib = ops._require_native()
    lib.lz_set_max_blocks(k)
    try:
        yield
    finally:
        lib.lz_set_max_blocks(0)


def _check_payload(x_cpu, got, want):
    """A kernel-packed segment against the torch codec's, byte for byte."""
    assert_wire_equal(x_cpu, got, want, f"wired segment n={x_cpu.numel()}")


def _check_encoded(leaves, wired, got, want, offs):
    """``got``: the kernel's wire buffer (CPU copy); ``want``: the torch
    twin's.  Wired segments against ops.mx8_pack and the twin; every other
    byte (raw segments, gaps) against the twin, exactly."""
    assert got.numel() == want.numel()
    other = torch.ones(got.numel(), dtype=torch.bool)
    for t, w, off in zip(leaves, wired, offs):
        if not w:
            continue
        n = ops.mx8_nbytes(t.numel())
        seg = got[off: off + n]
        assert torch.equal(seg, ops.mx8_pack(t.cuda()).cpu()), t.numel()
        _check_payload(t, seg, want[off: off + n])
        other[off: off + n] = False
    assert torch.equal(got[other], want[other])


# ---------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_encode_matches_mx8_pack_and_the_twin(dtype):
    leaves, wired, want, woffs, _, _ = _case(dtype)
    # a dirty out= proves every byte is written, not inherited
    out = torch.full((want.numel(),), 0xAB, dtype=torch.uint8, device="cuda")
    buf, offs = ops.pack_tensors_wire([t.cuda() for t in leaves], wired, out=out)
    assert buf is out and offs == woffs
    _check_encoded(leaves, wired, buf.cpu(), want, woffs)
    buf2, offs2 = ops.pack_tensors_wire([t.cuda() for t in leaves], wired)
    assert offs2 == woffs and buf2.data_ptr() % 128 == 0
    assert torch.equal(buf2, buf)  # deterministic


@requires_gpu
def test_special_values_as_a_wired_leaf():
    v = special_vector()
    filler = torch.arange(40, dtype=torch.int64)
    buf, offs = ops.pack_tensors_wire([filler.cuda(), v.cuda()], [False, True])
    host = buf.cpu()
    seg = host[offs[1]: offs[1] + ops.mx8_nbytes(128)]
    assert seg[128:].tolist() == [0, 119, 120, 247]
    check_special_decode(seg[128:], mx8_unpack_torch(seg, 128, torch.float32))
    exact, eoffs = ops.unpack_tensors_wire(
        buf, [False, True], [(40,), (128,)], [torch.int64, torch.float32])
    got = ops.unpack_tensors(exact, eoffs, [(40,), (128,)],
                             [torch.int64, torch.float32])
    check_special_decode(seg[128:], got[1])
    assert torch.equal(got[0].cpu(), filler)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_decode_matches_the_twin_exactly(dtype):
    leaves, wired, wire, _, want, want_offs = _case(dtype)
    out = torch.full((want.numel(),), 0xAB, dtype=torch.uint8, device="cuda")
    buf, offs = ops.unpack_tensors_wire(
        wire.cuda(), wired, [t.shape for t in leaves],
        [t.dtype for t in leaves], out=out)
    assert buf is out and offs == want_offs
    assert torch.equal(buf.cpu(), want)
    # the twin's buffer is pack_tensors_torch of the torch-decoded leaves
    dec = [mx8_unpack_torch(mx8_pack_torch(t), t.shape, t.dtype) if w else t
           for t, w in zip(leaves, wired)]
    assert torch.equal(ops.pack_tensors_torch(dec)[0], want)
    views = ops.unpack_tensors(buf, offs, [t.shape for t in leaves],
                               [t.dtype for t in leaves])
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1


# ---------------------------------------------------------------------------
# misaligned sources
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_misaligned_wired_sources_blind_to_neighbours(dtype):
    """Wired sources that are views 1, 3 and 7 elements into their
    allocation: the guarded per-element path gives the bytes of the aligned
    run, whatever surrounds the sources."""
    isz = torch.empty(0, dtype=dtype).element_size()
    payload = [_input(n, dtype, seed=70 + k)
               for k, n in enumerate((E + 5, 2 * E + 3, 37))]
    wired = [True, True, True]
    aligned, _ = ops.pack_tensors_wire([p.cuda() for p in payload], wired)
    results = []
    for sentinel in (0x11, 0xEE):
        leaves = []
        for k, p in zip((1, 3, 7), payload):
            alloc = torch.full(((k + p.numel() + 9) * isz,), sentinel,
                               dtype=torch.uint8, device="cuda").view(dtype)
            alloc[k: k + p.numel()] = p.cuda()
            leaf = alloc[k: k + p.numel()]
            assert leaf.data_ptr() % 16 == (k * isz) % 16 != 0
            leaves.append(leaf)
        results.append(ops.pack_tensors_wire(leaves, wired)[0])
    assert torch.equal(results[0], aligned)
    assert torch.equal(results[1], aligned)


# ---------------------------------------------------------------------------
# nothing written outside
# ---------------------------------------------------------------------------

@requires_gpu
def test_both_directions_write_nothing_outside_out():
    leaves, wired, wire, woffs, exact, _ = _case(torch.bfloat16)
    shapes, dtypes = [t.shape for t in leaves], [t.dtype for t in leaves]
    big = torch.full((wire.numel() + 512,), 0xCD, dtype=torch.uint8, device="cuda")
    out = big[256: 256 + wire.numel()]
    ops.pack_tensors_wire([t.cuda() for t in leaves], wired, out=out)
    host = big.cpu()
    _check_encoded(leaves, wired, host[256: 256 + wire.numel()], wire, woffs)
    assert (host[:256] == 0xCD).all() and (host[256 + wire.numel():] == 0xCD).all()

    big = torch.full((exact.numel() + 512,), 0xCD, dtype=torch.uint8, device="cuda")
    out = big[256: 256 + exact.numel()]
    src = wire.cuda()
    ops.unpack_tensors_wire(src, wired, shapes, dtypes, out=out)
    host = big.cpu()
    assert torch.equal(host[256: 256 + exact.numel()], exact)
    assert (host[:256] == 0xCD).all() and (host[256 + exact.numel():] == 0xCD).all()
    assert torch.equal(src.cpu(), wire)  # the source is only read


# ---------------------------------------------------------------------------
# grid-stride
# ---------------------------------------------------------------------------

@requires_gpu
def test_grid_stride_two_blocks_300_segments():
    rng = random.Random(9)
    g = torch.Generator().manual_seed(19)
    pool = torch.randint(0, 256, (3 * T + 64,), generator=g, dtype=torch.uint8)
    leaves, wired = [], []
    for j in range(300):
        kind = rng.randrange(4)
        if kind == 3:
            n = rng.randint(1, 3 * T)
            s = rng.randint(0, 3 * T + 64 - n)
            leaves.append(pool[s: s + n])
        else:
            leaves.append(_input(rng.randint(1, 3 * E), DTYPES[kind], seed=j))
        wired.append(kind != 3)
    shapes, dtypes = [t.shape for t in leaves], [t.dtype for t in leaves]
    want, woffs = ops.pack_tensors_wire_torch(leaves, wired)
    exact, eoffs = ops.unpack_tensors_wire_torch(want, wired, shapes, dtypes)
    counts = [t.numel() for t in leaves]
    modes = [ops.SEGCODEC_ENCODE if w else ops.SEGCODEC_RAW for w in wired]
    _, ntiles = ops.segcodec_table([0] * 300, [0] * 300, counts, modes)
    assert ntiles > 300  # every block of the capped grid walks many tiles
    dev = [t.cuda() for t in leaves]
    wire_dev = want.cuda()
    with _capped(2):
        buf, offs = ops.pack_tensors_wire(dev, wired)
        dec, doffs = ops.unpack_tensors_wire(wire_dev, wired, shapes, dtypes)
        torch.cuda.synchronize()
    assert offs == woffs and doffs == eoffs
    _check_encoded(leaves, wired, buf.cpu(), want, woffs)
    assert torch.equal(dec.cpu(), exact)


# ---------------------------------------------------------------------------
# argument checks, stale library
# ---------------------------------------------------------------------------

@requires_gpu
def test_argument_checks():
    a = torch.zeros(100, device="cuda")
    total = ops.segcopy_nbytes([ops.mx8_nbytes(100)], 128)
    with pytest.raises(ValueError):  # a wired int leaf
        ops.pack_tensors_wire([torch.arange(100, device="cuda")], [True])
    with pytest.raises(ValueError):  # a CPU leaf
        ops.pack_tensors_wire([a, torch.zeros(4)], [True, False])
    with pytest.raises(ValueError):  # flags of another length
        ops.pack_tensors_wire([a], [True, False])
    with pytest.raises(ValueError):  # wrong out size
        ops.pack_tensors_wire([a], [True], out=torch.empty(
            total + 128, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):  # out not aligned to the layout
        ops.pack_tensors_wire([a], [True], out=torch.empty(
            total + 1, dtype=torch.uint8, device="cuda")[1:])
    with pytest.raises(ValueError):  # CPU out
        ops.pack_tensors_wire([a], [True],
                              out=torch.empty(total, dtype=torch.uint8))
    buf, _ = ops.pack_tensors_wire([a], [True])
    assert buf.numel() == total
    etotal = ops.segcopy_nbytes([400], 128)
    with pytest.raises(ValueError):  # decode: a CPU wire buffer
        ops.unpack_tensors_wire(buf.cpu(), [True], [(100,)], [torch.float32])
    with pytest.raises(ValueError):  # decode: wrong wire size
        ops.unpack_tensors_wire(buf[:-128], [True], [(100,)], [torch.float32])
    with pytest.raises(ValueError):  # decode: a wired int leaf
        ops.unpack_tensors_wire(buf, [True], [(100,)], [torch.int32])
    with pytest.raises(ValueError):  # decode: wrong out size
        ops.unpack_tensors_wire(buf, [True], [(100,)], [torch.float32],
                                out=torch.empty(etotal + 128, dtype=torch.uint8,
                                                device="cuda"))
    with pytest.raises(ValueError):  # decode: misaligned out
        ops.unpack_tensors_wire(buf, [True], [(100,)], [torch.float32],
                                out=torch.empty(etotal + 1, dtype=torch.uint8,
                                                device="cuda")[1:])
    with pytest.raises(ValueError):  # decode: CPU out
        ops.unpack_tensors_wire(buf, [True], [(100,)], [torch.float32],
                                out=torch.empty(etotal, dtype=torch.uint8))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):  # out on another device
            ops.pack_tensors_wire([a], [True], out=torch.empty(
                total, dtype=torch.uint8, device="cuda:1"))


@requires_gpu
def test_stale_library_raises_never_falls_back(monkeypatch):
    from lzy_amd.channels import bundle

    a = torch.zeros(100, device="cuda")
    buf, _ = ops.pack_tensors_wire([a], [True])
    value = {"w": torch.zeros(70000, device="cuda")}
    spec = bundle.bundle_spec(value)
    wire = bundle.pack_bundle(value, wire="mxfp8")
    monkeypatch.setattr(ops, "_SEGCODEC", False)
    with pytest.raises(NativeExtensionMissing):
        ops.pack_tensors_wire([a], [True])
    with pytest.raises(NativeExtensionMissing):
        ops.unpack_tensors_wire(buf, [True], [(100,)], [torch.float32])
    with pytest.raises(NativeExtensionMissing):
        bundle.pack_bundle(value, wire="mxfp8")  # no torch codec on a device
    with pytest.raises(NativeExtensionMissing):
        bundle.unpack_bundle_wire(wire, spec, "mxfp8")
    # the exact path and the other exports are untouched
    assert ops.pack_tensors([a])[0].numel() == 512
    assert bundle.pack_bundle(value).numel() == spec["nbytes"]
    assert ops.mx8_pack(a).numel() == ops.mx8_nbytes(100)


# ---------------------------------------------------------------------------
# end to end: two ranks, one GPU
# ---------------------------------------------------------------------------

@requires_gpu
def test_wired_bundle_two_ranks_one_gpu(tmp_path):
    """tests/pool_script_bundle_wire.py with device leaves, both ranks on one
    GPU (the host-staged path: kernel encode before staging, kernel decode on
    arrival).  The script holds the checks: received leaves on the
    consumer's current device and views of one allocation, wired leaves
    within the docs/mxwire.md bound, exact leaves bit-equal, meta kind
    ``bundle``, ``lzy_transfers_bundle_wired >= 1``."""
    env = dict(os.environ)
    env["BUNDLE_DEVICE"] = "cuda"
    env["LZY_BUNDLE_WIRE_CAST"] = "mxfp8"
    env["HIP_VISIBLE_DEVICES"] = "0"  # both ranks share one GPU
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LZY_CHANNEL_BUNDLES"):
        env.pop(k, None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    res = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node=2",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            "tests/pool_script_bundle_wire.py",
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=240,
    )
    print("STDOUT:", res.stdout[-4000:])
    if res.returncode != 0:
        print("STDERR:", res.stderr[-4000:])
    assert res.returncode == 0
    assert "BUNDLE-WIRE-SCRIPT-OK" in res.stdout
