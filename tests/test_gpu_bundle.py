"""The segmented-copy kernel (ops.pack_tensors / unpack_tensors) against its
torch oracle ``pack_tensors_torch``, byte for byte, and a tensor bundle
carried between two pool ranks on one GPU.  Host-side parts:
tests/test_bundle.py.
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
from lzy_amd.exceptions import NativeExtensionMissing

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROOT = Path(__file__).resolve().parent.parent
T = ops.SEGCOPY_TILE
SIZES = [0, 1, 2, 15, 16, 17, 127, 128, 129, T - 1, T, T + 1, 2 * T + 3]
DTYPES = [torch.bool, torch.uint8, torch.int64, torch.bfloat16, torch.float16,
          torch.float32, torch.float64, torch.float8_e4m3fn]


def _itemsize(dt):
    return torch.empty(0, dtype=dt).element_size()


def _leaf(nbytes, dtype, g):
    """A CPU leaf of exactly ``nbytes`` bytes of ``dtype`` from random bytes."""
    if dtype is torch.bool:
        return torch.rand(nbytes, generator=g) > 0.5
    raw = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)
    return raw.view(dtype)


def _mixed_leaves(sizes, g):
    """One leaf per byte length, every dtype of DTYPES used: the lengths
    every itemsize divides take the wide types, the odd ones cycle through
    the one-byte types."""
    wide = {0: torch.int64, 16: torch.float32, 128: torch.float64,
            T: torch.bfloat16, 2: torch.float16}
    narrow = [torch.bool, torch.uint8, torch.float8_e4m3fn]
    return [_leaf(n, wide.get(n, narrow[j % 3]), g)
            for j, n in enumerate(sizes)]


def _oracle(cpu_leaves, align=128):
    return ops.pack_tensors_torch(cpu_leaves, align=align)


@contextmanager
def _capped(k):
    lib = ops._require_native()
    lib.lz_set_max_blocks(k)
    try:
        yield
    finally:
        lib.lz_set_max_blocks(0)


# ---------------------------------------------------------------------------
# byte-exact pack
# ---------------------------------------------------------------------------

@requires_gpu
def test_pack_sizes_in_order_exact():
    g = torch.Generator().manual_seed(11)
    cpu = [_leaf(n, torch.uint8, g) for n in SIZES]
    want, want_offs = _oracle(cpu)
    # a dirty out= proves the pad is written, not inherited
    out = torch.full((want.numel(),), 0xAB, dtype=torch.uint8, device="cuda")
    buf, offs = ops.pack_tensors([t.cuda() for t in cpu], out=out)
    assert buf is out and offs == want_offs
    assert torch.equal(buf.cpu(), want)
    buf2, offs2 = ops.pack_tensors([t.cuda() for t in cpu])
    assert offs2 == want_offs and buf2.data_ptr() % 128 == 0
    assert torch.equal(buf2.cpu(), want)


@requires_gpu
def test_pack_sizes_shuffled_mixed_dtypes_exact():
    rng = random.Random(5)
    g = torch.Generator().manual_seed(12)
    sizes = list(SIZES)
    rng.shuffle(sizes)
    cpu = _mixed_leaves(sizes, g)
    assert {t.dtype for t in cpu} == set(DTYPES)
    want, want_offs = _oracle(cpu)
    out = torch.full((want.numel(),), 0xAB, dtype=torch.uint8, device="cuda")
    buf, offs = ops.pack_tensors([t.cuda() for t in cpu], out=out)
    assert offs == want_offs
    assert torch.equal(buf.cpu(), want)


@requires_gpu
def test_pack_noncontiguous_and_scalar_leaves():
    g = torch.Generator().manual_seed(13)
    cpu = [torch.randn(70, 50, generator=g).t(), torch.tensor(1.5),
           torch.empty(0, 3), torch.randn(9, generator=g)[::2]]
    want, _ = _oracle(cpu)
    buf, _ = ops.pack_tensors([t.cuda() for t in cpu])
    assert torch.equal(buf.cpu(), want)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16])
def test_misaligned_sources_exact_and_blind_to_neighbours(dtype):
    """Views starting 1, 3 and 7 elements into an allocation: 1 B-, 2 B- and
    6 B-aligned source addresses.  The output depends on the leaf bytes
    alone, whatever surrounds the sources."""
    g = torch.Generator().manual_seed(14)
    isz = _itemsize(dtype)
    numels = [(T + 5) // isz, 2 * T // isz + 3, 37]
    payload = [_leaf(n * isz, dtype, g) for n in numels]
    want, _ = _oracle(payload)
    results = []
    for sentinel in (0x11, 0xEE):
        leaves = []
        for k, p in zip((1, 3, 7), payload):
            alloc = torch.full(((k + p.numel() + 9) * isz,), sentinel,
                               dtype=torch.uint8, device="cuda").view(dtype)
            alloc[k: k + p.numel()] = p.cuda()
            leaf = alloc[k: k + p.numel()]
            assert leaf.data_ptr() % 16 == (k * isz) % 16
            leaves.append(leaf)
        buf, _ = ops.pack_tensors(leaves)
        results.append(buf.cpu())
    assert torch.equal(results[0], want)
    assert torch.equal(results[1], want)


# ---------------------------------------------------------------------------
# nothing written outside
# ---------------------------------------------------------------------------

@requires_gpu
def test_pack_writes_nothing_outside_out():
    g = torch.Generator().manual_seed(15)
    cpu = [_leaf(n, torch.uint8, g) for n in SIZES]
    want, _ = _oracle(cpu)
    total = want.numel()
    big = torch.full((total + 512,), 0xCD, dtype=torch.uint8, device="cuda")
    out = big[256: 256 + total]
    ops.pack_tensors([t.cuda() for t in cpu], out=out)
    host = big.cpu()
    assert torch.equal(host[256: 256 + total], want)
    assert (host[:256] == 0xCD).all() and (host[256 + total:] == 0xCD).all()


@requires_gpu
def test_scatter_exact_and_writes_nothing_outside():
    rng = random.Random(6)
    g = torch.Generator().manual_seed(16)
    sizes = list(SIZES)
    rng.shuffle(sizes)
    cpu = _mixed_leaves(sizes, g)
    packed, offs = _oracle(cpu)
    buf = packed.cuda()
    allocs, outs = [], []
    for i, t in enumerate(cpu):
        lead = (1, 3, 7)[i % 3]  # element offsets: misaligned destinations
        isz = t.element_size()
        alloc = torch.full(((lead + t.numel() + 5) * isz,), 0x5A,
                           dtype=torch.uint8, device="cuda")
        allocs.append((alloc, lead * isz, t.numel() * isz))
        outs.append(alloc.view(t.dtype)[lead: lead + t.numel()])
    got = ops.unpack_tensors(buf, offs, [t.shape for t in cpu],
                             [t.dtype for t in cpu], out=outs)
    assert all(a is b for a, b in zip(got, outs))
    for (alloc, lo, n), t in zip(allocs, cpu):
        host = alloc.cpu()
        assert torch.equal(host[lo: lo + n], t.reshape(-1).view(torch.uint8))
        # no pad in the scatter direction: both neighbours keep the sentinel
        assert (host[:lo] == 0x5A).all() and (host[lo + n:] == 0x5A).all()
    assert torch.equal(buf.cpu(), packed)  # the source is only read


# ---------------------------------------------------------------------------
# grid-stride
# ---------------------------------------------------------------------------

@requires_gpu
def test_grid_stride_two_blocks_300_segments():
    rng = random.Random(7)
    g = torch.Generator().manual_seed(17)
    sizes = [rng.randint(1, 3 * T) for _ in range(300)]
    pool = torch.randint(0, 256, (3 * T + 64,), generator=g, dtype=torch.uint8)
    starts = [rng.randint(0, 3 * T + 64 - n) for n in sizes]
    cpu = [pool[s: s + n] for s, n in zip(starts, sizes)]
    want, _ = _oracle(cpu)
    dev_pool = pool.cuda()
    leaves = [dev_pool[s: s + n] for s, n in zip(starts, sizes)]
    _, ntiles = ops.segcopy_table([0] * 300, [0] * 300, sizes)
    assert ntiles > 300  # every block of the capped grid walks many tiles
    with _capped(2):
        buf, _ = ops.pack_tensors(leaves)
        torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), want)


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------

@requires_gpu
def test_unpack_returns_views_of_the_buffer():
    g = torch.Generator().manual_seed(18)
    cpu = [torch.randn(33, 5, generator=g), torch.tensor(7, dtype=torch.int64),
           torch.randn(130, generator=g).to(torch.bfloat16), torch.empty(0, 2),
           torch.rand(19, generator=g) > 0.5]
    buf, offs = ops.pack_tensors([t.cuda() for t in cpu])
    leaves = ops.unpack_tensors(buf, offs, [t.shape for t in cpu],
                                [t.dtype for t in cpu])
    for leaf, t, off in zip(leaves, cpu, offs):
        assert leaf.is_cuda and leaf.dtype == t.dtype and leaf.shape == t.shape
        assert leaf.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        if t.numel():  # torch reports a null data_ptr for empty tensors
            assert leaf.data_ptr() == buf.data_ptr() + off
        assert torch.equal(leaf.cpu(), t)


# ---------------------------------------------------------------------------
# argument checks, stale library
# ---------------------------------------------------------------------------

@requires_gpu
def test_argument_checks():
    a = torch.zeros(100, device="cuda")
    total = ops.segcopy_nbytes([400], 128)
    with pytest.raises(ValueError):
        ops.pack_tensors([a, torch.zeros(4)])  # a CPU leaf
    with pytest.raises(ValueError):  # wrong out size
        ops.pack_tensors([a], out=torch.empty(total + 128, dtype=torch.uint8,
                                              device="cuda"))
    with pytest.raises(ValueError):  # non-contiguous out
        ops.pack_tensors([a], out=torch.empty(2 * total, dtype=torch.uint8,
                                              device="cuda")[::2])
    with pytest.raises(ValueError):  # CPU out
        ops.pack_tensors([a], out=torch.empty(total, dtype=torch.uint8))
    with pytest.raises(ValueError):  # out not aligned to the layout
        ops.pack_tensors([a], out=torch.empty(total + 1, dtype=torch.uint8,
                                              device="cuda")[1:])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):  # leaves on different devices
            ops.pack_tensors([a, torch.zeros(4, device="cuda:1")])
    buf, offs = ops.pack_tensors([a])
    with pytest.raises(ValueError):  # scatter: wrong out shape
        ops.unpack_tensors(buf, offs, [(100,)], [torch.float32],
                           out=[torch.empty(99, device="cuda")])
    with pytest.raises(ValueError):  # scatter: non-contiguous out
        ops.unpack_tensors(buf, offs, [(100,)], [torch.float32],
                           out=[torch.empty(200, device="cuda")[::2]])
    with pytest.raises(ValueError):  # scatter: CPU out
        ops.unpack_tensors(buf, offs, [(100,)], [torch.float32],
                           out=[torch.empty(100)])


@requires_gpu
def test_stale_library_raises_never_falls_back(monkeypatch):
    from lzy_amd.channels import bundle

    a = torch.zeros(100, device="cuda")
    buf, offs = ops.pack_tensors([a])
    value = {"w": torch.zeros(20000, device="cuda")}
    monkeypatch.setattr(ops, "_SEGCOPY", False)
    with pytest.raises(NativeExtensionMissing):
        ops.pack_tensors([a])
    with pytest.raises(NativeExtensionMissing):
        ops.unpack_tensors(buf, offs, [(100,)], [torch.float32],
                           out=[torch.empty(100, device="cuda")])
    with pytest.raises(NativeExtensionMissing):
        bundle.pack_bundle(value)  # the device dispatcher: no torch codec
    # views need no kernel; the other exports are untouched
    assert ops.unpack_tensors(buf, offs, [(100,)], [torch.float32])[0].shape == (100,)
    assert ops.axpby(a, a).shape == (100,)


# ---------------------------------------------------------------------------
# stream hand-off
# ---------------------------------------------------------------------------

@requires_gpu
def test_bundle_stream_handoff():
    from lzy_amd.runtime.streams import StreamPlacer
    from lzy_amd.utils.metrics import METRICS

    placer = StreamPlacer()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        value = {"w": torch.ones(20000, device="cuda")}
    placer.record_output("e-dev", value, stream=s1)
    assert "e-dev" in placer._events and placer._events["e-dev"][1] == s1
    waits = METRICS.counter_value("lzy_stream_waits_inserted")
    with torch.cuda.stream(s2):
        placer.wait_value("e-dev", value)
    assert METRICS.counter_value("lzy_stream_waits_inserted") == waits + 1
    placer.record_output("e-cpu", {"w": torch.ones(20000)}, stream=s1)
    assert "e-cpu" not in placer._events
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# end to end: two ranks, one GPU
# ---------------------------------------------------------------------------

@requires_gpu
def test_state_dict_bundle_two_ranks_one_gpu(tmp_path):
    """A transformer state_dict (device leaves, ~400 KiB) plus an int and a
    str from one rank to an op on the other, both ranks on one GPU (the
    host-staged path).  tests/pool_script_bundle.py holds the checks: bit
    equality, leaves on the consumer's current device and views of one
    allocation, meta kind ``bundle``, no pickle in the producer's store,
    ``lzy_transfers_bundle >= 1``, and the driver-side read."""
    env = dict(os.environ)
    env["BUNDLE_DEVICE"] = "cuda"
    env["BUNDLE_EXPECT"] = "bundle"
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
            "tests/pool_script_bundle.py",
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=240,
    )
    print("STDOUT:", res.stdout[-4000:])
    if res.returncode != 0:
        print("STDERR:", res.stderr[-4000:])
    assert res.returncode == 0
    assert "BUNDLE-SCRIPT-OK" in res.stdout
