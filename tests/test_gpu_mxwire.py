"""Block-scaled FP8 (mxfp8) HIP pack/unpack kernels on MI355X (gfx950).

The oracle is the torch codec (lzy_amd.channels.mxwire) run on the CPU
copy of the data, never the kernels themselves.  These tests REQUIRE the
native extension: a missing libhipops.so fails loudly."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from mxwire_util import (
    assert_wire_equal,
    assert_within_bound,
    check_special_decode,
    special_vector,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROOT = Path(__file__).resolve().parent.parent

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
SIZES = [1, 7, 31, 32, 33, 255, 256, 257, 2048 + 5, 65536 + 7]
MAGS = [1e-4, 1.0, 3e3]


@pytest.fixture(scope="module", autouse=True)
def _native():
    import lzy_amd.ops as ops

    if torch.cuda.is_available():
        assert ops.NATIVE, "HIP ops must be built+loadable on a GPU box"
    yield


def _input(n, dtype, seed=0):
    """CPU tensor whose three thirds sit at the three magnitudes."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(n, generator=g)
    mag = torch.tensor(MAGS)[(torch.arange(n) * 3) // max(n, 1)]
    return (x * mag).to(dtype)


def _check_pack(x_cpu, got_cpu):
    """Kernel-packed bytes vs the oracle's: every scale byte, payload byte
    and padding byte equal.  Both sides round the exact fp32 product to
    e4m3 with ties to even, so there is nothing to allow for."""
    from lzy_amd.channels.mxwire import mx8_pack_torch

    assert_wire_equal(x_cpu, got_cpu, mx8_pack_torch(x_cpu),
                      f"mx8_pack n={x_cpu.numel()} {x_cpu.dtype}")


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_matches_oracle(dtype):
    from lzy_amd.ops import mx8_nbytes, mx8_pack

    for n in SIZES:
        x = _input(n, dtype, seed=n)
        buf = mx8_pack(x.cuda())
        assert buf.is_cuda and buf.numel() == mx8_nbytes(n)
        _check_pack(x, buf.cpu())
    # out= variant writes in place
    x = _input(257, dtype)
    out = torch.empty(mx8_nbytes(257), dtype=torch.uint8, device="cuda")
    assert mx8_pack(x.cuda(), out=out) is out
    _check_pack(x, out.cpu())


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grid_stride_wraps(dtype):
    """Grid capped at 2 blocks: every lane takes several trips, the last
    one partial, at a tiny size."""
    import lzy_amd.ops as ops
    from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch

    lib = ops._require_native()
    n = 3 * 4096 + 45
    x = _input(n, dtype, seed=5)
    want = mx8_pack_torch(x)
    lib.lz_set_max_blocks(2)
    try:
        buf = ops.mx8_pack(x.cuda())
        dec = ops.mx8_unpack(want.cuda(), n, dtype)
        torch.cuda.synchronize()
    finally:
        lib.lz_set_max_blocks(0)
    _check_pack(x, buf.cpu())
    assert torch.equal(dec.cpu(), mx8_unpack_torch(want, n, dtype))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_matches_oracle(dtype):
    from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch
    from lzy_amd.ops import mx8_unpack

    for n in SIZES:
        for src_dtype in DTYPES:
            wire = mx8_pack_torch(_input(n, src_dtype, seed=n))
            want = mx8_unpack_torch(wire, n, dtype)
            got = mx8_unpack(wire.cuda(), n, dtype)
            assert got.dtype == dtype and got.shape == (n,)
            assert torch.equal(got.cpu(), want), (n, src_dtype)
    # shape form
    wire = mx8_pack_torch(_input(6 * 50, dtype))
    got = mx8_unpack(wire.cuda(), (6, 50), dtype)
    assert got.shape == (6, 50)
    assert torch.equal(got.cpu(), mx8_unpack_torch(wire, (6, 50), dtype))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_never_writes_past_out(dtype):
    from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch
    from lzy_amd.ops import mx8_unpack

    guard, sentinel = 64, -7.0
    for n in [1, 31, 33, 257, 2048 + 5]:
        wire = mx8_pack_torch(_input(n, dtype, seed=n))
        want = mx8_unpack_torch(wire, n, dtype)
        for lead in (guard, guard + 1):  # aligned and element-aligned out
            full = torch.full((lead + n + guard,), sentinel, dtype=dtype,
                              device="cuda")
            out = full[lead: lead + n]
            assert mx8_unpack(wire.cuda(), n, dtype, out=out) is out
            host = full.cpu()
            assert host[:lead].eq(sentinel).all()
            assert host[lead + n:].eq(sentinel).all()
            assert torch.equal(host[lead: lead + n], want)


@requires_gpu
def test_element_aligned_views():
    """src / dst that are only element-aligned (views starting at element
    1 or 3) give the bytes of the aligned run on the same values."""
    from lzy_amd.ops import mx8_pack, mx8_unpack

    for dtype, offs in ((torch.bfloat16, (1, 3)), (torch.float32, (1,)),
                        (torch.float16, (1,))):
        base = _input(4096 + 3 + 77, dtype, seed=3).cuda()
        for off in offs:
            view = base[off:]
            assert view.data_ptr() % 16 != 0
            aligned = view.clone()
            assert aligned.data_ptr() % 16 == 0
            a = mx8_pack(view)
            b = mx8_pack(aligned)
            assert torch.equal(a, b)
            _check_pack(view.cpu(), a.cpu())
            n = view.numel()
            want = mx8_unpack(b, n, dtype)
            full = torch.zeros(n + 1, dtype=dtype, device="cuda")
            mx8_unpack(b, n, dtype, out=full[1:])
            assert torch.equal(full[1:], want)
            assert full[0].item() == 0
    # a wire buffer that is itself only byte-aligned
    x = _input(1000, torch.bfloat16, seed=4).cuda()
    wire = mx8_pack(x)
    shifted = torch.empty(wire.numel() + 1, dtype=torch.uint8, device="cuda")
    mx8_pack(x, out=shifted[1:])
    assert torch.equal(shifted[1:], wire)
    assert torch.equal(
        mx8_unpack(shifted[1:], 1000, torch.bfloat16),
        mx8_unpack(wire, 1000, torch.bfloat16),
    )


@requires_gpu
def test_special_values_on_device():
    from lzy_amd.channels.mxwire import mx8_unpack_torch
    from lzy_amd.ops import mx8_pack, mx8_unpack

    v = special_vector()
    buf = mx8_pack(v.cuda())
    host = buf.cpu()
    check_special_decode(host[128:], mx8_unpack_torch(host, 128, torch.float32))
    check_special_decode(host[128:], mx8_unpack(buf, 128, torch.float32))
    # a block with no finite element at all gets b == 0
    w = torch.full((32,), float("inf"))
    w[3], w[7] = float("nan"), float("-inf")
    buf = mx8_pack(w.cuda())
    assert buf[32:].tolist() == [0]
    d = mx8_unpack(buf, 32, torch.float32).cpu()
    assert torch.isnan(d).nonzero().reshape(-1).tolist() == [3]
    # fp32 subnormals: b == 0 blocks scale by 2^127 and decode by the
    # subnormal multiplier 2^-127 — nothing may be flushed to zero
    g = torch.Generator().manual_seed(2)
    tiny = torch.randn(96, generator=g) * 1e-40
    buf = mx8_pack(tiny.cuda())
    assert buf[96:].tolist() == [0, 0, 0]
    _check_pack(tiny, buf.cpu())
    want = mx8_unpack_torch(buf.cpu(), 96, torch.float32)
    assert want.ne(0).any()
    assert torch.equal(mx8_unpack(buf, 96, torch.float32).cpu(), want)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cross_decoding(dtype):
    """The host-staged path's contract: either side may be the kernel."""
    from lzy_amd.channels import mxwire
    from lzy_amd.ops import mx8_pack, mx8_unpack

    n = 65536 + 7
    for mag in MAGS:
        g = torch.Generator().manual_seed(11)
        x = (torch.randn(n, generator=g) * mag).to(dtype)
        # GPU pack -> host -> torch unpack
        y = mxwire.mx8_unpack_torch(mx8_pack(x.cuda()).cpu(), n, dtype)
        assert assert_within_bound(y, x, dtype) < 0.04
        # torch pack -> device -> GPU unpack
        z = mx8_unpack(mxwire.mx8_pack_torch(x).cuda(), n, dtype)
        assert assert_within_bound(z, x, dtype) < 0.04
        # the dispatchers take the kernel for device tensors
        buf = mxwire.mx8_pack(x.cuda())
        assert buf.is_cuda
        assert torch.equal(mxwire.mx8_unpack(buf, n, dtype).cpu(), y)


@requires_gpu
def test_error_paths():
    from lzy_amd.ops import mx8_nbytes, mx8_pack, mx8_unpack

    with pytest.raises(ValueError):
        mx8_pack(torch.arange(64, device="cuda"))  # int64
    good = mx8_pack(torch.randn(100, device="cuda"))
    assert good.numel() == mx8_nbytes(100)
    with pytest.raises(ValueError):
        mx8_unpack(good[:-1], 100, torch.float32)  # short buffer
    with pytest.raises(ValueError):
        mx8_unpack(good, 100, torch.int64)
    with pytest.raises(ValueError):
        mx8_pack(torch.randn(100, device="cuda"),
                 out=torch.empty(10, dtype=torch.uint8, device="cuda"))
    empty = mx8_pack(torch.empty(0, device="cuda"))
    assert empty.numel() == 0 and empty.dtype == torch.uint8
    back = mx8_unpack(empty, 0, torch.bfloat16)
    assert back.numel() == 0 and back.dtype == torch.bfloat16


@requires_gpu
def test_transport_mxfp8_two_ranks_one_gpu(tmp_path):
    """Device bf16 tensor over the host-staged path (2 ranks, 1 GPU):
    kernel pack before staging, kernel unpack on arrival."""
    env = dict(os.environ)
    env["MXWIRE_DEVICE"] = "cuda"
    env["HIP_VISIBLE_DEVICES"] = "0"  # both ranks share one GPU
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    res = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node=2",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            "tests/mxwire_transport_script.py",
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300,
    )
    if res.returncode != 0:
        print("STDOUT:", res.stdout[-4000:])
        print("STDERR:", res.stderr[-4000:])
    assert res.returncode == 0
    assert "MXWIRE-TRANSPORT-OK" in res.stdout
