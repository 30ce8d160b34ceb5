"""Block-scaled FP8 (mxfp8) wire codec: the torch codec against the format
spec (docs/mxwire.md), special values, and the transport over gloo."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from mxwire_util import (
    assert_within_bound,
    check_special_decode,
    special_vector,
)

ROOT = Path(__file__).resolve().parent.parent

SIZES = [1, 31, 32, 33, 1000, 65536 + 7]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MAGS = [1e-4, 1.0, 3e3]


def _input(n, dtype, mag):
    g = torch.Generator().manual_seed(1234)
    return (torch.randn(n, generator=g) * mag).to(dtype)


@pytest.mark.parametrize("mag", MAGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_torch_codec_matches_spec(dtype, mag):
    from lzy_amd.channels.mxwire import (
        mx8_nbytes, mx8_pack_torch, mx8_unpack_torch,
    )

    for n in SIZES:
        x = _input(n, dtype, mag)
        buf = mx8_pack_torch(x)
        nblk = (n + 31) // 32
        assert buf.dtype == torch.uint8 and buf.dim() == 1
        assert buf.numel() == 33 * nblk == mx8_nbytes(n)
        assert torch.equal(buf, mx8_pack_torch(x))  # deterministic
        # payload bytes of the padded tail encode 0.0
        assert buf[n: 32 * nblk].eq(0).all()
        # scale bytes: integer arithmetic on the block amax, per the spec
        xf = torch.zeros(nblk * 32)
        xf[:n] = x.float()
        amax_bits = xf.view(nblk, 32).abs().amax(dim=1).view(torch.int32)
        want_b = []
        for bits in amax_bits.tolist():
            e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
            want_b.append(max(0, e - 8 + (1 if m > 0x600000 else 0)))
        assert buf[32 * nblk:].tolist() == want_b
        assert max(want_b) <= 247
        # payload: e4m3_rne(x * 2^(127-b)), nothing saturates
        scale = torch.tensor(want_b, dtype=torch.float64).sub(127).exp2()
        scaled = xf.view(nblk, 32).double() / scale[:, None]
        assert scaled.abs().max().item() <= 448
        want_q = scaled.float().to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(buf[: 32 * nblk], want_q.reshape(-1))

        y = mx8_unpack_torch(buf, x.shape, dtype)
        assert y.dtype == dtype and y.shape == x.shape
        rel = assert_within_bound(y, x, dtype)
        if n >= 1000:
            assert rel < 0.04, f"relative L2 error {rel}"


def test_plain_e4m3_cast_zeroes_small_values():
    """Why the block scale exists: an unscaled e4m3 cast of gradient-sized
    values is all zero, the block-scaled codec keeps ~2.7 % error."""
    from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch

    x = _input(65536 + 7, torch.float32, 1e-4)
    plain = x.to(torch.float8_e4m3fn).float()
    assert plain.eq(0).all()
    y = mx8_unpack_torch(mx8_pack_torch(x), x.shape, torch.float32)
    assert ((y - x).norm() / x.norm()).item() < 0.04


def test_special_values():
    from lzy_amd.channels.mxwire import mx8_pack_torch, mx8_unpack_torch

    v = special_vector()
    buf = mx8_pack_torch(v)
    assert buf.numel() == 33 * 4
    check_special_decode(buf[128:], mx8_unpack_torch(buf, 128, torch.float32))
    for dt in (torch.bfloat16, torch.float16):
        d = mx8_unpack_torch(buf, 128, dt)
        assert torch.isnan(d).nonzero().reshape(-1).tolist() == [32]
        assert d[64].item() == 3.5 and d[65].item() == -3.5

    # a block with no finite element at all gets b == 0
    w = torch.full((32,), float("inf"))
    w[3], w[7] = float("nan"), float("-inf")
    buf = mx8_pack_torch(w)
    assert buf[32:].tolist() == [0]
    d = mx8_unpack_torch(buf, 32, torch.float32)
    assert torch.isnan(d).nonzero().reshape(-1).tolist() == [3]


def test_shapes_and_errors():
    from lzy_amd.channels.mxwire import (
        mx8_nbytes, mx8_pack, mx8_pack_torch, mx8_unpack, mx8_unpack_torch,
    )

    assert [mx8_nbytes(n) for n in (0, 1, 32, 33)] == [0, 33, 33, 66]
    x = _input(6 * 50, torch.bfloat16, 1.0).reshape(6, 50)
    buf = mx8_pack(x)  # CPU tensor -> torch codec
    assert torch.equal(buf, mx8_pack_torch(x))
    # a non-contiguous view packs in logical (contiguous) order
    assert torch.equal(mx8_pack_torch(x.t()), mx8_pack_torch(x.t().contiguous()))
    y = mx8_unpack(buf, (6, 50), torch.bfloat16)
    assert y.shape == (6, 50)
    assert torch.equal(y, mx8_unpack_torch(buf, (6, 50), torch.bfloat16))
    empty = mx8_pack_torch(torch.empty(0))
    assert empty.numel() == 0
    assert mx8_unpack_torch(empty, 0, torch.float32).numel() == 0
    with pytest.raises(ValueError):
        mx8_pack_torch(torch.arange(64))
    with pytest.raises(ValueError):
        mx8_unpack_torch(buf[:-1], (6, 50), torch.bfloat16)
    with pytest.raises(ValueError):
        mx8_unpack_torch(buf, (6, 50), torch.int64)


def test_ops_api_validation():
    """ops.mx8_*: size helper, and CPU tensors are refused like the
    neighbouring device-only ops."""
    import lzy_amd.ops as ops

    assert ops.mx8_nbytes(65536 + 7) == 33 * 2049
    with pytest.raises(ValueError):
        ops.mx8_pack(torch.zeros(64))
    with pytest.raises(ValueError):
        ops.mx8_unpack(torch.zeros(66, dtype=torch.uint8), 64, torch.float32)


def test_stale_library_keeps_existing_ops(monkeypatch):
    """A libhipops.so built before the mx8 exports still loads: the
    existing ops stay bound, only mx8_* raise NativeExtensionMissing."""
    import ctypes

    import lzy_amd.ops as ops
    from lzy_amd.exceptions import NativeExtensionMissing

    if not ops.NATIVE:
        pytest.skip("libhipops.so not loadable here")

    real_cdll = ctypes.CDLL

    class Stale:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("lz_mx8"):
                raise AttributeError(name)
            return getattr(self._lib, name)

    def fake_cdll(path, *a, **k):
        lib = real_cdll(path, *a, **k)
        return Stale(lib) if str(path) == ops._LIB_PATH else lib

    monkeypatch.setattr(ops, "_lib", None)
    monkeypatch.setattr(ops, "_MX8", True)
    monkeypatch.setattr(ctypes, "CDLL", fake_cdll)
    lib = ops._try_load()
    assert lib is not None and ops._MX8 is False
    assert ops._require_native() is lib  # existing ops unaffected
    assert lib.lz_cast_copy is not None
    with pytest.raises(NativeExtensionMissing):
        ops._require_mx8()


def test_transport_predicate():
    from lzy_amd.channels import transport as tp

    n = tp._WIRE_MIN_ELEMS
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert tp._should_mxcast(dt, n, True)
        assert not tp._should_mxcast(dt, n, False)
        assert not tp._should_mxcast(dt, n - 1, True)
    assert not tp._should_mxcast(torch.int64, n, True)
    assert not tp._should_mxcast(torch.float64, n, True)
    assert "mxfp8" not in tp._WIRE_DTYPES  # not a torch dtype


def _run_distributed(script: str, nproc: int, tmp_path, extra_env=None, timeout=180):
    env = dict(os.environ)
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    env["MASTER_ADDR"] = "127.0.0.1"
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    if extra_env:
        env.update(extra_env)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={nproc}",
        "--master-addr", "127.0.0.1", "--master-port", str(port),
        script,
    ]
    return subprocess.run(
        cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout
    )


def test_transport_mxfp8_over_gloo(tmp_path):
    r = _run_distributed("tests/mxwire_transport_script.py", 2, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "MXWIRE-TRANSPORT-OK" in r.stdout
