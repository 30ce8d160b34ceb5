"""Streamed merge-tree plans on the MXFP8 wire, CPU side: the torch
reference of the fused decode-combine, the plan builder's ``wire``
keyword, the config field, and the world-4 / world-2 gloo runs whose
results must equal a host emulation bit for bit (docs/mxwire.md, "Plans").
"""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from lzy_amd.channels import mxwire
from lzy_amd.channels.mxwire import (
    mx8_axpby_torch,
    mx8_nbytes,
    mx8_pack_torch,
    mx8_unpack_torch,
)
from lzy_amd.channels.treeplan import build_plan, find_components
from lzy_amd.config import Config
from mxplan_util import make_tree

ROOT = Path(__file__).resolve().parent.parent

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ---------------------------------------------------------------------------
# mx8_axpby_torch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 31, 32, 33, 257])
def test_axpby_torch_is_the_formula(n):
    """decode to fp32, p = fp32(x^ * beta), a*alpha + p in float64, round
    to fp32, round to the output dtype — spelled out independently."""
    g = torch.Generator().manual_seed(n)
    alpha, beta = 0.3, -1.7  # not fp32 values: the codec rounds them first
    for a_dtype in DTYPES:
        a = (torch.randn(n, generator=g) * 5).to(a_dtype)
        wire = mx8_pack_torch(torch.randn(n, generator=g) * 3e3)
        x = mx8_unpack_torch(wire, n, torch.float32)
        p = x * _f32(beta)
        assert p.dtype == torch.float32
        s = a.double() * _f32(alpha).double() + p.double()
        for out_dtype in DTYPES:
            want = s.float().to(out_dtype)
            got = mx8_axpby_torch(a, wire, alpha, beta, out_dtype=out_dtype)
            assert got.dtype == out_dtype and got.shape == a.shape
            assert torch.equal(got, want), (a_dtype, out_dtype)
        assert mx8_axpby_torch(a, wire, alpha, beta).dtype == a_dtype


def test_axpby_torch_decoded_operand_is_not_rounded_to_16_bits():
    """f16: 448 * 2^8 decodes to 114688 in fp32 (past the f16 maximum);
    times beta = 0.5 it fits again.  unpack-to-f16 then axpby gives Inf."""
    wire = torch.zeros(33, dtype=torch.uint8)
    wire[0], wire[32] = 0x7E, 127 + 8
    a = torch.zeros(1, dtype=torch.float16)
    assert torch.isinf(mx8_unpack_torch(wire, 1, torch.float16)).all()
    got = mx8_axpby_torch(a, wire, 1.0, 0.5)
    assert got.dtype == torch.float16 and got.item() == 57344.0


def test_axpby_torch_nan_and_shape():
    a = torch.ones(2, 32)
    x = torch.ones(64)
    x[5] = float("nan")
    wire = mx8_pack_torch(x)
    assert wire[5].item() == 0x7F
    got = mx8_axpby_torch(a, wire, 1.0, 1.0)
    assert got.shape == (2, 32)
    assert torch.isnan(got.reshape(-1)).nonzero().reshape(-1).tolist() == [5]
    wire[6] = 0xFF  # the other NaN code
    got = mx8_axpby_torch(a, wire, 1.0, 0.0)
    assert torch.isnan(got.reshape(-1)).nonzero().reshape(-1).tolist() == [5, 6]


def test_axpby_torch_errors():
    a = torch.ones(64)
    wire = mx8_pack_torch(a)
    with pytest.raises(ValueError):
        mx8_axpby_torch(a, wire[:-1], 1.0, 1.0)            # short wire
    with pytest.raises(ValueError):
        mx8_axpby_torch(a, wire.to(torch.int16), 1.0, 1.0)  # not uint8
    with pytest.raises(ValueError):
        mx8_axpby_torch(a.to(torch.int64), wire, 1.0, 1.0)
    with pytest.raises(ValueError):
        mx8_axpby_torch(a, wire, 1.0, 1.0, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        mx8_axpby_torch(torch.ones(65), wire, 1.0, 1.0)    # numel mismatch


def test_axpby_dispatcher_cpu():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(100, generator=g)
    wire = mx8_pack_torch(torch.randn(100, generator=g))
    want = mx8_axpby_torch(a, wire, 0.5, 0.5)
    assert torch.equal(mxwire.mx8_axpby(a, wire, 0.5, 0.5), want)
    dst = torch.empty(100, dtype=torch.bfloat16)
    assert mxwire.mx8_axpby(a, wire, 0.5, 0.5, dst=dst) is dst
    assert torch.equal(
        dst, mx8_axpby_torch(a, wire, 0.5, 0.5, out_dtype=torch.bfloat16))
    acc = a.clone()  # in place
    assert mxwire.mx8_axpby(acc, wire, 0.5, 0.5, dst=acc) is acc
    assert torch.equal(acc, want)
    with pytest.raises(ValueError):
        mxwire.mx8_axpby(a, wire, 0.5, 0.5, dst=torch.empty(99))


# ---------------------------------------------------------------------------
# build_plan(..., wire=)
# ---------------------------------------------------------------------------

def _plan(shape, dtype="float32", chunk_bytes=32 << 20, **kw):
    calls, metas = make_tree(4, shape=shape, dtype=dtype)
    [order] = find_components(calls)
    return build_plan("p", order, calls, metas.get, chunk_bytes=chunk_bytes,
                      cuda_p2p=False, **kw)


def test_build_plan_wired():
    plan = _plan((1 << 20,), wire="mxfp8")
    assert plan["wire"] == "mxfp8"
    assert plan["chunk_elems"] % 256 == 0
    assert plan["numel"] / plan["chunk_elems"] >= 4
    # a size that is no multiple of anything: rounded UP after the
    # "at least 4 chunks" adjustment
    n = (1 << 20) + 40
    plan = _plan((n,), wire="mxfp8")
    assert plan["wire"] == "mxfp8" and plan["chunk_elems"] == 262400
    assert -(-n // plan["chunk_elems"]) == 4
    assert n - 3 * plan["chunk_elems"] == 261416
    # chunk j's wire bytes start 8 B-aligned, its elements 16 B-aligned
    assert mx8_nbytes(plan["chunk_elems"]) % 264 == 0
    for dtype in ("bfloat16", "float16"):
        plan = _plan((1 << 18,), dtype=dtype, chunk_bytes=1 << 16, wire="mxfp8")
        assert plan["wire"] == "mxfp8" and plan["chunk_elems"] % 256 == 0
    # a chunk size that is already a multiple stays as it is
    assert _plan((1 << 20,), chunk_bytes=4 << 18, wire="mxfp8")[
        "chunk_elems"] == 1 << 18


@pytest.mark.parametrize("shape,dtype", [
    ((65535,), "float32"),       # under the transport's threshold
    ((1 << 20,), "int64"),       # not a float dtype
    ((1 << 20,), "float64"),
])
def test_build_plan_stays_unwired(shape, dtype):
    base = _plan(shape, dtype=dtype)
    plan = _plan(shape, dtype=dtype, wire="mxfp8")
    assert plan["wire"] == ""
    assert plan == base


def test_build_plan_threshold_is_inclusive():
    assert _plan((65536,), chunk_bytes=1 << 16, wire="mxfp8")["wire"] == "mxfp8"


def test_build_plan_default_is_unchanged():
    """wire="" (the default): every field the parent computed, unchanged;
    the one new key says unwired."""
    for shape, chunk in (((1 << 20,), 32 << 20), (((1 << 20) + 40,), 1 << 20),
                         ((1024,), 1024), ((300, 1000), 1 << 18)):
        plan = _plan(shape, chunk_bytes=chunk)
        assert plan == _plan(shape, chunk_bytes=chunk, wire="")
        assert plan.pop("wire") == ""
        numel = 1
        for d in shape:
            numel *= d
        per = max(1, chunk // 4)
        if numel // per < 4:
            per = max((1 << 20) // 4, -(-numel // 4))
        assert plan["chunk_elems"] == per
        assert set(plan) == {
            "plan_id", "nonce", "shape", "dtype", "numel", "chunk_elems",
            "device_cuda", "cuda_p2p", "steps_by_rank", "participants",
            "node_rank", "member_order",
        }


def test_build_plan_rejects_unknown_wire():
    with pytest.raises(ValueError):
        _plan((1 << 20,), wire="fp8")


# ---------------------------------------------------------------------------
# Config
# ---------------------------------------------------------------------------

def test_config_stream_wire_cast(monkeypatch):
    monkeypatch.delenv("LZY_STREAM_WIRE_CAST", raising=False)
    try:
        assert Config.reset().stream_wire_cast == ""
        monkeypatch.setenv("LZY_STREAM_WIRE_CAST", "mxfp8")
        cfg = Config.reset()
        assert cfg.stream_wire_cast == "mxfp8"
        assert cfg.channel_wire_cast == ""  # a field of its own
        # explicit overrides outrank the environment
        assert Config.reset(stream_wire_cast="").stream_wire_cast == ""
    finally:
        monkeypatch.delenv("LZY_STREAM_WIRE_CAST", raising=False)
        Config.reset()


def test_scheduler_rejects_bad_stream_wire_cast():
    """The driver scheduler validates the field when it reads it (the
    world-4 script below covers the same through a real workflow)."""
    from types import SimpleNamespace

    from lzy_amd.runtime.pool import _DriverScheduler

    try:
        Config.reset(stream_wire_cast="fp8")
        with pytest.raises(ValueError, match="stream_wire_cast"):
            _DriverScheduler(SimpleNamespace(world=1), SimpleNamespace(), [], None)
    finally:
        Config.reset()


# ---------------------------------------------------------------------------
# gloo runs
# ---------------------------------------------------------------------------

def _torchrun(script, nproc, tmp_path, timeout):
    env = dict(os.environ)
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    env["MASTER_ADDR"] = "127.0.0.1"
    for k in ("RANK", "WORLD_SIZE", "MXPLAN_DEVICE", "LZY_STREAM_WIRE_CAST"):
        env.pop(k, None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    res = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", f"--nproc-per-node={nproc}",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            script,
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout,
    )
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_wired_plan_world4_bit_identical_to_host_emulation(tmp_path):
    out = _torchrun("tests/pool_script_mxplan.py", 4, tmp_path, timeout=300)
    assert "MXPLAN-WIRED-OK" in out
    assert "MXPLAN-OK" in out


def test_wired_pair_two_ranks_bit_identical_to_host_emulation(tmp_path):
    out = _torchrun("tests/mxplan_pair_script.py", 2, tmp_path, timeout=180)
    assert "MXPLAN-PAIR-OK" in out
