"""The MXINT8 wire codec, CPU side (docs/mxwire.md, "MXINT8"): the torch
codec against a float64 reference written from the spec, bit for bit; the
fused decode-combine against its formula; the plan and config plumbing; a
world-2 gloo pair; the error bound.  The reference and the inputs below are
shared with tests/test_gpu_mxint8.py.
"""
import numpy as np
import pytest
import torch

from lzy_amd.channels import mxwire
from lzy_amd.channels.mxwire import (
    mx8_nbytes,
    mxi8_axpby_torch,
    mxi8_pack_torch,
    mxi8_unpack_torch,
)
from lzy_amd.config import Config
from test_mxplan import _plan, _torchrun

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = ["f32", "bf16", "f16"]
SCALES = (0, 1, 5, 6, 7, 127, 133, 134, 253, 254)
ALPHA, BETA = 0.5, -1.5


def mxi8_pack_ref(x: np.ndarray) -> np.ndarray:
    """fp32 values -> wire bytes.  Every product below is exact in float64."""
    n = x.size
    nblk = -(-n // 32)
    v = np.zeros(nblk * 32, np.float64)
    v[:n] = x.astype(np.float64)
    v = v.reshape(nblk, 32)
    amax = np.where(np.isfinite(v), np.abs(v), 0.0).max(axis=1, initial=0.0)

    def fits(b):
        return np.rint(np.ldexp(amax, 133 - b)) <= 127      # rint is RNE

    # the smallest b in [0, 254] that fits: walk up from two below log2
    b = np.where(amax > 0, np.clip(np.frexp(amax)[1] + 124, 0, 254), 0)
    for _ in range(4):
        b = np.where(fits(b) | (b == 254), b, b + 1)
    assert np.all(fits(b) | (b == 254)) and np.all((b == 0) | ~fits(np.maximum(b - 1, 0)))
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(np.ldexp(v, (133 - b)[:, None])), -127, 127)
    q = np.where(np.isnan(v), -128.0, q).astype(np.int8)    # -0.0 -> 0x00
    return np.concatenate([q.view(np.uint8).ravel(), b.astype(np.uint8)])


def mxi8_unpack_ref(buf: np.ndarray, n: int) -> np.ndarray:
    """wire bytes -> the decoded values in float64 (exact; NaN for 0x80)."""
    nblk = -(-n // 32)
    q = buf[: 32 * nblk].view(np.int8).astype(np.float64).reshape(nblk, 32)
    x = np.ldexp(q, buf[32 * nblk:].astype(np.int64)[:, None] - 133)
    x[q == -128] = np.nan
    return x.ravel()[:n]


def to_dtype(x64: np.ndarray, dtype) -> torch.Tensor:
    """One RNE rounding of float64 values to a torch dtype (values that went
    through fp32 on the way are exact there, so bf16 rounds once too)."""
    with np.errstate(over="ignore"):
        if dtype == F16:
            return torch.from_numpy(x64.astype(np.float16))
        return torch.from_numpy(x64.astype(np.float32)).to(dtype)


def axpby_ref(a: torch.Tensor, wire: np.ndarray, dst_dtype) -> torch.Tensor:
    """round(fmaf(a, alpha, fl32(x^ * beta))).  The inputs keep the float64
    sum exact, so its rounding to fp32 is the FMA's."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (mxi8_unpack_ref(wire, a.numel()) * BETA).astype(np.float32)
        r = a.to(torch.float64).numpy() * ALPHA + p.astype(np.float64)
        return to_dtype(r.astype(np.float32).astype(np.float64), dst_dtype)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def assert_same(got: torch.Tensor, want: torch.Tensor, what=""):
    """Bit equality, NaN by position."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    bad = (bits(got) != bits(want)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} differ, first at " \
        f"{int(bad.nonzero()[0])}"


def _f32_bits(words) -> torch.Tensor:
    return torch.tensor(words, dtype=torch.int64).to(torch.int32).view(F32)


def encode_inputs() -> torch.Tensor:
    """Whole blocks of fp32: both sides of every boundary of the scale rule,
    amax 0 / largest subnormal / FLT_MAX, every rounding tie, the specials."""
    blocks = []
    amaxes = [(e << 23 | 0x7F0000) + d for e in (1, 6, 127, 253, 254) for d in (-1, 0, 1)]
    amaxes += [0x7F8000 + d for d in (-1, 0, 1)] + [0, 0x007FFFFF, 0x7F7FFFFF]
    frac = torch.tensor([1.0, -0.75, 0.5, -0.3, 0.1, -0.01, 1e-3, -1e-5] * 4)
    for w in amaxes:
        blocks.append(_f32_bits([w]) * frac)       # |frac| <= 1: amax is element 0
    # amax 127 has b = 133, where the scaled value is x itself: k + 0.5
    ties = torch.arange(-127, 127, dtype=F32) + 0.5
    for s in range(0, 254, 31):
        t = torch.zeros(32)
        t[0] = 127.0
        t[1: 1 + len(ties[s: s + 31])] = ties[s: s + 31]
        blocks.append(t)
    for head in ([float("nan"), 1.0], [float("inf"), float("-inf"), 2.0], [-0.0, 1e-45]):
        blocks.append(torch.tensor(head + [0.0] * (32 - len(head))))
    return torch.cat(blocks)


def decode_inputs():
    """All 256 payload bytes under each of SCALES: (wire buffer, numel)."""
    payload = np.tile(np.arange(256, dtype=np.uint8), len(SCALES))
    scales = np.repeat(np.array(SCALES, np.uint8), 8)
    return np.concatenate([payload, scales]), payload.size


def axpby_operand(wire: np.ndarray, n: int) -> torch.Tensor:
    """fp32 accumulator values within 2^10 of the decoded ones in magnitude
    (1.0 where those are zero or NaN), so that the float64 sum is exact."""
    x = mxi8_unpack_ref(wire, n)
    g = np.random.default_rng(7)
    e = np.frexp(np.where(np.isfinite(x) & (x != 0), x, 1.0))[1]
    e = np.clip(e + g.integers(-10, 11, n), -140, 127)
    a = np.ldexp(g.uniform(0.5, 1.0, n).astype(np.float32).astype(np.float64), e)
    return torch.from_numpy((a * g.choice([-1.0, 1.0], n)).astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_torch_equals_reference(dtype):
    x = encode_inputs().to(dtype)
    want = mxi8_pack_ref(x.to(F32).numpy())
    got = mxi8_pack_torch(x).numpy()
    assert got.size == mx8_nbytes(x.numel())
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert 0xFF not in set(want[x.numel():])


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33])
def test_pack_torch_sizes(n):
    x = encode_inputs()[32 * 20 - 1:][:n]       # starts on a tie block's last element
    got = mxi8_pack_torch(x).numpy()
    assert np.array_equal(got, mxi8_pack_ref(x.numpy()))
    assert_same(mxi8_unpack_torch(torch.from_numpy(got), n, F32),
                to_dtype(mxi8_unpack_ref(got, n), F32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_torch_equals_reference(dtype):
    wire, n = decode_inputs()
    got = mxi8_unpack_torch(torch.from_numpy(wire), n, dtype)
    assert_same(got, to_dtype(mxi8_unpack_ref(wire, n), dtype))
    assert int(torch.isnan(got).sum()) == len(SCALES)       # 0x80, nothing else
    assert bits(got)[0] == 0                                # payload 0x00 is +0


@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("a_dtype", DTYPES, ids=IDS)
def test_axpby_torch_is_the_formula(a_dtype, dst_dtype):
    wire, n = decode_inputs()
    a = axpby_operand(wire, n).to(a_dtype)
    got = mxi8_axpby_torch(a, torch.from_numpy(wire), ALPHA, BETA, out_dtype=dst_dtype)
    assert_same(got, axpby_ref(a, wire, dst_dtype))


def test_build_plan_records_mxint8():
    n = (1 << 20) + 40
    plan = _plan((n,), wire="mxint8")
    assert plan["wire"] == "mxint8" and plan["chunk_elems"] == 262400
    fp8 = _plan((n,), wire="mxfp8")
    assert fp8["wire"] == "mxfp8"
    assert {k: v for k, v in plan.items() if k != "wire"} == \
        {k: v for k, v in fp8.items() if k != "wire"}
    assert _plan((65535,), wire="mxint8") == _plan((65535,))
    assert _plan((n,), wire="")["wire"] == ""
    with pytest.raises(ValueError):
        _plan((n,), wire="fp8")


@pytest.mark.parametrize("wire,ok", [("mxint8", True), ("fp8", False)])
def test_scheduler_stream_wire_cast(wire, ok):
    from types import SimpleNamespace

    from lzy_amd.runtime.pool import _DriverScheduler

    pool = SimpleNamespace(world=1, agent=SimpleNamespace(transport=None))
    try:
        Config.reset(stream_wire_cast=wire)
        if ok:
            assert _DriverScheduler(pool, SimpleNamespace(), [], None)._stream_wire == wire
        else:
            with pytest.raises(ValueError, match="stream_wire_cast"):
                _DriverScheduler(pool, SimpleNamespace(), [], None)
    finally:
        Config.reset()


def test_pair_two_ranks_bit_identical_to_host_emulation(tmp_path):
    out = _torchrun("tests/mxint8_pair_script.py", 2, tmp_path, timeout=180)
    assert "MXINT8-PAIR-OK" in out


@pytest.mark.parametrize("mag", [1.0, 1e-4])
def test_error_bound_and_less_error_than_mxfp8(mag):
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(3)) * mag
    wire = mxi8_pack_torch(x)
    dec = mxi8_unpack_torch(wire, x.numel(), F32)
    err = (dec.double() - x.double()).abs()
    half_step = torch.ldexp(torch.ones(1, dtype=torch.float64),
                            wire[x.numel():].to(torch.int32) - 134)
    assert bool((err.view(-1, 32).amax(1) <= half_step).all())
    fp8 = mxwire.mx8_unpack_torch(mxwire.mx8_pack_torch(x), x.numel(), F32)
    rel, rel_fp8 = (float((y.double() - x.double()).norm() / x.double().norm())
                    for y in (dec, fp8))
    print(f"relative L2 at {mag}: mxint8 {rel:.4f}, mxfp8 {rel_fp8:.4f}")
    assert 0 < rel < rel_fp8
