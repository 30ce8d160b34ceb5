"""The MXFP6 (e2m3) wire codec, CPU side (docs/mxwire.md, "MXFP6"): the torch
codec against a float64 reference written from the format, bit for bit; the
names; a two-rank gloo plan and pair; the error bound and the quoted figure.
The reference and the inputs are shared with tests/test_gpu_mxfp6.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lzy_amd.channels import mxwire
from lzy_amd.channels.mxwire import mx6_axpby_torch, mx6_nbytes, mx6_pack_torch, mx6_unpack_torch
from lzy_amd.config import Config
from test_mxint8 import DTYPES, F32, IDS, assert_same, to_dtype
from test_mxplan import _torchrun

SCALES = (0, 1, 2, 120, 121, 122, 126, 127, 128, 252, 253, 254, 255)
ALPHA, BETA = 0.5, -1.5
C = np.arange(32)
E2M3 = np.where(C < 8, C / 8, (1 + (C & 7) / 8) * 2.0 ** ((C >> 3) - 1))
TIES = (E2M3[:-1] + E2M3[1:]) / 2      # 31: tie i lies between codes i and i+1


def codes_to_bytes(q: np.ndarray) -> np.ndarray:
    """Codes [nblk, 32] -> payload: element i at bits [6i, 6i+6), little-endian."""
    q = q.astype(np.uint32).reshape(-1, 8, 4)
    w = q[..., 0] | q[..., 1] << 6 | q[..., 2] << 12 | q[..., 3] << 18
    return np.stack([w, w >> 8, w >> 16], axis=2).astype(np.uint8).ravel()


def mx6_pack_ref(x: np.ndarray) -> np.ndarray:
    """fp32 values -> wire bytes.  Every product below is exact in float64."""
    n = x.size
    nblk = -(-n // 32)
    v = np.zeros(nblk * 32, np.float64)
    v[:n] = x
    v = v.reshape(nblk, 32)
    nan = np.isnan(v).any(axis=1)
    amax = np.where(np.isfinite(v), np.abs(v), 0.0).max(axis=1)
    # smallest b >= 0 with amax * 2^(127-b) <= 7.5: amax = m * 2^e, m in [.5, 1)
    m, e = np.frexp(amax)
    b = np.where(amax > 0, np.maximum(e + 124 + (m > 0.9375), 0), 0)
    assert np.all(np.ldexp(amax, 127 - b) <= 7.5)
    assert np.all((b == 0) | (np.ldexp(amax, 128 - b) > 7.5))
    with np.errstate(invalid="ignore"):
        s = np.minimum(np.ldexp(np.abs(v), (127 - b)[:, None]), 7.5)
        # a tie between codes i and i+1 goes to the even one: up iff i is odd
        code = sum((s >= t) if i % 2 else (s > t) for i, t in enumerate(TIES))
    q = code | (np.signbit(v) << 5)
    q[nan] = 0
    return np.concatenate([codes_to_bytes(q), np.where(nan, 255, b).astype(np.uint8)])


def mx6_unpack_ref(buf: np.ndarray, n: int) -> np.ndarray:
    """wire bytes -> the decoded values in float64 (exact; NaN under 0xff)."""
    nblk = -(-n // 32)
    bits = np.unpackbits(buf[: 24 * nblk], bitorder="little").reshape(nblk, 32, 6)
    q = (bits << np.arange(6, dtype=np.uint8)).sum(axis=2)
    b = buf[24 * nblk:].astype(np.int64)[:, None]
    x = np.ldexp(np.where(q & 32, -1.0, 1.0) * E2M3[q & 31], b - 127)
    return np.where(b == 255, np.nan, x).ravel()[:n]


def axpby_ref(a: torch.Tensor, wire: np.ndarray, dst_dtype) -> torch.Tensor:
    """round(fmaf(a, alpha, fl32(x^ * beta))); the float64 sum is exact."""
    with np.errstate(over="ignore", invalid="ignore"):
        xh = mx6_unpack_ref(wire, a.numel()).astype(np.float32).astype(np.float64)
        p = (xh * BETA).astype(np.float32).astype(np.float64)
        r = a.to(torch.float64).numpy() * ALPHA + p
        return to_dtype(r.astype(np.float32).astype(np.float64), dst_dtype)


def encode_inputs() -> torch.Tensor:
    """Whole blocks: both sides of the scale boundary, every scaled tie with its
    neighbours and both signs (amax 7.5: b = 127), and the specials."""
    frac = np.array([1.0, -0.75, 0.5, -0.3, 0.1, -0.01, 1e-3, -1e-5] * 4, np.float32)
    blocks = [np.array([e << 23 | m], np.uint32).view(np.float32) * frac
              for e in (0, 1, 2, 3, 127, 253, 254) for m in (0x700000, 0x700001)]
    t = TIES.astype(np.float32)
    t = np.concatenate([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(9))])
    blocks += [np.concatenate([[7.5], part]) for part in np.concatenate([t, -t]).reshape(6, 31)]
    inf, nan = float("inf"), float("nan")
    for head in ([0.0], [nan, 1.0], [inf, -inf, 2.0], [15.0, -1.75, 3e38, 1e-45],
                 [-0.0, 7.5, -0.01, 1e-40], [nan] * 32):
        blocks.append(np.array(head + [0.0] * (32 - len(head))))
    return torch.from_numpy(np.concatenate(blocks).astype(np.float32))


def decode_inputs():
    """Under each of SCALES, all 64 codes at each position mod 4: (wire, numel)."""
    codes = np.concatenate([(np.arange(64) + r) % 64 for r in range(4)])
    payload = codes_to_bytes(np.tile(codes, len(SCALES)).reshape(-1, 32))
    return np.concatenate([payload, np.repeat(np.array(SCALES, np.uint8), 8)]), 256 * len(SCALES)


def axpby_operand(wire: np.ndarray, n: int) -> torch.Tensor:
    """fp32 accumulators k * 2^(b-137), |k| < 2^20 (b capped, to stay finite)."""
    b = np.repeat(wire[24 * (n // 32):].astype(np.int64), 32)[:n]
    k = np.random.default_rng(7).integers(-(1 << 20), 1 << 20, n).astype(np.float64)
    return torch.from_numpy(np.ldexp(k, np.minimum(b, 230) - 137).astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_torch_codec_equals_reference(dtype):
    x = encode_inputs().to(dtype)
    got = mx6_pack_torch(x).numpy()
    want = mx6_pack_ref(x.to(F32).numpy())
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    wire, n = decode_inputs()
    assert_same(mx6_unpack_torch(torch.from_numpy(wire), n, dtype),
                to_dtype(mx6_unpack_ref(wire, n), dtype), "unpack")
    for a_dtype in DTYPES:
        a = axpby_operand(wire, n).to(a_dtype)
        assert_same(mx6_axpby_torch(a, torch.from_numpy(wire), ALPHA, BETA, out_dtype=dtype),
                    axpby_ref(a, wire, dtype), f"axpby from {a_dtype}")


def test_hand_worked_scale_bytes_sizes_and_names():
    x = encode_inputs()[-6 * 32: -2 * 32]
    for pack in (mx6_pack_torch(x).numpy(), mx6_pack_ref(x.numpy())):
        assert pack[96:].tolist() == [0, 255, 126, 252]
        # +-Inf are +-7.5 (codes 0x1f, 0x3f), 2.0 / 2^-1 is code 0x18
        assert not pack[:48].any() and pack[48:52].tolist() == [0xDF, 0x8F, 0x01, 0]
    for n in (1, 32, 33):
        assert mxwire.wire_nbytes("mxfp6", n) == mx6_nbytes(n) == 25 * -(-n // 32)
        assert mx6_pack_torch(x[:n]).numel() == mx6_nbytes(n)
    assert mxwire.wire_codec("mxfp6") == (mxwire.mx6_pack, mxwire.mx6_unpack, mxwire.mx6_axpby)
    assert mxwire.wire_fused("mxfp6") == (mxwire.mx6_axpby_pack, mxwire.mx6_axpby2_pack)


def test_scheduler_takes_mxfp6_for_plans_not_for_bundles():
    from lzy_amd.runtime.pool import _DriverScheduler

    pool = SimpleNamespace(world=1, agent=SimpleNamespace(transport=None))
    try:
        Config.reset(stream_wire_cast="mxfp6")
        assert _DriverScheduler(pool, SimpleNamespace(), [], None)._stream_wire == "mxfp6"
        Config.reset(bundle_wire_cast="mxfp6")
        with pytest.raises(ValueError, match="bundle_wire_cast"):
            _DriverScheduler(pool, SimpleNamespace(), [], None)
    finally:
        Config.reset()


def test_plan_and_pair_two_ranks_bit_identical(tmp_path):
    out = _torchrun("tests/mxfp6_script.py", 2, tmp_path, timeout=180)
    assert "MXFP6-PLAN-OK" in out and "MXFP6-PAIR-OK" in out


@pytest.mark.parametrize("mag", [1e-4, 1.0, 3e3])
def test_error_bound_and_relative_error(mag):
    """docs/mxwire.md quotes the figure printed here for mag 1."""
    x = (np.random.default_rng(0).standard_normal(1 << 18) * mag).astype(np.float32)
    wire = mx6_pack_ref(x)
    dec = mx6_unpack_ref(wire, x.size)
    b = wire[24 * (x.size // 32):].astype(np.int64)
    print(f"relative L2 of MXFP6 on randn * {mag}: "
          f"{np.linalg.norm(dec - x) / np.linalg.norm(x.astype(np.float64)):.4f}")
    floor = np.ldexp(1.0, b - 131)
    assert np.all(floor < np.abs(x).reshape(-1, 32).max(axis=1) / 60)
    assert np.all(np.abs(dec - x) <= np.maximum(np.abs(x) / 16, np.repeat(floor, 32)))
