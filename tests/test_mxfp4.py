"""The MXFP4 wire codec, CPU side (docs/mxwire.md, "MXFP4"): the torch codec
against a float64 reference written from the format, bit for bit; sizes; a
two-rank gloo plan with a forwarding node; the quoted error figure.  The
reference and the inputs are shared with tests/test_gpu_mxfp4.py.
"""
import numpy as np
import pytest
import torch

from lzy_amd.channels.mxwire import (
    mx4_axpby_torch, mx4_nbytes, mx4_pack_torch, mx4_unpack_torch, wire_nbytes,
)
from test_mxint8 import DTYPES, F32, IDS, assert_same, to_dtype
from test_mxplan import _torchrun

SCALES = (0, 1, 2, 126, 127, 128, 252, 253, 254, 255)
ALPHA, BETA = 0.5, -1.5
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])
TIES = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])     # -> 0, 1, 1, 2, 2, 4, 4


def mx4_pack_ref(x: np.ndarray) -> np.ndarray:
    """fp32 values -> wire bytes.  Every product below is exact in float64."""
    n = x.size
    nblk = -(-n // 32)
    v = np.zeros(nblk * 32, np.float64)
    v[:n] = x
    v = v.reshape(nblk, 32)
    nan = np.isnan(v).any(axis=1)
    amax = np.where(np.isfinite(v), np.abs(v), 0.0).max(axis=1)
    # smallest b >= 0 with amax * 2^(127-b) <= 6: amax = m * 2^e, m in [.5, 1)
    m, e = np.frexp(amax)
    b = np.where(amax > 0, np.maximum(e + 124 + (m > 0.75), 0), 0)
    assert np.all(np.ldexp(amax, 127 - b) <= 6)
    assert np.all((b == 0) | (np.ldexp(amax, 128 - b) > 6))
    with np.errstate(invalid="ignore"):
        s = np.minimum(np.ldexp(np.abs(v), (127 - b)[:, None]), 6.0)
        # a tie between codes i and i+1 goes to the even one: up iff i is odd
        code = sum((s >= t) if i % 2 else (s > t) for i, t in enumerate(TIES))
    q = (code | (np.signbit(v) << 3)).astype(np.uint8)
    q[nan] = 0
    b = np.where(nan, 255, b)
    return np.concatenate([(q[:, 0::2] | (q[:, 1::2] << 4)).ravel(), b.astype(np.uint8)])


def mx4_unpack_ref(buf: np.ndarray, n: int) -> np.ndarray:
    """wire bytes -> the decoded values in float64 (exact; NaN under 0xff)."""
    nblk = -(-n // 32)
    p = buf[: 16 * nblk].reshape(nblk, 16)
    q = np.stack([p & 15, p >> 4], axis=2).reshape(nblk, 32)
    b = buf[16 * nblk:].astype(np.int64)[:, None]
    x = np.ldexp(np.where(q & 8, -1.0, 1.0) * E2M1[q & 7], b - 127)
    return np.where(b == 255, np.nan, x).ravel()[:n]


def axpby_ref(a: torch.Tensor, wire: np.ndarray, dst_dtype) -> torch.Tensor:
    """round(fmaf(a, alpha, fl32(x^ * beta))), x^ in fp32.  The inputs keep
    the float64 sum exact, so its rounding to fp32 is the FMA's."""
    with np.errstate(over="ignore", invalid="ignore"):
        xh = mx4_unpack_ref(wire, a.numel()).astype(np.float32).astype(np.float64)
        p = (xh * BETA).astype(np.float32).astype(np.float64)
        r = a.to(torch.float64).numpy() * ALPHA + p
        return to_dtype(r.astype(np.float32).astype(np.float64), dst_dtype)


def encode_inputs() -> torch.Tensor:
    """Whole blocks of fp32: both sides of the scale rule's boundary at the
    ends and the middle of the exponent range, every scaled tie with its
    neighbours and both signs (amax 6 has b = 127: the scaled value is x),
    and the specials."""
    frac = np.array([1.0, -0.75, 0.5, -0.3, 0.1, -0.01, 1e-3, -1e-5] * 4, np.float32)
    blocks = [np.array([e << 23 | m], np.uint32).view(np.float32) * frac
              for e in (0, 1, 2, 3, 127, 128, 253, 254) for m in (0x400000, 0x400001)]
    t = TIES.astype(np.float32)
    t = np.concatenate([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(9))])
    for half in (t[:11], t[11:]):
        blocks.append(np.concatenate([[6.0], half, -half, np.zeros(31 - 2 * half.size)]))
    inf, nan = float("inf"), float("nan")
    for head in ([0.0], [1e-40, -1e-41], [-0.0, 6.0, -0.1], [inf, -inf, 2.0, -0.3],
                 [nan, 1.0], [nan] * 32):
        blocks.append(np.array(head + [0.0] * (32 - len(head))))
    return torch.from_numpy(np.concatenate(blocks).astype(np.float32))


def decode_inputs():
    """All 256 payload bytes under each of SCALES: (wire buffer, numel)."""
    payload = np.tile(np.arange(256, dtype=np.uint8), len(SCALES))
    return np.concatenate([payload, np.repeat(np.array(SCALES, np.uint8), 16)]), 5120


def axpby_operand(wire: np.ndarray, n: int) -> torch.Tensor:
    """fp32 accumulators k * 2^(b-137), |k| < 2^20 (b capped, to stay
    finite): within 2^24 of the decoded values, so the float64 sum is exact."""
    b = np.repeat(wire[n // 2:].astype(np.int64), 32)[:n]
    k = np.random.default_rng(7).integers(-(1 << 20), 1 << 20, n).astype(np.float64)
    return torch.from_numpy(np.ldexp(k, np.minimum(b, 230) - 137).astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_torch_codec_equals_reference(dtype):
    x = encode_inputs().to(dtype)
    got = mx4_pack_torch(x).numpy()
    want = mx4_pack_ref(x.to(F32).numpy())
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    wire, n = decode_inputs()
    assert_same(mx4_unpack_torch(torch.from_numpy(wire), n, dtype),
                to_dtype(mx4_unpack_ref(wire, n), dtype), "unpack")
    for a_dtype in DTYPES:
        a = axpby_operand(wire, n).to(a_dtype)
        assert_same(mx4_axpby_torch(a, torch.from_numpy(wire), ALPHA, BETA, out_dtype=dtype),
                    axpby_ref(a, wire, dtype), f"axpby from {a_dtype}")


def test_hand_worked_scale_bytes_and_sizes():
    heads = ([0.0], [float("nan"), 1.0], [float("inf"), float("-inf"), 2.0], [6.0, -0.25],
             [6.0000005])
    x = torch.tensor([h + [0.0] * (32 - len(h)) for h in heads]).reshape(-1)
    for pack in (mx4_pack_torch(x).numpy(), mx4_pack_ref(x.numpy())):
        assert pack[80:].tolist() == [0, 255, 126, 127, 128]
        assert pack[48] == 0x87 and not pack[16:32].any()
    for n in (1, 32, 33):
        assert wire_nbytes("mxfp4", n) == mx4_nbytes(n) == 17 * -(-n // 32)
        assert mx4_pack_torch(x[:n]).numel() == mx4_nbytes(n)
        assert wire_nbytes("mxfp8", n) == wire_nbytes("mxint8", n) == 33 * -(-n // 32)


def test_plan_two_ranks_forwarding_node_bit_identical(tmp_path):
    assert "MXFP4-PLAN-OK" in _torchrun("tests/mxfp4_plan_script.py", 2, tmp_path, timeout=180)


def test_relative_error_is_the_documented_figure():
    """docs/mxwire.md quotes 0.115 per hop on randn (65,536 blocks, seed 0)."""
    x = np.random.default_rng(0).standard_normal(65536 * 32).astype(np.float32)
    dec = mx4_unpack_ref(mx4_pack_ref(x), x.size)
    rel = np.linalg.norm(dec - x) / np.linalg.norm(x.astype(np.float64))
    print(f"relative L2 of MXFP4 on randn: {rel:.4f}")
    assert abs(rel - 0.115) < 0.0005
    b = np.repeat(mx4_pack_ref(x)[x.size // 2:].astype(np.int64), 32)
    assert np.all(np.abs(dec - x) <= np.maximum(0.25 * np.abs(x), np.ldexp(1.0, b - 129)))
