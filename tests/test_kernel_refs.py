"""CPU tests of the host references in kernel_refs.py (no GPU needed).

The GPU suite trusts these references, so they are pinned here against
published constants, against structural properties every byte-covering
digest must have, and against an independent brute-force rounding."""
import numpy as np
import pytest
import torch

from kernel_refs import (
    FP8_MAX,
    all_bits16,
    all_codes8,
    checksum_mfma_ref,
    checksum_valu_ref,
    fill_pattern_ref,
    fp8_cast_ref,
    fp8_nearest_bruteforce,
    mfma_grid_blocks,
    narrowing_boundaries,
    splitmix64,
)

CHECKSUMS = [checksum_valu_ref, checksum_mfma_ref]
CHECKSUM_IDS = ["valu", "mfma"]


def _buffer() -> bytes:
    rng = np.random.default_rng(1234)
    return rng.integers(0, 256, size=3 * 1024 + 13, dtype=np.uint8).tobytes()


def test_splitmix64_published_vector():
    # first outputs of the reference splitmix64 generator seeded with 0
    assert int(splitmix64(0)) == 0xE220A8397B1DCDAF
    got = splitmix64(np.array([0, 0x9E3779B97F4A7C15], dtype=np.uint64))
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


@pytest.mark.parametrize("ref", CHECKSUMS, ids=CHECKSUM_IDS)
def test_checksum_ref_has_no_dead_byte(ref):
    data = _buffer()
    base = ref(data)
    assert 0 <= base < (1 << 64)
    for i in range(len(data)):
        flipped = bytearray(data)
        flipped[i] ^= 0xFF
        assert ref(bytes(flipped)) != base, f"byte {i} does not reach the digest"


@pytest.mark.parametrize("ref", CHECKSUMS, ids=CHECKSUM_IDS)
def test_checksum_ref_length_and_position(ref):
    data = _buffer()
    base = ref(data)
    assert ref(data + b"\0") != base
    zeros = bytes(len(data))
    assert ref(zeros + b"\0") != ref(zeros)
    # swap two unequal 16-byte granules: inside one tile, across tiles, and
    # between the last full tile and the tail
    for ga, gb in [(0, 1), (3, 64 + 3), (5, 130), (191, 192)]:
        a, b = data[16 * ga:16 * ga + 16], data[16 * gb:16 * gb + 16]
        assert a != b
        sw = bytearray(data)
        sw[16 * ga:16 * ga + 16], sw[16 * gb:16 * gb + 16] = b, a
        assert ref(bytes(sw)) != base, (ga, gb)


def test_checksum_mfma_ref_models_the_launch_grid():
    """The MFMA digest folds one accumulator per wave, so it is a function
    of the bytes and of how many waves the launcher starts."""
    data = _buffer() * 8   # 24 tiles: the launcher wants 2 blocks
    assert mfma_grid_blocks(len(data)) == 2
    assert mfma_grid_blocks(len(data), max_blocks=1) == 1
    assert mfma_grid_blocks(65536) == 4 and mfma_grid_blocks(1023) == 1
    assert checksum_mfma_ref(data, max_blocks=1) != checksum_mfma_ref(data, max_blocks=2)
    assert checksum_mfma_ref(data, max_blocks=2) == checksum_mfma_ref(data)


def test_fill_pattern_ref_words_and_tail():
    full = fill_pattern_ref(64, seed=42)
    w = np.frombuffer(full, dtype="<u8")
    assert int(w[3]) == int(splitmix64(np.uint64(42 ^ 3)))
    for nb in (0, 2, 4, 6, 8, 62):
        assert fill_pattern_ref(nb, seed=42) == full[:nb]
    masked = np.frombuffer(fill_pattern_ref(64, 42, 0x3FFF), dtype="<u2")
    assert (masked == (np.frombuffer(full, dtype="<u2") & 0x3FFF)).all()
    assert fill_pattern_ref(16, (1 << 63) + 5) != fill_pattern_ref(16, 5)


@pytest.mark.parametrize("dtype", list(FP8_MAX), ids=["e4m3fn", "e5m2"])
def test_fp8_cast_ref_is_nearest_even_saturating(dtype):
    x = narrowing_boundaries(dtype)
    want = fp8_nearest_bruteforce(x, dtype)
    got = fp8_cast_ref(x, dtype)
    nan = torch.isnan(x)
    assert torch.isnan(got.float()[nan]).all()
    assert not torch.isnan(got.float()[~nan]).any()
    assert not torch.isinf(got.float()).any()
    assert torch.equal(got.view(torch.uint8)[~nan], want[~nan])
    # saturation, not torch's NaN/Inf, past the largest finite value
    m = FP8_MAX[dtype]
    big = torch.tensor([m * 1.5, -m * 1.5, 3e38, float("inf")])
    assert fp8_cast_ref(big, dtype).float().tolist() == [m, -m, m, m]


@pytest.mark.parametrize(
    "dtype", [torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2],
    ids=["f16", "bf16", "e4m3fn", "e5m2"],
)
def test_boundary_sets_cover_values_ties_and_specials(dtype):
    x = narrowing_boundaries(dtype)
    xs = set(x[torch.isfinite(x)].double().tolist())
    if dtype in FP8_MAX:
        vals = all_codes8(dtype).float()
    else:
        vals = all_bits16(dtype).float()
    vals = vals[torch.isfinite(vals)].double()
    assert set(vals.tolist()) <= xs
    pos = torch.unique(vals[vals >= 0])
    mids = (pos[:-1] + pos[1:]) / 2
    assert set(mids.tolist()) <= xs and set((-mids).tolist()) <= xs
    assert torch.isnan(x).any() and torch.isinf(x).sum() >= 2
    assert (x == 0).sum() >= 2 and torch.signbit(x[x == 0]).any()
    assert float(x[torch.isfinite(x)].max()) > 1e38
    tiny = x[(x != 0) & (x.abs() < 1.1754944e-38)]
    assert tiny.numel() >= 4                      # f32 subnormals
    assert all_bits16(torch.float16).view(torch.int16).unique().numel() == 65536
