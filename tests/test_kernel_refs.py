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


# ---------------------------------------------------------------------------
# the combine contract: fma_ref against exact rationals, and the input sets
# ---------------------------------------------------------------------------
import math
from fractions import Fraction

import kernel_refs as kr
from kernel_refs import BF16, F16, F32, FLOATS3

# (stored mantissa bits, exponent bits)
_FMT = {F32: (23, 8), F16: (10, 5), BF16: (7, 8)}


def _round_fraction(v: Fraction, neg_zero: bool, dtype) -> int:
    """Bit pattern of the exact rational v rounded once, to nearest even,
    to ``dtype``: subnormals, overflow to Inf; a zero takes ``neg_zero``."""
    mb, eb = _FMT[dtype]
    bias = (1 << (eb - 1)) - 1
    if v == 0:
        return int(neg_zero) << (mb + eb)
    sign = int(v < 0) << (mb + eb)
    m = abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    e -= Fraction(2) ** e > m                         # 2^e <= m < 2^(e+1)
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1)
    e = max(e, 1 - bias)
    k = m / Fraction(2) ** (e - mb)                   # in units of the last place
    n = k.numerator // k.denominator
    rem = k - n
    n += rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1)
    if n == 1 << (mb + 1):
        n, e = n >> 1, e + 1
    if e > bias:
        return sign | ((1 << eb) - 1) << mb           # Inf
    if n < 1 << mb:
        return sign | n                               # subnormal or zero
    return sign | (e + bias) << mb | (n - (1 << mb))


def _from_bits32(b: int) -> float:
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])


def _fma_fraction(a: float, alpha: float, x: float, beta: float, dtype, two_step: bool):
    """One element of the contract in exact rational arithmetic; None = NaN."""
    if not all(map(math.isfinite, (a, alpha, x, beta))):
        r = a * alpha + x * beta                      # Inf or NaN: no rounding in it
        assert not math.isfinite(r)
        return None if math.isnan(r) else _round_fraction(Fraction(0), False, dtype) | \
            (int(r < 0) << sum(_FMT[dtype])) | ((1 << _FMT[dtype][1]) - 1) << _FMT[dtype][0]
    pneg = math.copysign(1, x) * math.copysign(1, beta) < 0
    p = _from_bits32(_round_fraction(Fraction(x) * Fraction(beta), pneg, F32))
    tneg = math.copysign(1, a) * math.copysign(1, alpha) < 0
    if math.isinf(p):
        v32 = p
    else:
        t = Fraction(a) * Fraction(alpha)
        v = t + Fraction(p)
        # an exact zero sum is +0 unless both terms are negative zeros
        vneg = (tneg and math.copysign(1, p) < 0) if (t == 0 and p == 0) else False
        if not two_step:
            return _round_fraction(v, vneg, dtype)
        v32 = _from_bits32(_round_fraction(v, vneg, F32))
    if math.isinf(v32):
        return int(v32 < 0) << sum(_FMT[dtype]) | ((1 << _FMT[dtype][1]) - 1) << _FMT[dtype][0]
    return _round_fraction(Fraction(v32), math.copysign(1, v32) < 0, dtype)


def _check_against_fraction(a, alpha, x, beta, what):
    a64, x64 = kr._as_f64(a), kr._as_f64(x)
    al, be = float(np.float32(alpha)), float(np.float32(beta))
    # every element, each distinct (a, x) pair worked once (fma_ref is
    # elementwise; the scale_shift sets repeat some twenty pairs)
    pairs = np.stack([a64.view(np.int64), x64.view(np.int64)], axis=1)
    uniq, first, inv = np.unique(pairs, axis=0, return_index=True, return_inverse=True)
    for dtype in FLOATS3:
        for two_step in (True, False):
            bits, nan = kr.fma_ref(a, alpha, x, beta, dtype, two_step)
            for i in first:
                want = _fma_fraction(float(a64[i]), al, float(x64[i]), be, dtype, two_step)
                if want is None:
                    assert nan[i], (what, dtype, two_step, i)
                else:
                    assert not nan[i] and int(bits[i]) == want, (
                        what, dtype, two_step, i, a64[i], x64[i], hex(int(bits[i])), hex(want))
            same = first[inv.reshape(-1)]             # equal inputs, equal outputs
            assert (nan == nan[same]).all() and (bits[~nan] == bits[same][~nan]).all()


@pytest.mark.parametrize("mid", [F16, BF16], ids=["f16", "bf16"])
def test_fma_ref_equals_exact_rationals_on_dr_sets(mid):
    a, alpha, x, beta = kr.dr_axpby_set(mid)
    _check_against_fraction(a, alpha, x, beta, "dr_axpby")
    for src in FLOATS3:
        for xs, sa, sb in kr.dr_scale_shift_sets(mid, src):
            _check_against_fraction(xs, sa, np.full(xs.size, sb), 1.0,
                                    f"dr_scale_shift {src}")


@pytest.mark.parametrize("src", FLOATS3, ids=["f32", "bf16", "f16"])
def test_fma_ref_equals_exact_rationals_on_inexact_and_specials(src):
    a, x = kr.inexact_set(src)
    for alpha, beta in kr.INEXACT_SCALARS:
        _check_against_fraction(a, alpha, x, beta, "inexact")
    for name, sa, sx, alpha, beta in kr.specials_runs(src):
        _check_against_fraction(sa, alpha, sx, beta, name)


def test_fma_ref_known_values():
    """Hand-worked: 1 + 2^-11 + 2^-27 is just above the f16 tie between 1
    and 1 + 2^-10; fp32 drops the 2^-27, and the tie then goes to 1."""
    one = np.array([1.0])
    beta = 2.0 ** -11 * (1 + 2.0 ** -16)
    assert kr.fma_ref(one, 1.0, one, beta, F16)[0][0] == 0x3C00
    assert kr.fma_ref(one, 1.0, one, beta, F16, two_step=False)[0][0] == 0x3C01
    assert kr.fma_ref(one, 1.0, one, beta, F32)[0][0] == 0x3F801000
    # fma(0, 0, -0.0) = +0.0; -0 + -0 = -0; 65520 is the f16 tie that goes to Inf
    z = np.array([0.0])
    assert kr.fma_ref(z, 0.0, -z, 1.0, F16)[0][0] == 0x0000
    assert kr.fma_ref(-z, 1.0, -z, 1.0, F16)[0][0] == 0x8000
    assert kr.fma_ref(one, 65504.0, np.array([2.0]), 8.0, F16)[0][0] == 0x7C00
    assert kr.fma_ref(one, 65504.0, np.array([2.0]), 7.995, F16)[0][0] == 0x7BFF
    assert kr.fma_ref(z, 1.0, z, float("inf"), BF16)[1][0]


@pytest.mark.parametrize("mid", [F16, BF16], ids=["f16", "bf16"])
def test_dr_sets_split_the_two_roundings(mid):
    """At least a quarter of every DR set rounds differently in two steps
    and in one (the constructions give about half), for the destination
    whose midpoints it sits on; the other destinations do not notice."""
    a, alpha, x, beta = kr.dr_axpby_set(mid)
    assert kr.dr_disagreement(a, alpha, x, beta, mid) >= 0.25
    for prefix in (7, 33, 4101):      # the GPU shapes are prefixes of the set
        assert kr.dr_disagreement(a[:prefix], alpha, x[:prefix], beta, mid) >= 0.25
    assert kr.dr_disagreement(a, alpha, x, beta, F32) == 0.0
    for src in FLOATS3:
        sets = kr.dr_scale_shift_sets(mid, src)
        assert len(sets) >= 2
        for xs, sa, sb in sets:
            b = np.full(xs.size, sb)
            assert kr.dr_disagreement(xs, sa, b, 1.0, mid) >= 0.25
            assert kr.dr_disagreement(xs[:9], sa, b[:9], 1.0, mid) >= 0.25
            t = torch.from_numpy(xs).to(src)
            assert torch.equal(t.double(), torch.from_numpy(xs))     # exact in the source


@pytest.mark.parametrize("mid", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("codec", kr.MX_CODECS)
def test_dr_operand_is_exact_on_every_wire(codec, mid):
    x = torch.from_numpy(kr.dr_axpby_set(mid)[2])
    for n in (7, 8, 9, 33, 2500, 4096, 4097, 4088, 4101, kr.COMBINE_N):
        wire = kr.mx_pack_ref(codec, x[:n].to(F32))
        assert (kr.mx_decode_ref(codec, wire, n) == x[:n].numpy()).all(), (codec, n)


def test_inexact_set_rounds_the_product_and_the_sum():
    for src in FLOATS3:
        a, x = kr.inexact_set(src)
        for alpha, beta in kr.INEXACT_SCALARS:
            prod = x.double().numpy() * float(np.float32(beta))
            assert (prod.astype(np.float32).astype(np.float64) != prod).mean() > 0.9
            two, _ = kr.fma_ref(a, alpha, x, beta, F16)
            one, _ = kr.fma_ref(a, alpha, x, beta, F16, two_step=False)
            assert (two != one).mean() < 0.01          # generic values: rare


def test_specials_reach_what_they_claim():
    runs = {r[0]: r for r in kr.specials_runs(F32)}
    bits, nan = kr.fma_ref(*[runs["cross"][i] for i in (1, 3, 2, 4)], F16)
    assert nan.any() and (bits[~nan] == 0x7C00).any() and (bits[~nan] == 0xFC00).any()
    assert (bits[~nan] == 0x8000).any() and (bits[~nan] == 0x0000).any()
    assert kr.fma_ref(*[runs["cross-inf"][i] for i in (1, 3, 2, 4)], F16)[1].sum() > nan.sum()
    for name, dtype, lo in (("f16sub", F16, 2.0 ** -14), ("bf16sub", BF16, 2.0 ** -126)):
        b, _ = kr.fma_ref(*[runs[name][i] for i in (1, 3, 2, 4)], dtype)
        v = kr.from_bits(b, dtype).double().abs()
        assert ((v > 0) & (v < lo)).sum() > 100        # subnormal results
    e, _ = kr.fma_ref(*[runs["edge"][i] for i in (1, 3, 2, 4)], F16)
    assert {0x7BFF, 0x7C00, 0xFBFF, 0xFC00} <= set(e.tolist())
    for src in FLOATS3:
        r = {r[0]: r for r in kr.specials_runs(src)}["ovf"]
        b, n = kr.fma_ref(r[1], r[3], r[2], r[4], F32)
        # each term is finite in fp32, only the sum overflows; max - max is +0
        assert not n.any() and set(b.tolist()) >= {0x7F800000, 0xFF800000, 0}
