"""Data-plane HIP kernels pinned to exact host references (MI355X, gfx950).

Inputs are built on the CPU (seeded where random), expected values are
computed on the CPU from the operation's definition (kernel_refs.py, torch
CPU casts, integer sums); the kernels are never their own oracle.  Sizes
are tiny: the grid is capped with lz_set_max_blocks(k) so that the
grid-stride loops wrap, the unrolled and non-unrolled trips and the scalar
tails all run at a few thousand elements.  These tests REQUIRE the native
extension: a missing libhipops.so fails loudly."""
import functools
import itertools
import math
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from kernel_refs import (
    FP8_MAX,
    LZ_BLOCK,
    LZ_MAX_BLOCKS,
    all_bits16,
    all_codes8,
    checksum_mfma_ref,
    checksum_valu_ref,
    fill_pattern_ref,
    fp8_cast_ref,
    narrowing_boundaries,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
U8, I32, I64, F64 = torch.uint8, torch.int32, torch.int64, torch.float64
FLOATS3 = [F32, F16, BF16]
NAMES = {F32: "f32", F16: "f16", BF16: "bf16", E4M3: "e4m3", E5M2: "e5m2",
         U8: "u8", I32: "i32", I64: "i64", F64: "f64"}

# grid caps every grid-sensitive test runs under; 0 = the default cap
GRIDS = [1, 2, 0]


def _pair_id(p):
    return "-".join(NAMES[d] for d in p)


@pytest.fixture(scope="module", autouse=True)
def _native():
    import lzy_amd.ops as ops

    if torch.cuda.is_available():
        assert ops.NATIVE, "HIP ops must be built+loadable on a GPU box"
    yield


@contextmanager
def _capped(k):
    import lzy_amd.ops as ops

    lib = ops._require_native()
    lib.lz_set_max_blocks(k)
    try:
        yield
    finally:
        lib.lz_set_max_blocks(0)


def _threads(k):
    """Threads of a grid capped at k blocks (the default cap is never
    reached at these sizes; its cases reuse the k=2 sizes)."""
    return LZ_BLOCK * (k if k else 2)


def _grid_n(V, U, k):
    """Two unrolled trips, a partial non-unrolled trip and a full scalar
    tail for a kernel of V elements per vector and unroll U."""
    T = _threads(k)
    return V * (2 * U * T + T + 37) + (V - 1)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32,
                                8: torch.int64}[t.element_size()])


def _isnan(t):
    if not t.dtype.is_floating_point:
        return torch.zeros(t.shape, dtype=torch.bool)
    return torch.isnan(t.double() if t.dtype == F64 else t.float())


def _assert_same_bits(got, want, what, skip=None):
    """Bytes equal; NaN positions compared by NaN-ness, not payload."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = _isnan(got), _isnan(want)
    keep = ~wn if skip is None else ~wn & ~skip
    if skip is not None:
        gn, wn = gn & ~skip, wn & ~skip
    assert torch.equal(gn, wn), f"{what}: NaN positions differ at {(gn != wn).nonzero()[:8].flatten().tolist()}"
    bad = (_bits(got) != _bits(want)) & keep
    if bad.any():
        idx = bad.nonzero().flatten()[:8]
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at "
            f"{idx.tolist()}: got bits {_bits(got)[idx].tolist()} want {_bits(want)[idx].tolist()}"
        )


# ---------------------------------------------------------------------------
# checksums
# ---------------------------------------------------------------------------

def _fills(nbytes, seed):
    rng = np.random.default_rng(seed)
    return [
        ("random", rng.integers(0, 256, size=nbytes, dtype=np.uint8)),
        ("zeros", np.zeros(nbytes, dtype=np.uint8)),
        ("ones", np.full(nbytes, 0xFF, dtype=np.uint8)),
    ]


@requires_gpu
@pytest.mark.parametrize("k", GRIDS)
def test_checksum_valu_equals_reference(k):
    from lzy_amd.ops import device_checksum

    T = _threads(k)
    sizes = list(range(49)) + [16 * (3 * T + 37) + 8 + j for j in range(8)]
    with _capped(k):
        for nb in sizes:
            for name, arr in _fills(nb, seed=nb):
                got = device_checksum(torch.from_numpy(arr).cuda(), method="valu")
                assert got == checksum_valu_ref(arr.tobytes()), (nb, name)


@requires_gpu
@pytest.mark.parametrize("k", GRIDS)
def test_checksum_mfma_equals_reference(k):
    from lzy_amd.ops import device_checksum

    cap = k if k else LZ_MAX_BLOCKS
    with _capped(k):
        for ntiles, rem in itertools.product([0, 1, 4, 5, 16, 17, 39],
                                             [0, 1, 7, 8, 9, 1023]):
            nb = 1024 * ntiles + rem
            for name, arr in _fills(nb, seed=nb):
                got = device_checksum(torch.from_numpy(arr).cuda(), method="mfma")
                want = checksum_mfma_ref(arr.tobytes(), max_blocks=cap)
                assert got == want, (ntiles, rem, name)


@requires_gpu
def test_checksum_auto_switches_at_64k():
    from lzy_amd.ops import device_checksum

    with _capped(0):
        for nb, ref in [(65535, checksum_valu_ref), (65536, checksum_mfma_ref)]:
            arr = _fills(nb, seed=nb)[0][1]
            assert device_checksum(torch.from_numpy(arr).cuda()) == ref(arr.tobytes()), nb


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16, I64], ids=["f32", "bf16", "i64"])
def test_checksum_covers_the_bytes_of_any_dtype(dtype):
    """The digest is over the tensor's bytes in memory order, whatever the
    dtype and shape say."""
    from lzy_amd.ops import device_checksum

    arr = _fills(5 * 1024 + 40, seed=77)[0][1]
    t = torch.from_numpy(arr).view(dtype)
    assert _bits(t).numpy().tobytes() == arr.tobytes()
    with _capped(0):
        d = t.cuda()
        assert device_checksum(d) == checksum_valu_ref(arr.tobytes())
        assert device_checksum(d.view(-1, 5), method="valu") == checksum_valu_ref(arr.tobytes())
        assert device_checksum(d, method="mfma") == checksum_mfma_ref(arr.tobytes())


# ---------------------------------------------------------------------------
# reductions: exact on integer-valued data
# ---------------------------------------------------------------------------

# (V, U) of lz_stats per element size, and of the ten lz_stats_variant shapes
STATS_VU = {2: (16, 4), 4: (8, 4)}
VARIANT_VU = {
    2: [(16, 4), (16, 8), (32, 2), (32, 4), (8, 8), (16, 2), (8, 4), (16, 4), (8, 8), (16, 2)],
    4: [(8, 4), (8, 8), (16, 2), (16, 4), (4, 8), (8, 2), (4, 4), (8, 4), (16, 4), (8, 2)],
}
INT_MAX_ABS = 64


@functools.lru_cache(maxsize=None)
def _int_data(n):
    """Integer-valued samples in [-64, 64] and their exact sums."""
    x = np.random.default_rng(n).integers(-INT_MAX_ABS, INT_MAX_ABS + 1, size=n)
    return x, int(x.sum()), int(np.abs(x).sum()), int((x * x).sum())


def _assert_lane_partials_exact(n, V, k, max_abs=INT_MAX_ABS):
    """No f32 lane partial can reach 2^24 (so every f32 add, the f64 folds
    and the f64 atomics are exact): a lane takes at most ceil(vec_n / T)
    vectors and ceil(tail / T) tail elements, T = threads in the grid."""
    want = max(1, -(-(n // 8) // LZ_BLOCK))
    T = LZ_BLOCK * min(want, k if k else LZ_MAX_BLOCKS)
    per_lane = V * -(-(n // V) // T) + -(-(n % V) // T)
    assert per_lane * max_abs * max_abs < 2 ** 24, (n, V, k)
    assert n * max_abs * max_abs < 2 ** 53


def _stats_sizes(V, U, k):
    T = _threads(k)
    return [_grid_n(V, U, k), 1, 7, 8, 9, V * T - 1, V * T, V * T + 1]


@requires_gpu
@pytest.mark.parametrize("k", GRIDS)
@pytest.mark.parametrize("dtype", FLOATS3, ids=["f32", "f16", "bf16"])
def test_stats_exact_on_integers(dtype, k):
    from lzy_amd.ops import abs_mean, mean_std, stats

    V, U = STATS_VU[torch.empty(0, dtype=dtype).element_size()]
    with _capped(k):
        for n in _stats_sizes(V, U, k):
            _assert_lane_partials_exact(n, V, k)
            x, s, sa, s2 = _int_data(n)
            t = torch.from_numpy(x).to(dtype).cuda()
            assert stats(t).cpu().tolist() == [float(s), float(s2)], n
            assert stats(t, use_abs=True).cpu().tolist() == [float(sa), float(s2)], n
            assert abs_mean(t) == sa / n, n
            mean = s / n
            var = s2 / n - mean * mean
            assert mean_std(t) == (mean, math.sqrt(max(var, 0.0))), n
            if n > 1:
                ub = var * (n / (n - 1))
                assert mean_std(t, unbiased=True) == (mean, math.sqrt(max(ub, 0.0))), n


@requires_gpu
@pytest.mark.parametrize("variant", range(10))
@pytest.mark.parametrize("dtype", FLOATS3, ids=["f32", "f16", "bf16"])
def test_stats_variants_exact_on_integers(dtype, variant):
    from lzy_amd.ops import stats_variant

    V, U = VARIANT_VU[torch.empty(0, dtype=dtype).element_size()][variant]
    for k in GRIDS:
        with _capped(k):
            for n in _stats_sizes(V, U, k):
                _assert_lane_partials_exact(n, V, k)
                x, s, sa, s2 = _int_data(n)
                t = torch.from_numpy(x).to(dtype).cuda()
                assert stats_variant(t, variant).cpu().tolist() == [float(s), float(s2)], (k, n)
                assert stats_variant(t, variant, use_abs=True).cpu().tolist() == \
                    [float(sa), float(s2)], (k, n)


@requires_gpu
def test_stats_randn_within_tolerance():
    from lzy_amd.ops import stats

    g = torch.Generator().manual_seed(3)
    x = torch.randn(_grid_n(8, 4, 2), generator=g)
    ref = x.double()
    with _capped(2):
        s = stats(x.cuda()).cpu()
    assert abs(float(s[0]) - float(ref.sum())) <= 1e-3 * max(1.0, abs(float(ref.sum())))
    assert abs(float(s[1]) - float((ref * ref).sum())) <= 1e-3 * float((ref * ref).sum() + 1)


# ---------------------------------------------------------------------------
# cast_copy: bit-exact on boundary sets
# ---------------------------------------------------------------------------

def _run_cast(src_cpu, dst_dtype):
    from lzy_amd.ops import cast_copy

    src = src_cpu.cuda()
    dst = torch.empty(src.shape, dtype=dst_dtype, device="cuda")
    cast_copy(src, dst)
    return dst.cpu()


def _via_f32(src_cpu, dst_dtype):
    """The kernel's route for every pair with a 16- or 8-bit float: widen to
    f32 (exact), then one round-to-nearest-even narrowing; fp8 saturates."""
    f = src_cpu.to(F32)
    return fp8_cast_ref(f, dst_dtype) if dst_dtype in FP8_MAX else f.to(dst_dtype)


def _check_fp8_inf(src_f32, got, dst_dtype, what):
    """+-Inf into fp8 is the hardware convert's answer, not the project's:
    e4m3fn may give NaN or +-max, e5m2 +-Inf or +-max (sign kept)."""
    inf = torch.isinf(src_f32)
    if not inf.any():
        return inf
    g, s = got.float()[inf], src_f32[inf]
    m = FP8_MAX[dst_dtype]
    sat = g == torch.sign(s) * m
    other = torch.isnan(g) if dst_dtype == E4M3 else (g == s)
    print(f"{what}: Inf -> {g.tolist()} (bits {_bits(got)[inf].tolist()})")
    assert (sat | other).all(), f"{what}: Inf gave {g.tolist()}"
    return inf


@requires_gpu
@pytest.mark.parametrize("pair", [(F16, F32), (F16, BF16), (BF16, F32), (BF16, F16)],
                         ids=_pair_id)
def test_cast_all_16bit_patterns(pair):
    src = all_bits16(pair[0])
    _assert_same_bits(_run_cast(src, pair[1]), _via_f32(src, pair[1]), _pair_id(pair))


@requires_gpu
@pytest.mark.parametrize("pair", list(itertools.product([E4M3, E5M2], FLOATS3)),
                         ids=_pair_id)
def test_cast_all_fp8_codes(pair):
    src = all_codes8(pair[0])
    _assert_same_bits(_run_cast(src, pair[1]), _via_f32(src, pair[1]), _pair_id(pair))


@requires_gpu
@pytest.mark.parametrize("dst", [F16, BF16], ids=["f16", "bf16"])
def test_cast_f32_narrowing_ties(dst):
    x = narrowing_boundaries(dst)
    _assert_same_bits(_run_cast(x, dst), x.to(dst), f"f32-{NAMES[dst]}")


@requires_gpu
@pytest.mark.parametrize("pair", list(itertools.product(FLOATS3, [E4M3, E5M2])),
                         ids=_pair_id)
def test_cast_to_fp8_ties_and_saturation(pair):
    """Mismatch share 0 against round-to-nearest-even with finite
    saturation, on every tie and on both sides of it."""
    src_dtype, dst = pair
    src = narrowing_boundaries(dst) if src_dtype == F32 else all_bits16(src_dtype)
    got = _run_cast(src, dst)
    inf = _check_fp8_inf(src.float(), got, dst, _pair_id(pair))
    _assert_same_bits(got, fp8_cast_ref(src.float(), dst), _pair_id(pair), skip=inf)


_I32_VALS = [0, 1, -1, 255, 256, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, -(2 ** 24 + 1),
             123456789, -987654321, 2 ** 31 - 1, -(2 ** 31)]
_I64_VALS = _I32_VALS + [2 ** 31, -(2 ** 31) - 1, 2 ** 32 + 5, 2 ** 53 - 1, -(2 ** 53 - 1),
                         2 ** 53, 2 ** 53 + 1, 2 ** 62 + 1, 2 ** 63 - 1, -(2 ** 63)]
_F64_VALS = [0.0, -0.0, 1.0, 0.1, -1.0 / 3.0, 1.0 + 2.0 ** -52, float(2 ** 53 - 1),
             -float(2 ** 53 - 1), 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52,
             1.0 + 3 * 2.0 ** -24, 16777217.0, 3.4028235677973366e38, 1e300, -1e300,
             1e-300, 1e-40, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -150,
             float("nan"), float("inf"), float("-inf")]
_SMALL_INT_VALS = [0, 1, -1, 255, 257, 2047, 2049, -2049, 65504, 65519, 65520, 70000,
                   2 ** 24 - 1, -(2 ** 24 - 1)]
_F32_TO_INT = {
    I32: [0.0, -0.0, 0.5, -0.5, 0.99999994, 1.5, -1.5, 2.5, -2.5, 123456.7, 16777216.0,
          2147483520.0, -2147483648.0],
    I64: [0.0, 0.5, -0.5, 1.5, -1.5, 2147483648.0, -4294967296.0, 1e15,
          9223371487098961920.0, -9223372036854775808.0],
    U8: [0.0, 0.5, 0.999, 1.5, 2.5, 127.5, 254.5, 255.0, 255.9],
}

_ALL9 = [F32, F16, BF16, E4M3, E5M2, U8, I32, I64, F64]
_WIDE_PAIRS = (
    [(I32, I32), (I64, I64), (I32, I64), (I64, I32), (I32, F64), (I64, F64),
     (F64, F64), (F64, F32), (I32, F16), (I32, BF16), (I64, F16), (I64, BF16)]
    + [(U8, d) for d in _ALL9]
    + [(F32, I32), (F32, I64), (F32, U8)]
)


def _wide_input(pair):
    src, dst = pair
    if src == U8:
        return torch.arange(256, dtype=torch.int32).to(U8)
    if src == F32:
        return torch.tensor(_F32_TO_INT[dst], dtype=F32)
    if src == F64:
        return torch.tensor(_F64_VALS, dtype=F64)
    if dst in (F16, BF16):                      # int -> 16-bit float: |v| < 2^24
        return torch.tensor(_SMALL_INT_VALS, dtype=src)
    return torch.tensor(_I32_VALS if src == I32 else _I64_VALS, dtype=src)


@requires_gpu
@pytest.mark.parametrize("pair", _WIDE_PAIRS, ids=_pair_id)
def test_cast_integer_and_f64_pairs(pair):
    """Against torch's CPU .to(): direct conversion between plain types (no
    trip through f32), via f32 for 16- and 8-bit float targets."""
    src = _wide_input(pair)
    want = fp8_cast_ref(src.float(), pair[1]) if pair[1] in FP8_MAX else src.to(pair[1])
    # 8 copies + 5: the vector body and the scalar tail both see every value
    rep = torch.cat([src.repeat(8), src[:5]])
    wrep = torch.cat([want.repeat(8), want[:5]])
    _assert_same_bits(_run_cast(rep, pair[1]), wrep, _pair_id(pair))


@requires_gpu
@pytest.mark.parametrize("pair", [(F32, BF16), (F32, F16), (BF16, F32), (F16, BF16),
                                  (F32, E4M3), (BF16, E5M2), (E4M3, F16), (I32, I64),
                                  (I64, F64), (F64, F32)], ids=_pair_id)
def test_cast_sizes_and_capped_grid(pair):
    src_dtype, dst = pair
    if src_dtype in (F16, BF16):
        pool = all_bits16(src_dtype)
    elif src_dtype in FP8_MAX:
        pool = all_codes8(src_dtype)
    elif src_dtype == F32:
        pool = narrowing_boundaries(dst)
    else:
        pool = _wide_input(pair)
    if dst in FP8_MAX:                          # Inf -> fp8 is checked above
        pool = pool[~torch.isinf(pool.float())]
    for k in GRIDS:
        with _capped(k):
            for n in [1, 7, 8, 9, _grid_n(8, 1, k)]:
                # stride 7 walks the whole pool at any n
                src = pool[(torch.arange(n) * 7 + n) % pool.numel()]
                if dst in FP8_MAX or src_dtype in FP8_MAX or \
                        (src_dtype in (F16, BF16) and dst in (F16, BF16)):
                    want = _via_f32(src, dst)
                else:
                    want = src.to(dst)
                _assert_same_bits(_run_cast(src, dst), want, f"{_pair_id(pair)} k={k} n={n}")


# ---------------------------------------------------------------------------
# scale_shift / axpby: single fused rounding, predicted to the bit
# ---------------------------------------------------------------------------

SS_A, SS_B = 2.5, -1.25
AX_ALPHA, AX_BETA = 0.75, -1.5


@functools.lru_cache(maxsize=None)
def _few_bit_values(n, seed):
    """+-m * 2^e with an 8-bit m (so exact in bf16, f16 and f32; within the
    11 significant bits the proof needs) and |value| in [2^-8, 2^9).
    Returns (float64 values, the same scaled by 2^15 as exact int64)."""
    rng = np.random.default_rng(seed)
    m = rng.integers(128, 256, size=n)
    e = rng.integers(-8, 9, size=n)
    sign = rng.choice([-1, 1], size=n)
    scaled = sign * m * (1 << (e + 8))            # value * 2^15, integer
    return scaled.astype(np.float64) / 2.0 ** 15, scaled.astype(np.int64)


def _assert_fused_exact(scaled_terms, expr_f64):
    """expr_f64 == the exact rational value: scaled_terms are integers whose
    sum is value * 2^19, small enough for int64 and for 53 bits."""
    total = sum(scaled_terms)
    assert (np.abs(total) < 2 ** 53).all()
    assert (total.astype(np.float64) / 2.0 ** 19 == expr_f64).all()


def _fused_ref(expr_f64, dst_dtype):
    """round_dst(round_f32(exact)): the kernel's fmaf rounds the exact value
    once to f32, the store narrows that once more."""
    return torch.from_numpy(expr_f64).to(F32).to(dst_dtype)


_PAIRS9 = list(itertools.product(FLOATS3, FLOATS3))


@requires_gpu
@pytest.mark.parametrize("pair", _PAIRS9, ids=_pair_id)
def test_scale_shift_bit_exact(pair):
    from lzy_amd.ops import scale_shift

    src_dtype, dst_dtype = pair
    for k in GRIDS:
        for n in [1, 7, 8, 9, _grid_n(8, 1, k)]:
            x, xi = _few_bit_values(n, seed=11)
            expr = x * SS_A + SS_B
            # x*a: 8 x 3 significant bits, exact in f32 and f64; a*4, b*2^19 integers
            _assert_fused_exact([xi * int(SS_A * 4) * 4, np.int64(int(SS_B * 2 ** 19))], expr)
            src = torch.from_numpy(x).to(src_dtype)
            assert (src.double().numpy() == x).all()
            want = _fused_ref(expr, dst_dtype)
            with _capped(k):
                d = src.cuda()
                dst = torch.empty(n, dtype=dst_dtype, device="cuda")
                assert scale_shift(d, SS_A, SS_B, dst=dst) is dst
                _assert_same_bits(dst.cpu(), want, f"{_pair_id(pair)} k={k} n={n}")
                if src_dtype == dst_dtype:
                    out = scale_shift(d, SS_A, SS_B)
                    _assert_same_bits(out.cpu(), want, "new dst")
                    _assert_same_bits(d.cpu(), src, "src untouched")
                    assert scale_shift(d, SS_A, SS_B, dst=d) is d    # in place
                    _assert_same_bits(d.cpu(), want, f"in place k={k} n={n}")


@requires_gpu
@pytest.mark.parametrize("pair", _PAIRS9, ids=_pair_id)
def test_axpby_bit_exact(pair):
    from lzy_amd.ops import axpby

    src_dtype, dst_dtype = pair
    for k in GRIDS:
        for n in [1, 7, 8, 9, _grid_n(8, 1, k)]:
            x, xi = _few_bit_values(n, seed=21)
            y, yi = _few_bit_values(n, seed=22)
            yb = y * AX_BETA
            assert (yb.astype(np.float32).astype(np.float64) == yb).all()  # y*beta exact in f32
            expr = x * AX_ALPHA + yb
            _assert_fused_exact([xi * int(AX_ALPHA * 4) * 4, yi * int(AX_BETA * 2) * 8], expr)
            a = torch.from_numpy(x).to(src_dtype)
            b = torch.from_numpy(y).to(src_dtype)
            assert (a.double().numpy() == x).all() and (b.double().numpy() == y).all()
            with _capped(k):
                dst = torch.empty(n, dtype=dst_dtype, device="cuda")
                assert axpby(a.cuda(), b.cuda(), AX_ALPHA, AX_BETA, dst=dst) is dst
            _assert_same_bits(dst.cpu(), _fused_ref(expr, dst_dtype),
                              f"{_pair_id(pair)} k={k} n={n}")


# ---------------------------------------------------------------------------
# transpose_cast
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("pair", _PAIRS9, ids=_pair_id)
def test_transpose_cast_bit_exact(pair):
    from lzy_amd.ops import transpose_cast

    src_dtype, dst_dtype = pair
    g = torch.Generator().manual_seed(5)
    for rows, cols in [(64, 64), (128, 192), (65, 63), (1, 130), (130, 1), (63, 129)]:
        src = (torch.randn(rows, cols, generator=g) * 8).to(src_dtype)
        want = src.t().contiguous().to(dst_dtype)
        out = transpose_cast(src.cuda(), dtype=dst_dtype)
        assert out.shape == (cols, rows) and out.is_contiguous()
        _assert_same_bits(out.cpu(), want, f"{_pair_id(pair)} {rows}x{cols}")
        dst = torch.empty(cols, rows, dtype=dst_dtype, device="cuda")
        assert transpose_cast(src.cuda(), dst=dst) is dst
        _assert_same_bits(dst.cpu(), want, f"{_pair_id(pair)} {rows}x{cols} dst=")


# ---------------------------------------------------------------------------
# normalize: derived error bound against the f64 definition
# ---------------------------------------------------------------------------

NORM_EPS = 1e-6
NORM_DISTS = {"mean5_std3": (5.0, 3.0), "mean0_std1": (0.0, 1.0), "mean100_std2": (100.0, 2.0)}


@requires_gpu
@pytest.mark.parametrize("dist", list(NORM_DISTS))
@pytest.mark.parametrize("pair", [(F32, F32), (BF16, BF16), (BF16, F32)], ids=_pair_id)
def test_normalize_within_derived_bound(pair, dist):
    """|out - ref| <= 2^-22 (|z| + |mu| rstd + 1) + half an ulp of the output
    dtype at |ref|, ref = (x - mu) / sqrt(max(var, 0) + eps) in f64.

    Derivation: mu is rounded to f32 (|mu| 2^-24 rstd), x - mu and the
    product each round once in f32 (|z| 2^-24 each), rstd is within 1 ulp
    of f32 (|z| 2^-23); the sum, doubled for second-order terms, is below
    the first term; the store into the output dtype adds the second.
    mean100_std2 is the ill-conditioned case: forming var in f32 there
    cancels to ~1e-4 relative on rstd and misses the bound."""
    from lzy_amd.ops import normalize

    src_dtype, dst_dtype = pair
    mu0, sd0 = NORM_DISTS[dist]
    eps32 = float(np.float32(NORM_EPS))
    for k in GRIDS:
        n = _grid_n(8, 1, k)
        rng = np.random.default_rng(100 + k)
        # integer-valued and |x| <= 128: exact in bf16, exact stats
        x = np.clip(np.rint(rng.standard_normal(n) * sd0 + mu0), -128, 128)
        _assert_lane_partials_exact(n, STATS_VU[torch.empty(0, dtype=src_dtype).element_size()][0],
                                    k, max_abs=128)
        mu = x.mean()
        var = ((x - mu) ** 2).mean()
        rstd = 1.0 / np.sqrt(max(var, 0.0) + eps32)
        ref = (x - mu) * rstd
        mant_bits = 24 if dst_dtype == F32 else 8
        _, e = np.frexp(np.abs(ref))                 # |ref| in [2^(e-1), 2^e)
        half_ulp = np.where(ref == 0, 0.0, np.ldexp(1.0, e - 1 - mant_bits))
        bound = 2.0 ** -22 * (np.abs(ref) + abs(mu) * rstd + 1) + half_ulp

        src = torch.from_numpy(x).to(src_dtype)
        assert (src.double().numpy() == x).all()
        with _capped(k):
            if dst_dtype == src_dtype:
                out = normalize(src.cuda(), eps=NORM_EPS)
            else:
                out = torch.empty(n, dtype=dst_dtype, device="cuda")
                assert normalize(src.cuda(), dst=out, eps=NORM_EPS) is out
        assert out.dtype == dst_dtype
        err = np.abs(out.cpu().double().numpy() - ref)
        worst = int(np.argmax(err / bound))
        print(f"normalize {_pair_id(pair)} {dist} k={k}: max err/bound "
              f"{err[worst] / bound[worst]:.3f} (err {err[worst]:.3e})")
        assert (err <= bound).all(), (
            f"{dist} k={k}: err {err[worst]:.3e} > bound {bound[worst]:.3e} at "
            f"x={x[worst]}, ref={ref[worst]}")


# ---------------------------------------------------------------------------
# fill_pattern
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("k", [1, 0])
def test_fill_pattern_equals_reference(k):
    from lzy_amd.ops import fill_pattern

    T = _threads(k)
    sizes = [8 * (2 * T + 37) + r for r in (0, 2, 4, 6)] + [2, 4, 6, 8, 10]
    with _capped(k):
        for nb, seed, mask in itertools.product(sizes, [0, 42, 2 ** 63 + 5], [0, 0x3FFF]):
            # a guard element after the filled view must stay untouched
            buf = torch.full((nb // 2 + 4,), 0x5A5A, dtype=torch.int16, device="cuda")
            t = buf[: nb // 2].view(BF16)
            assert t.is_contiguous() and t.numel() * 2 == nb
            fill_pattern(t, seed=seed, mask16=mask)
            got = buf.cpu()
            assert _bits(got[: nb // 2]).numpy().tobytes() == fill_pattern_ref(nb, seed, mask), \
                (nb, seed, mask)
            assert (got[nb // 2:] == 0x5A5A).all(), (nb, seed, mask)


# ---------------------------------------------------------------------------
# wrapper contract: a destination the kernel cannot write linearly is
# rejected before anything is launched
# ---------------------------------------------------------------------------

def _bad_dsts(n, dtype):
    """(label, dst tensor, the storage to check afterwards)"""
    wide = torch.full((2 * n,), 7, dtype=dtype, device="cuda")
    short = torch.full((n - 3,), 7, dtype=dtype, device="cuda")
    host = torch.full((n,), 7, dtype=dtype)
    return [("non-contiguous", wide[::2], wide), ("short", short, short), ("cpu", host, host)]


@requires_gpu
@pytest.mark.parametrize("op_name", ["cast_copy", "normalize", "scale_shift", "axpby"])
def test_wrappers_reject_bad_dst(op_name):
    import lzy_amd.ops as ops

    n = 64
    src = torch.arange(n, dtype=F32).cuda()
    calls = {
        "cast_copy": lambda d: ops.cast_copy(src, d),
        "normalize": lambda d: ops.normalize(src, dst=d),
        "scale_shift": lambda d: ops.scale_shift(src, 2.0, 1.0, dst=d),
        "axpby": lambda d: ops.axpby(src, src, 1.0, 1.0, dst=d),
    }
    for dtype in (F32, BF16):
        for label, dst, storage in _bad_dsts(n, dtype):
            with pytest.raises(ValueError):
                calls[op_name](dst)
            torch.cuda.synchronize()
            assert (storage.cpu().float() == 7).all(), (op_name, label)


@requires_gpu
def test_transpose_cast_rejects_bad_dst():
    from lzy_amd.ops import transpose_cast

    rows, cols = 6, 10
    src = torch.arange(rows * cols, dtype=F32).view(rows, cols).cuda()
    wide = torch.full((cols, 2 * rows), 7.0, device="cuda")
    bad = [
        ("non-contiguous", wide[:, ::2], wide),
        ("wrong shape", torch.full((rows, cols), 7.0, device="cuda"), None),
        ("wrong numel", torch.full((cols, rows - 1), 7.0, device="cuda"), None),
        ("cpu", torch.full((cols, rows), 7.0), None),
    ]
    for label, dst, storage in bad:
        with pytest.raises(ValueError):
            transpose_cast(src, dst=dst)
        torch.cuda.synchronize()
        assert ((storage if storage is not None else dst).cpu() == 7).all(), label


@requires_gpu
def test_fill_pattern_rejects_non_contiguous():
    from lzy_amd.ops import fill_pattern

    wide = torch.full((128,), 7.0, device="cuda")
    with pytest.raises(ValueError):
        fill_pattern(wide[::2], seed=1)
    with pytest.raises(ValueError):
        fill_pattern(torch.zeros(16), seed=1)
    torch.cuda.synchronize()
    assert (wide.cpu() == 7).all()
