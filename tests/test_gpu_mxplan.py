"""The fused MXFP8 decode-combine kernel (lz_mx8_axpby) on MI355X (gfx950)
and a wired streamed plan on one GPU.

The oracle is the torch codec (lzy_amd.channels.mxwire) on the CPU copy of
the data, or exact integer arithmetic — never a kernel.  These tests
REQUIRE the native extension: a missing libhipops.so fails loudly."""
import functools
import itertools
import os
import socket
import subprocess
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROOT = Path(__file__).resolve().parent.parent

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, BF16, F16]
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
PAIRS9 = list(itertools.product(DTYPES, DTYPES))

ALPHA, BETA = 0.75, -1.5


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


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_same_bits(got, want, what):
    """Bytes equal; NaN compared by position, not payload."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn), (
        f"{what}: NaN positions differ at {(gn != wn).nonzero()[:8].flatten().tolist()}")
    bad = (_bits(got) != _bits(want)) & ~wn
    if bad.any():
        idx = bad.nonzero().flatten()[:8]
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at "
            f"{idx.tolist()}: got {got[idx].tolist()} want {want[idx].tolist()}")


# e4m3fn code -> value * 2^9 as an exact integer (the smallest subnormal is
# 2^-9); the two NaN codes map to 0 and are masked by position
_E4M3 = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(
    torch.float8_e4m3fn).to(torch.float64).numpy()
_E4M3_NAN = np.isnan(_E4M3)
_E4M3_I = np.where(_E4M3_NAN, 0.0, _E4M3 * 512).astype(np.int64)
assert _E4M3_NAN.nonzero()[0].tolist() == [0x7F, 0xFF]
assert (_E4M3_I.astype(np.float64) / 512 == np.where(_E4M3_NAN, 0.0, _E4M3)).all()


def _hand_wire(n, scales):
    """A wire buffer built by hand: element i carries payload code
    (37*i + 11) % 256 — every 256 consecutive elements hold all 256 codes —
    and block k the scale byte scales[k % len(scales)].  Returns (uint8
    wire, codes, per-element scale byte)."""
    nblk = (n + 31) // 32
    codes = (np.arange(32 * nblk) * 37 + 11) % 256
    codes[n:] = 0  # the padded tail encodes 0.0
    sb = np.asarray(scales)[np.arange(nblk) % len(scales)]
    wire = torch.from_numpy(np.concatenate([codes, sb]).astype(np.uint8))
    return wire, codes[:n], np.repeat(sb, 32)[:n]


@functools.lru_cache(maxsize=None)
def _few_bit_values(n, seed):
    """+-m * 2^e with an 8-bit m (exact in bf16, f16 and f32) and |value| in
    [2^-8, 2^9).  Returns (float64 values, the same times 2^15 as int64)."""
    rng = np.random.default_rng(seed)
    m = rng.integers(128, 256, size=n)
    e = rng.integers(-15, 2, size=n)          # value in [2^(7+e), 2^(8+e))
    sign = rng.choice([-1, 1], size=n)
    scaled = sign * m * (1 << (e + 15))       # value * 2^15, integer
    return scaled.astype(np.float64) / 2.0 ** 15, scaled.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _exact_case(n):
    """Inputs whose float64 evaluation is provably the exact value, and
    that value.  Everything is an integer multiple of 2^-17:
    a*alpha*2^17 = (a*2^15) * 3; x^ = q*2^-9 * 2^(b-127) with b in
    120..134, so x^*beta*2^17 = (q*2^9) * 2^(b-120) * -3."""
    a, ai = _few_bit_values(n, seed=31)
    wire, codes, sb = _hand_wire(n, list(range(120, 135)))
    qi = _E4M3_I[codes]
    xhat = qi.astype(np.float64) / 512 * 2.0 ** (sb.astype(np.float64) - 127)
    p = xhat * BETA
    # x^ has <= 4 significant bits, x^*beta <= 6: exact in fp32
    assert (xhat.astype(np.float32).astype(np.float64) == xhat).all()
    assert (p.astype(np.float32).astype(np.float64) == p).all()
    expr = a * ALPHA + p
    total = ai * 3 + qi * (1 << (sb.astype(np.int64) - 120)) * -3
    assert (np.abs(ai * 3) + np.abs(total - ai * 3) < 2 ** 53).all()
    assert (total.astype(np.float64) / 2.0 ** 17 == expr).all()
    nan = _E4M3_NAN[codes]
    expr = np.where(nan, np.nan, expr)
    return a, wire, expr


# ---------------------------------------------------------------------------
# bit-exact combine
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("pair", PAIRS9, ids=_pair_id)
def test_mx8_axpby_bit_exact(pair):
    """dst == round_dst(round_f32(exact)) for every payload code, scale
    bytes 120..134, all 9 dtype pairs; a capped grid at the largest size
    so every lane takes several trips, the last one partial."""
    from lzy_amd.ops import mx8_axpby

    a_dtype, dst_dtype = pair
    for n, cap in [(1, 0), (7, 0), (8, 0), (9, 0), (31, 0), (32, 0), (33, 0),
                   (257, 0), (3 * 4096 + 45, 2)]:
        a_np, wire, expr = _exact_case(n)
        a = torch.from_numpy(a_np).to(a_dtype)
        assert (a.double().numpy() == a_np).all()
        want = torch.from_numpy(expr).to(F32).to(dst_dtype)
        what = f"{_pair_id(pair)} n={n} cap={cap}"
        with _capped(cap):
            d = a.cuda()
            dst = torch.empty(n, dtype=dst_dtype, device="cuda")
            assert mx8_axpby(d, wire.cuda(), ALPHA, BETA, dst=dst) is dst
            _assert_same_bits(dst.cpu(), want, what)
            if a_dtype == dst_dtype:
                out = mx8_axpby(d, wire.cuda(), ALPHA, BETA)
                _assert_same_bits(out.cpu(), want, what + " new dst")
                _assert_same_bits(d.cpu(), a, what + " a untouched")
                assert mx8_axpby(d, wire.cuda(), ALPHA, BETA, dst=d) is d
                _assert_same_bits(d.cpu(), want, what + " in place")


# ---------------------------------------------------------------------------
# scale extremes
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dst_dtype", [F32, BF16], ids=["f32", "bf16"])
def test_mx8_axpby_scale_extremes(dst_dtype):
    """a = 0, alpha = 0, beta = 1 leaves the decoded value alone: b == 0
    blocks decode through the subnormal multiplier 2^-127 (nothing is
    flushed to zero), b == 247 is the largest scale the packer emits."""
    from lzy_amd.channels.mxwire import mx8_unpack_torch
    from lzy_amd.ops import mx8_axpby

    n = 16 * 32 + 5
    wire, codes, sb = _hand_wire(n, [0, 247, 1, 0])
    x = mx8_unpack_torch(wire, n, F32)
    tiny = x[torch.from_numpy(sb == 0)]
    tiny = tiny[~torch.isnan(tiny)]
    assert tiny.ne(0).any() and tiny.abs().max() < 2.0 ** -118  # 448 * 2^-127
    assert x[~torch.isnan(x)].abs().max() == 448 * 2.0 ** 120
    want = x.to(dst_dtype)
    for a_dtype in DTYPES:
        a = torch.zeros(n, dtype=a_dtype, device="cuda")
        got = mx8_axpby(a, wire.cuda(), 0.0, 1.0,
                        dst=torch.empty(n, dtype=dst_dtype, device="cuda")).cpu()
        gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
        assert torch.equal(gn, wn)
        assert wn.sum().item() == np.isin(codes, [0x7F, 0xFF]).sum()
        # by value: fma(0, 0, -0.0) is +0.0, the bare decode keeps -0.0
        assert torch.equal(got[~wn].double(), want[~wn].double()), NAMES[a_dtype]


# ---------------------------------------------------------------------------
# random data
# ---------------------------------------------------------------------------

def _ordered(t):
    """Floats as integers in value order (sign-magnitude -> two's
    complement), so adjacent representable values differ by 1."""
    b = _bits(t).to(torch.int64)
    mask = (1 << (8 * t.element_size() - 1)) - 1
    mag = b & mask
    return torch.where(b < 0, -mag, mag)


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS9, ids=_pair_id)
def test_mx8_axpby_random_within_one_ulp(pair):
    """The kernel's FMA rounds the exact sum to fp32 once; the reference
    rounds it to float64 first.  The two fp32 values are equal or adjacent,
    and rounding is monotonic, so the results in the destination dtype are
    equal or adjacent too: at most one unit in the last place."""
    from lzy_amd.channels.mxwire import mx8_axpby_torch, mx8_pack_torch
    from lzy_amd.ops import mx8_axpby

    a_dtype, dst_dtype = pair
    n = 3 * 4096 + 45
    g = torch.Generator().manual_seed(77)
    for mag in (1e-4, 1.0, 3e3):
        a = (torch.randn(n, generator=g) * mag).to(a_dtype)
        wire = mx8_pack_torch(torch.randn(n, generator=g) * mag)
        for alpha, beta in ((0.3, -1.7), (0.5, 0.5)):
            want = mx8_axpby_torch(a, wire, alpha, beta, out_dtype=dst_dtype)
            assert torch.isfinite(want.float()).all()
            got = mx8_axpby(
                a.cuda(), wire.cuda(), alpha, beta,
                dst=torch.empty(n, dtype=dst_dtype, device="cuda")).cpu()
            ulps = (_ordered(got) - _ordered(want)).abs()
            print(f"mx8_axpby {_pair_id(pair)} mag={mag} ({alpha}, {beta}): "
                  f"max {ulps.max().item()} ulp, "
                  f"{ulps.ne(0).float().mean().item():.2e} of elements differ")
            assert ulps.max().item() <= 1


# ---------------------------------------------------------------------------
# no stray writes, views, in place
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=[NAMES[d] for d in DTYPES])
def test_mx8_axpby_never_writes_past_dst(dtype):
    from lzy_amd.channels.mxwire import mx8_axpby_torch, mx8_pack_torch
    from lzy_amd.ops import mx8_axpby

    guard, sentinel = 64, -7.0
    g = torch.Generator().manual_seed(5)
    for n in [1, 31, 33, 257, 2053]:
        a = torch.randint(-8, 9, (n,), generator=g).to(dtype)
        wire = mx8_pack_torch(torch.randint(-8, 9, (n,), generator=g).float())
        want = mx8_axpby_torch(a, wire, 1.0, 1.0)  # small integers: exact
        for lead in (guard, guard + 1):  # aligned and element-aligned dst
            full = torch.full((lead + n + guard,), sentinel, dtype=dtype,
                              device="cuda")
            dst = full[lead: lead + n]
            assert mx8_axpby(a.cuda(), wire.cuda(), 1.0, 1.0, dst=dst) is dst
            hostv = full.cpu()
            assert hostv[:lead].eq(sentinel).all(), (n, lead)
            assert hostv[lead + n:].eq(sentinel).all(), (n, lead)
            assert torch.equal(hostv[lead: lead + n], want), (n, lead)


@requires_gpu
def test_mx8_axpby_views_and_in_place():
    """An element-aligned a, a byte-shifted wire and an element-aligned dst
    take the guarded path and give the bytes of the aligned run."""
    from lzy_amd.ops import mx8_axpby, mx8_pack

    g = torch.Generator().manual_seed(9)
    for dtype in DTYPES:
        n = 4096 + 77
        base = (torch.randn(n + 1, generator=g) * 3).to(dtype).cuda()
        a_view = base[1:]
        assert a_view.data_ptr() % 16 != 0
        a = a_view.clone()
        assert a.data_ptr() % 16 == 0
        wire = mx8_pack((torch.randn(n, generator=g) * 3).cuda())
        shifted = torch.empty(wire.numel() + 1, dtype=torch.uint8, device="cuda")
        shifted[1:] = wire
        want = mx8_axpby(a, wire, ALPHA, BETA)
        assert torch.equal(mx8_axpby(a_view, wire, ALPHA, BETA), want)
        assert torch.equal(mx8_axpby(a, shifted[1:], ALPHA, BETA), want)
        full = torch.zeros(n + 1, dtype=dtype, device="cuda")
        mx8_axpby(a, wire, ALPHA, BETA, dst=full[1:])
        assert torch.equal(full[1:], want) and full[0].item() == 0
        # in place, aligned and element-aligned
        acc = a.clone()
        assert mx8_axpby(acc, wire, ALPHA, BETA, dst=acc) is acc
        assert torch.equal(acc, want)
        assert mx8_axpby(a_view, wire, ALPHA, BETA, dst=a_view) is a_view
        assert torch.equal(a_view, want)


# ---------------------------------------------------------------------------
# wrapper
# ---------------------------------------------------------------------------

@requires_gpu
def test_mx8_axpby_wrapper_errors():
    """Rejected before any launch: dst keeps its bytes."""
    from lzy_amd.ops import mx8_axpby, mx8_nbytes, mx8_pack

    n = 100
    a = torch.randn(n, device="cuda")
    wire = mx8_pack(torch.randn(n, device="cuda"))
    assert wire.numel() == mx8_nbytes(n)
    dst = torch.full((n,), -7.0, device="cuda")
    wide = torch.full((2 * n,), -7.0, device="cuda")
    bad_calls = [
        lambda: mx8_axpby(a, wire[:-1], dst=dst),                  # short wire
        lambda: mx8_axpby(a, torch.cat([wire, wire[:33]]), dst=dst),
        lambda: mx8_axpby(a, wire.to(torch.int8), dst=dst),        # not uint8
        lambda: mx8_axpby(a, torch.cat([wire, wire])[::2], dst=dst),  # strided
        lambda: mx8_axpby(a.to(torch.int32), wire, dst=dst),       # int a
        lambda: mx8_axpby(a, wire, dst=wide[::2]),                 # strided dst
        lambda: mx8_axpby(a, wire, dst=wide),                      # wrong size
        lambda: mx8_axpby(a, wire, dst=wide[: n - 1]),
        lambda: mx8_axpby(a, wire, dst=torch.zeros(n, dtype=torch.int32,
                                                   device="cuda")),
        lambda: mx8_axpby(a.cpu(), wire, dst=dst),                 # host tensors
        lambda: mx8_axpby(a, wire.cpu(), dst=dst),
        lambda: mx8_axpby(a, wire, dst=dst.cpu()),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert dst.eq(-7.0).all() and wide.eq(-7.0).all(), i
    # n == 0 is a no-op
    e = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    out = mx8_axpby(e, torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert out.numel() == 0 and out.dtype == torch.bfloat16


@requires_gpu
def test_lz_mx8_axpby_argument_checks():
    """The C entry point itself: a negative n or a dtype outside
    f32/f16/bf16 is hipErrorInvalidValue (1), n == 0 is success, all
    without a launch (the pointers are null)."""
    import ctypes

    import lzy_amd.ops as ops

    lib = ops._require_native()
    z, one = ctypes.c_void_p(0), ctypes.c_float(1.0)
    assert lib.lz_mx8_axpby(z, 0, z, z, 0, -1, one, one, z) == 1
    for bad in (3, 5, 7, 8, 99):  # e4m3, u8, i64, f64, unknown
        assert lib.lz_mx8_axpby(z, bad, z, z, 0, 8, one, one, z) == 1
        assert lib.lz_mx8_axpby(z, 0, z, z, bad, 8, one, one, z) == 1
    for code in (0, 1, 2):
        assert lib.lz_mx8_axpby(z, code, z, z, 2 - code, 0, one, one, z) == 0


@requires_gpu
def test_mx8_axpby_stale_library_raises(monkeypatch):
    """A libhipops.so without the export: this op raises, the others work,
    and the dispatcher takes no torch detour."""
    import lzy_amd.ops as ops
    from lzy_amd.channels import mxwire
    from lzy_amd.exceptions import NativeExtensionMissing

    a = torch.randn(64, device="cuda")
    wire = ops.mx8_pack(a)
    monkeypatch.setattr(ops, "_MX8_AXPBY", False)
    with pytest.raises(NativeExtensionMissing):
        ops.mx8_axpby(a, wire)
    with pytest.raises(NativeExtensionMissing):
        mxwire.mx8_axpby(a, wire, 0.5, 0.5)
    assert ops.mx8_unpack(wire, 64, torch.float32).shape == (64,)
    assert ops.axpby(a, a).shape == (64,)


@requires_gpu
def test_mx8_axpby_dispatcher_takes_the_kernel():
    from lzy_amd.channels import mxwire

    g = torch.Generator().manual_seed(1)
    a = torch.randn(1000, generator=g)
    wire = mxwire.mx8_pack_torch(torch.randn(1000, generator=g))
    want = mxwire.mx8_axpby_torch(a, wire, 0.5, 0.5)
    dst = torch.empty(1000, device="cuda")
    assert mxwire.mx8_axpby(a.cuda(), wire.cuda(), 0.5, 0.5, dst=dst) is dst
    assert (_ordered(dst.cpu()) - _ordered(want)).abs().max().item() <= 1


# ---------------------------------------------------------------------------
# a wired plan on one GPU
# ---------------------------------------------------------------------------

@requires_gpu
def test_wired_plan_four_ranks_one_gpu(tmp_path):
    """Device leaves, 4 ranks sharing one GPU (the host-staged path): kernel
    pack before staging, kernel decode-combine on arrival.  The script
    holds every node output to the per-hop bound of docs/mxwire.md
    propagated through the plan, demands a nonzero error, the mx8_nbytes
    wire-byte total and at least one stream plan."""
    env = dict(os.environ)
    env["MXPLAN_DEVICE"] = "cuda"
    env["HIP_VISIBLE_DEVICES"] = "0"  # all ranks share one GPU
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env.pop("LZY_STREAM_WIRE_CAST", None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    res = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node=4",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            "tests/pool_script_mxplan.py",
        ],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300,
    )
    print("STDOUT:", res.stdout[-4000:])
    if res.returncode != 0:
        print("STDERR:", res.stderr[-4000:])
    assert res.returncode == 0
    assert "MXPLAN-WIRED-OK" in res.stdout
    assert "MXPLAN-OK" in res.stdout
