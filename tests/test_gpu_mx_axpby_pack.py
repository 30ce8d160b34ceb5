"""lz_mx8_axpby_pack, lz_mx8_axpby2_pack and their mxi8 twins on MI355X: dst
and wire_out against the float64 references, and against the sibling kernels
they fuse on every path of the loop.  REQUIRES the native extension."""
import itertools

import numpy as np
import pytest
import torch

import kernel_refs as kr
import test_gpu_mxplan as tp
import test_mxint8 as ti
from test_gpu_mxwire_exact import _capped, _guarded, _guards_untouched, _offset_view

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
PAIRS = list(itertools.product([F32, BF16, F16], repeat=2))
PAIR_IDS = [f"{NAMES[a]}-{NAMES[d]}" for a, d in PAIRS]
CODECS = ["mx8", "mxi8"]
# (n, grid cap, element-aligned views) -> the path of the loop it reaches.
# The default grid has stride >= ngroups, so a second group needs a cap.
SHAPES = [
    (1, 0, False), (31, 0, False),   # one wave, a padded last block
    (32, 0, False), (33, 0, False),  # a whole block; a partial scale dword
    (4101, 0, False),                # all guarded, three blocks of threads
    (2500, 1, False),                # guarded, second group present and cut by n
    (4101, 1, False),                # the two-group unguarded path + a guarded tail
    (4101, 0, True),                 # ALIGNED=false
    (65536 + 37, 2, False),          # several grid-stride trips
]


def _ops(codec):
    import lzy_amd.ops as ops
    assert ops.NATIVE, "HIP ops must be built+loadable on a GPU box"
    return ops, {k: getattr(ops, f"{codec}_{k}")
                 for k in ("pack", "axpby", "axpby_pack", "axpby2_pack")}


def _pack_ref(codec, dst_cpu):
    if codec == "mx8":
        return kr.mx8_wire_ref(dst_cpu)
    return torch.from_numpy(ti.mxi8_pack_ref(dst_cpu.to(F32).numpy()))


def _decode64(codec, wire, n):
    if codec == "mxi8":
        return ti.mxi8_unpack_ref(wire, n)
    nblk = (n + 31) // 32
    bits, nan = kr.mx8_unpack_ref(wire[: 32 * nblk], wire[32 * nblk:], n, F32)
    return np.where(nan, np.nan, kr.from_bits(bits, F32).double().numpy())


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("codec", CODECS)
def test_against_float64_references(codec, pair):
    """Every payload code under the scale bytes of the existing exact tests,
    few-bit a/alpha/beta: dst is the reference combine bit for bit, wire_out
    the reference pack of that dst byte for byte."""
    a_dtype, dst_dtype = pair
    if codec == "mx8":
        alpha, beta = tp.ALPHA, tp.BETA
        a_np, wire, expr = tp._exact_case(3 * 4096 + 45)
        a = torch.from_numpy(a_np).to(a_dtype)
        want = torch.from_numpy(expr).to(F32).to(dst_dtype)
    else:
        alpha, beta = ti.ALPHA, ti.BETA
        wire, n = ti.decode_inputs()
        a = ti.axpby_operand(wire, n).to(a_dtype)
        want = ti.axpby_ref(a, wire, dst_dtype)
        wire = torch.from_numpy(wire)
    _, f = _ops(codec)
    with _capped(2):
        dst, wout = f["axpby_pack"](a.cuda(), wire.cuda(), alpha, beta,
                                    dst=torch.empty(a.numel(), dtype=dst_dtype, device="cuda"))
    ti.assert_same(dst.cpu(), want, "dst")
    assert torch.equal(wout.cpu(), _pack_ref(codec, want))


def _run_shapes(codec, pair, plain):
    """dst and wire_out of the fused op == the combine kernel, then the pack
    kernel (both pinned to the spec elsewhere): what the plan relies on."""
    ops, f = _ops(codec)
    a_dtype, dst_dtype = pair
    g = torch.Generator().manual_seed(5)
    for n, cap, view in SHAPES:
        what = f"n={n} cap={cap} view={view}"
        a = (torch.randn(n, generator=g) * 3).to(a_dtype)
        b = torch.randn(n, generator=g).to(a_dtype)
        dev = _offset_view if view else torch.Tensor.cuda
        with _capped(cap):
            second = b.cuda() if plain else f["pack"](b.cuda())
            # the siblings on operands of the same alignment (every path
            # rounds an f16 the same way: test_gpu_combine_rounding.py)
            want = dev(torch.zeros(n, dtype=dst_dtype))
            (ops.axpby if plain else f["axpby"])(dev(a), dev(second.cpu()), 0.75, -1.25,
                                                 dst=want)
            want_wire = f["pack"](want)
            dst = dev(torch.zeros(n, dtype=dst_dtype))
            wout = dev(torch.zeros(want_wire.numel(), dtype=torch.uint8))
            got = f["axpby2_pack" if plain else "axpby_pack"](
                dev(a), dev(second.cpu()), 0.75, -1.25, dst=dst, wire_out=wout)
        assert got[0] is dst and got[1] is wout
        ti.assert_same(dst.cpu(), want.cpu(), what)
        assert torch.equal(wout.cpu(), want_wire.cpu()), what


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("codec", CODECS)
def test_shapes_equal_axpby_then_pack(codec, pair):
    _run_shapes(codec, pair, plain=False)


@requires_gpu
@pytest.mark.parametrize("codec", CODECS)
def test_plain_operand_equals_axpby_then_pack(codec):
    _run_shapes(codec, (BF16, BF16), plain=True)
    _run_shapes(codec, (F32, F16), plain=True)


@requires_gpu
@pytest.mark.parametrize("beta", [float("inf"), 1.0], ids=["inf", "one"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=list(NAMES.values()))
@pytest.mark.parametrize("codec", CODECS)
def test_padding_and_bounds(codec, dtype, beta):
    """n = 33 with the 31 padding payload bytes of wire_in set to 0x7e (448,
    or 126, times the block scale): positions >= n enter the encoder as
    +0.0.  With beta = inf every x^ != 0 gives +-Inf and x^ == 0 gives NaN."""
    n, alpha = 33, 0.5
    codes = (np.arange(64) * 7 + 9) % 120 + 1      # finite, nonzero in both codecs
    codes[1::2] |= 0x80
    codes[5], codes[n:] = 0, 0x7E
    wire = np.concatenate([codes, [127, 127] if codec == "mx8" else [133, 133]]).astype(np.uint8)
    a = torch.arange(-16, 17, dtype=F32).to(dtype)
    with np.errstate(all="ignore"):
        p = (_decode64(codec, wire, n).astype(np.float32) * np.float32(beta)).astype(np.float64)
        want = ti.to_dtype((a.double().numpy() * alpha + p).astype(np.float32).astype(np.float64), dtype)
    want_wire = _pack_ref(codec, want)
    assert want_wire[n:64].eq(0).all() and want_wire[65] == _pack_ref(codec, want[32:])[32]
    _, f = _ops(codec)
    big_w, wout = _guarded(66)
    buf = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    f["axpby_pack"](a.cuda(), torch.from_numpy(wire).cuda(), alpha, beta, dst=buf[:n], wire_out=wout)
    ti.assert_same(buf[:n].cpu(), want, "dst")
    assert torch.equal(wout.cpu(), want_wire)
    assert _guards_untouched(big_w, 66) and bool((buf[n:] == 7.0).all())
    acc = a.cuda()
    got = f["axpby_pack"](acc, torch.from_numpy(wire).cuda(), alpha, beta, dst=acc)
    ti.assert_same(acc.cpu(), want, "in place")
    assert torch.equal(got[1].cpu(), want_wire)


@requires_gpu
def test_wrapper_errors(monkeypatch):
    from lzy_amd.exceptions import NativeExtensionMissing

    ops, f = _ops("mx8")
    a = torch.randn(64, device="cuda")
    wire = ops.mx8_pack(a)
    for bad in (torch.empty(65, dtype=torch.uint8, device="cuda"),
                torch.empty(66, dtype=torch.int8, device="cuda"), wire):
        with pytest.raises(ValueError):
            ops.mx8_axpby_pack(a, wire, wire_out=bad)
    with pytest.raises(ValueError):
        ops.mx8_axpby_pack(a.cpu(), wire)
    monkeypatch.setattr(ops, "_MX_AXPBY_PACK", False)
    for name in ("mx8_axpby_pack", "mxi8_axpby_pack", "mx8_axpby2_pack", "mxi8_axpby2_pack"):
        with pytest.raises(NativeExtensionMissing):
            getattr(ops, name)(a, a if "2" in name else wire)
    assert ops.mx8_axpby(a, wire).shape == (64,)
