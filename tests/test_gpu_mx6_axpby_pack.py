"""lz_mx6_axpby_pack / lz_mx6_axpby2_pack on MI355X against the float64 reference of
tests/test_mxfp6.py and the two kernels they fuse.  REQUIRES the native extension."""
import itertools

import numpy as np
import pytest
import torch

import lzy_amd.ops as ops
import test_mxfp6 as ref
from test_mxfp6 import ALPHA, BETA, DTYPES, F32, IDS
from test_gpu_mxwire_exact import _capped, _guarded, _guards_untouched, _offset_view

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

PAIRS = list(itertools.product(DTYPES, repeat=2))
PAIR_IDS = [f"{a}-{d}" for a, d in itertools.product(IDS, repeat=2)]
# (n, grid cap, element-aligned view).  A lane owns one half (16 elements) per
# trip, a wave 1024 elements, a workgroup 4096.  1: one element; 15: a first half
# cut by n; 16: one half, the partner lane all padding; 17, 31: a second half
# cut; 32: whole blocks; 33: the padded second half of the last block; 3077: one
# workgroup, waves 0..2 unguarded and wave 3 cut; 4101 cap 1: a guarded second
# grid-stride trip; 4101 view: the element-aligned instantiation, two workgroups;
# 65536 + 37 cap 2: several trips of two workgroups, the last one guarded
SHAPES = [(n, 0, False) for n in (1, 15, 16, 17, 31, 32, 33, 3077)] + \
    [(4101, 1, False), (4101, 0, True), (65536 + 37, 2, False)]


def _wire_ref(dst_cpu):
    return torch.from_numpy(ref.mx6_pack_ref(dst_cpu.to(F32).numpy()))


@pytest.mark.parametrize("a_dtype,dst_dtype", PAIRS, ids=PAIR_IDS)
def test_against_float64_reference(a_dtype, dst_dtype):
    """All 64 codes at each of four positions under 13 scale bytes."""
    wire, n = ref.decode_inputs()
    a = ref.axpby_operand(wire, n).to(a_dtype)
    want = ref.axpby_ref(a, wire, dst_dtype)
    with _capped(2):
        dst, wout = ops.mx6_axpby_pack(a.cuda(), torch.from_numpy(wire).cuda(), ALPHA, BETA,
                                       dst=torch.empty(n, dtype=dst_dtype, device="cuda"))
    ref.assert_same(dst.cpu(), want, "dst")
    assert torch.equal(wout.cpu(), _wire_ref(want))


@pytest.mark.parametrize("a_dtype,dst_dtype,plain", [(*p, False) for p in PAIRS]
                         + [(torch.bfloat16,) * 2 + (True,), (F32, torch.float16, True)],
                         ids=PAIR_IDS + ["plain-bf16-bf16", "plain-f32-f16"])
def test_shapes_equal_combine_then_pack(a_dtype, dst_dtype, plain):
    """== the combine kernel, then mx6_pack, same alignment; a planted NaN: block 3."""
    g = torch.Generator().manual_seed(5)
    for n, cap, view in SHAPES:
        what = f"n={n} cap={cap} view={view}"
        a = (torch.randn(n, generator=g) * 3).to(a_dtype)
        b = torch.randn(n, generator=g).to(a_dtype)
        if n >= 3077:
            a[100] = float("nan")
        dev = _offset_view if view else torch.Tensor.cuda
        with _capped(cap):
            second = b if plain else ops.mx6_pack(b.cuda()).cpu()
            want = dev(torch.zeros(n, dtype=dst_dtype))
            (ops.axpby if plain else ops.mx6_axpby)(dev(a), dev(second), 0.75, -1.25, dst=want)
            want_wire = ops.mx6_pack(want)
            dst = dev(torch.zeros(n, dtype=dst_dtype))
            wout = dev(torch.zeros(want_wire.numel(), dtype=torch.uint8))
            got = (ops.mx6_axpby2_pack if plain else ops.mx6_axpby_pack)(
                dev(a), dev(second), 0.75, -1.25, dst=dst, wire_out=wout)
        assert got[0] is dst and got[1] is wout
        ref.assert_same(dst.cpu(), want.cpu(), what)
        assert torch.equal(wout.cpu(), want_wire.cpu()), what
        if n >= 3077:
            assert int(wout[24 * -(-n // 32) + 3]) == 0xFF, what


@pytest.mark.parametrize("last_scale", [127, 0xFF], ids=["finite", "nanblock"])
@pytest.mark.parametrize("beta", [1.0, float("inf")], ids=["one", "inf"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padding_and_bounds(dtype, beta, last_scale):
    """n = 33, the 31 padding codes of wire_in 0x3f: positions >= n enter the
    encoder as +0.0.  beta = inf turns x^ != 0 into +-Inf and x^ == 0 into NaN."""
    n, alpha = 33, 0.5
    q = np.full(64, 0x3F, np.uint8)
    q[:n] = (np.arange(n) * 5 + 1) % 64
    q[5] = 0
    wire = np.r_[ref.codes_to_bytes(q.reshape(2, 32)), 127, last_scale].astype(np.uint8)
    a = torch.arange(-16, 17, dtype=F32).to(dtype)
    with np.errstate(all="ignore"):
        xh = ref.mx6_unpack_ref(wire, n).astype(np.float32)
        p = (xh * np.float32(beta)).astype(np.float64)
        r = (a.double().numpy() * alpha + p).astype(np.float32)
    want = ref.to_dtype(r.astype(np.float64), dtype)
    assert bool(torch.isnan(want[32])) == (last_scale == 0xFF)
    want_wire = _wire_ref(want)
    w_in = torch.from_numpy(wire).cuda()
    big_w, wout = _guarded(50)
    buf = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    ops.mx6_axpby_pack(a.cuda(), w_in, alpha, beta, dst=buf[:n], wire_out=wout)
    ref.assert_same(buf[:n].cpu(), want, "dst")
    got = wout.cpu()
    assert torch.equal(got, want_wire)
    # element 32 is the low six bits of byte 24; the second half is bytes 36..47
    assert int(got[24]) >> 6 == 0 and not got[25:48].any()
    assert _guards_untouched(big_w, 50) and bool((buf[n:] == 7.0).all())
    acc = a.cuda()
    inplace = ops.mx6_axpby_pack(acc, w_in, alpha, beta, dst=acc)
    ref.assert_same(acc.cpu(), want, "in place")
    assert torch.equal(inplace[1].cpu(), want_wire)


def test_wrapper_and_dispatch(monkeypatch):
    from lzy_amd.channels import mxwire
    from lzy_amd.exceptions import NativeExtensionMissing

    a, b = torch.randn(64, device="cuda"), torch.randn(64, device="cuda")
    wire = ops.mx6_pack(b)
    for bad in (torch.empty(51, dtype=torch.uint8, device="cuda"),
                torch.empty(50, dtype=torch.int8, device="cuda"), wire):
        with pytest.raises(ValueError):
            ops.mx6_axpby_pack(a, wire, wire_out=bad)
    with pytest.raises(ValueError):
        ops.mx6_axpby_pack(a.cpu(), wire)
    want, want2 = ops.mx6_axpby(a, wire, 0.5, -1.5), ops.axpby(a, b, 0.5, -1.5)
    want_wires = ops.mx6_pack(want), ops.mx6_pack(want2)

    def no_pack(*args, **kw):
        raise AssertionError("the forwarding step took mx6_pack")

    with monkeypatch.context() as m:
        m.setattr(ops, "mx6_pack", no_pack)
        axpby_pack, axpby2_pack = mxwire.wire_fused("mxfp6")
        got, got2 = axpby_pack(a, wire, 0.5, -1.5), axpby2_pack(a, b, 0.5, -1.5)
    assert torch.equal(got[0], want) and torch.equal(got[1], want_wires[0])
    assert torch.equal(got2[0], want2) and torch.equal(got2[1], want_wires[1])
    monkeypatch.setattr(ops, "_MX6_AXPBY_PACK", False)
    for name, second in (("mx6_axpby_pack", wire), ("mx6_axpby2_pack", b)):
        with pytest.raises(NativeExtensionMissing):
            getattr(ops, name)(a, second)
    assert ops.mx6_axpby(a, wire).shape == (64,)
