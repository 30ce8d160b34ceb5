"""The MXFP6 kernels (lz_mx6_pack / _unpack / _axpby) against the float64
reference of tests/test_mxfp6.py, bit for bit, the forwarding-node step and
the pair primitive with device tensors (docs/mxwire.md, "MXFP6").
"""
import numpy as np
import pytest
import torch

import test_mxfp6 as ref
from test_mxfp6 import ALPHA, BETA, DTYPES, F32, IDS
from test_gpu_mxwire_exact import _capped, _offset_view
from test_mxplan import _torchrun

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
GUARD = 64

# (numel, grid cap, offset view); one wave is 1024 elements
PACK_CASES = [(n, 0, False) for n in (1, 15, 16, 17, 31, 32, 33, 1024 + 5, 4096 + 5)] + \
    [(4096 + 5, 0, True), ((1 << 18) + 37, 2, False)]


@requires_gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"n{c[0]}cap{c[1]}view{int(c[2])}")
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_equals_reference(dtype, case):
    import lzy_amd.ops as ops

    n, cap, view = case
    base = ref.encode_inputs()
    # short cases start in the NaN block, those past half a block run into the Inf block
    start = 32 * 21 + 16 * (n > 16) if n < 64 else 0
    x = base.repeat(-(-(start + n) // base.numel()))[start: start + n].to(dtype)
    want = ref.mx6_pack_ref(x.to(F32).numpy())
    big = torch.full((want.size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    with _capped(cap):
        ops.mx6_pack(_offset_view(x) if view else x.cuda(), out=big[GUARD: GUARD + want.size])
    got = big.cpu().numpy()
    assert want.size == ops.mx6_nbytes(n) == 25 * -(-n // 32)
    assert np.array_equal(got[GUARD: -GUARD], want), np.nonzero(got[GUARD: -GUARD] != want)[0][:8]
    assert (got[:GUARD] == 0xCD).all() and (got[-GUARD:] == 0xCD).all()


def _decode_case(n):
    """The first n elements of the decode inputs: the scale bytes move up."""
    full, total = ref.decode_inputs()
    nblk = -(-n // 32)
    return np.concatenate([full[: 24 * nblk], full[24 * total // 32:][:nblk]])


@requires_gpu
@pytest.mark.parametrize("n", [3328, 3328 - 13, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_equals_reference(dtype, n):
    import lzy_amd.ops as ops

    wire = _decode_case(n)
    want = ref.to_dtype(ref.mx6_unpack_ref(wire, n), dtype)
    for view in (False, True):
        buf = torch.full((n + GUARD + 1,), 7.0, dtype=dtype, device="cuda")
        out = buf[1: 1 + n] if view else buf[:n]
        ops.mx6_unpack(torch.from_numpy(wire).cuda(), n, dtype, out=out)
        ref.assert_same(out.cpu(), want, f"view={view}")
        rest = buf[1 + n:] if view else buf[n:]
        assert bool((rest == 7.0).all()) and (not view or float(buf[0]) == 7.0)


@requires_gpu
@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("a_dtype", DTYPES, ids=IDS)
def test_axpby_equals_reference(a_dtype, dst_dtype):
    import lzy_amd.ops as ops

    wire, n = ref.decode_inputs()
    a = ref.axpby_operand(wire, n).to(a_dtype)
    want = ref.axpby_ref(a, wire, dst_dtype)
    w = torch.from_numpy(wire).cuda()
    buf = torch.full((n + GUARD,), 7.0, dtype=dst_dtype, device="cuda")
    ops.mx6_axpby(a.cuda(), w, ALPHA, BETA, dst=buf[:n])
    ref.assert_same(buf[:n].cpu(), want)
    assert bool((buf[n:] == 7.0).all())
    ref.assert_same(ops.mx6_axpby(_offset_view(a), w, ALPHA, BETA).cpu(),
                    ref.axpby_ref(a, wire, a_dtype), "view")
    cut = n - 13                                   # a half cut by n
    ref.assert_same(ops.mx6_axpby(a[:cut].cuda(), torch.from_numpy(_decode_case(cut)).cuda(),
                                  ALPHA, BETA).cpu(), ref.axpby_ref(a, wire, a_dtype)[:cut], "cut")
    if a_dtype == dst_dtype:
        acc = a.cuda()
        assert ops.mx6_axpby(acc, w, ALPHA, BETA, dst=acc) is acc
        ref.assert_same(acc.cpu(), want, "in place")


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_forwarding_step_equals_the_two_steps(dtype, monkeypatch):
    import lzy_amd.ops as ops
    from lzy_amd.channels import mxwire
    from lzy_amd.exceptions import NativeExtensionMissing

    g = torch.Generator().manual_seed(5)
    a, b = (torch.randn(4096 + 5, generator=g).to(dtype).cuda() for _ in range(2))
    wire = ops.mx6_pack(b)
    axpby_pack, axpby2_pack = mxwire.wire_fused("mxfp6")
    for got, want in ((axpby_pack(a, wire, ALPHA, BETA), ops.mx6_axpby(a, wire, ALPHA, BETA)),
                      (axpby2_pack(a, b, ALPHA, BETA), ops.axpby(a, b, ALPHA, BETA))):
        assert torch.equal(got[0].view(torch.uint8), want.view(torch.uint8))
        assert torch.equal(got[1], ops.mx6_pack(want))
    monkeypatch.setattr(ops, "_MX6", False)    # a library without the exports
    with pytest.raises(NativeExtensionMissing):
        ops.mx6_pack(a)


@requires_gpu
def test_pair_two_ranks_device_tensors(tmp_path, monkeypatch):
    monkeypatch.setenv("MXFP6_DEVICE", "cuda")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    out = _torchrun("tests/mxfp6_script.py", 2, tmp_path, timeout=180)
    assert "MXFP6-PAIR-OK" in out and "MXFP6-PLAN-OK" not in out
