"""The MXFP4 kernels (lz_mx4_pack / _unpack / _axpby) against the float64
reference of tests/test_mxfp4.py, bit for bit, and the pair primitive with
device tensors (docs/mxwire.md, "MXFP4").
"""
import numpy as np
import pytest
import torch

import test_mxfp4 as ref
from test_mxfp4 import ALPHA, BETA, DTYPES, F32, IDS
from test_gpu_mxwire_exact import _capped, _offset_view
from test_mxplan import _torchrun

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
GUARD = 64

# (numel, where the slice of the cyclic encode inputs starts, grid cap, offset view)
PACK_CASES = [(1, 32 * 16, 0, False), (7, 32 * 17 + 9, 0, False), (31, 32 * 20 + 1, 0, False),
              (32, 32 * 21, 0, False), (33, 32 * 22 - 1, 0, False),
              (4096 + 5, 0, 0, False), (4096 + 5, 0, 0, True),
              ((1 << 18) + 37, 0, 2, False)]


@requires_gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"n{c[0]}cap{c[2]}view{int(c[3])}")
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_equals_reference(dtype, case):
    import lzy_amd.ops as ops

    n, start, cap, view = case
    base = ref.encode_inputs()
    x = base.repeat(-(-(start + n) // base.numel()))[start: start + n].to(dtype)
    want = ref.mx4_pack_ref(x.to(F32).numpy())
    with _capped(cap):
        got = ops.mx4_pack(_offset_view(x) if view else x.cuda()).cpu().numpy()
    assert got.size == ops.mx4_nbytes(n) == 17 * -(-n // 32)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def _decode_case(n):
    """The first n elements of the decode inputs: the scale bytes move up."""
    full, _ = ref.decode_inputs()
    nblk = -(-n // 32)
    return np.concatenate([full[: 16 * nblk], full[2560: 2560 + nblk]])


@requires_gpu
@pytest.mark.parametrize("n", [5120, 5120 - 13, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_equals_reference(dtype, n):
    import lzy_amd.ops as ops

    wire = _decode_case(n)
    want = ref.to_dtype(ref.mx4_unpack_ref(wire, n), dtype)
    for view in (False, True):
        buf = torch.full((n + GUARD + 1,), 7.0, dtype=dtype, device="cuda")
        out = buf[1: 1 + n] if view else buf[:n]
        ops.mx4_unpack(torch.from_numpy(wire).cuda(), n, dtype, out=out)
        ref.assert_same(out.cpu(), want, f"view={view}")
        rest = buf[1 + n:] if view else buf[n:]
        assert bool((rest == 7.0).all()) and (not view or float(buf[0]) == 7.0)


@requires_gpu
@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("a_dtype", DTYPES, ids=IDS)
def test_axpby_equals_reference(a_dtype, dst_dtype):
    import lzy_amd.ops as ops

    wire, n = ref.decode_inputs()
    a =ref.axpby_operand(wire, n).to(a_dtype)
    want = ref.axpby_ref(a, wire, dst_dtype)
    w = torch.from_numpy(wire).cuda()
    buf = torch.full((n + GUARD,), 7.0, dtype=dst_dtype, device="cuda")
    ops.mx4_axpby(a.cuda(), w, ALPHA, BETA, dst=buf[:n])
    ref.assert_same(buf[:n].cpu(), want)
    assert bool((buf[n:] == 7.0).all())
    ref.assert_same(ops.mx4_axpby(_offset_view(a), w, ALPHA, BETA).cpu(),
                    ref.axpby_ref(a, wire, a_dtype), "view")
    if a_dtype == dst_dtype:
        acc = a.cuda()
        assert ops.mx4_axpby(acc, w, ALPHA, BETA, dst=acc) is acc
        ref.assert_same(acc.cpu(), want, "in place")


@requires_gpu
def test_pair_two_ranks_device_tensors(tmp_path, monkeypatch):
    monkeypatch.setenv("MXFP4_DEVICE", "cuda")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    out = _torchrun("tests/mxfp4_pair_script.py", 2, tmp_path, timeout=180)
    assert "MXFP4-PAIR-OK" in out
