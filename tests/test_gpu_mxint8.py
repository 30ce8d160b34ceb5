"""The MXINT8 kernels (lz_mxi8_pack / _unpack / _axpby) against the float64
reference of tests/test_mxint8.py, bit for bit, and the pair primitive with
device tensors (docs/mxwire.md, "MXINT8").
"""
import numpy as np
import pytest
import torch

import test_mxint8 as ref
from test_mxint8 import ALPHA, BETA, DTYPES, F32, IDS
from test_gpu_mxwire_exact import _capped, _offset_view
from test_mxplan import _torchrun

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
GUARD = 64


def _cyclic(base, n, start):
    reps = -(-(start + n) // base.numel())
    return base.repeat(reps)[start: start + n].clone()


# (numel, where the slice of the cyclic inputs starts, grid cap, offset view)
PACK_CASES = [(1, 0, 0, False), (7, 32 * 5, 0, False), (31, 32 * 21, 0, False),
              (32, 32 * 30, 0, False), (33, 32 * 29 + 20, 0, False),
              (4096 + 5, 0, 0, False), (4096 + 5, 0, 0, True),
              ((1 << 18) + 37, 0, 2, False)]


@requires_gpu
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"n{c[0]}cap{c[2]}view{int(c[3])}")
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_equals_reference(dtype, case):
    import lzy_amd.ops as ops

    n, start, cap, view = case
    x = _cyclic(ref.encode_inputs(), n, start).to(dtype)
    want = ref.mxi8_pack_ref(x.to(F32).numpy())
    dev = _offset_view(x) if view else x.cuda()
    with _capped(cap):
        got = ops.mxi8_pack(dev).cpu().numpy()
    assert got.size == ops.mx8_nbytes(n)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


@requires_gpu
@pytest.mark.parametrize("n", [2560, 2560 - 13, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_equals_reference(dtype, n):
    """All 256 codes under every scale byte of the CPU test; sizes that cut a
    block (the wire buffer of the cut sizes keeps the scale bytes in place);
    the bytes past dst[n) stay as they were."""
    import lzy_amd.ops as ops

    full, _ = ref.decode_inputs()
    nblk = -(-n // 32)
    wire = np.concatenate([full[: 32 * nblk], full[2560: 2560 + nblk]])
    want = ref.to_dtype(ref.mxi8_unpack_ref(wire, n), dtype)
    for view in (False, True):
        buf = torch.full((n + GUARD + 1,), 7.0, dtype=dtype, device="cuda")
        out = buf[1: 1 + n] if view else buf[:n]
        ops.mxi8_unpack(torch.from_numpy(wire).cuda(), n, dtype, out=out)
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
    ops.mxi8_axpby(a.cuda(), w, ALPHA, BETA, dst=buf[:n])
    ref.assert_same(buf[:n].cpu(), want)
    assert bool((buf[n:] == 7.0).all())
    ref.assert_same(ops.mxi8_axpby(_offset_view(a), w, ALPHA, BETA).cpu(),
                    ref.axpby_ref(a, wire, a_dtype), "view")
    if a_dtype == dst_dtype:
        acc = a.cuda()
        assert ops.mxi8_axpby(acc, w, ALPHA, BETA, dst=acc) is acc
        ref.assert_same(acc.cpu(), want, "in place")


@requires_gpu
def test_pair_two_ranks_device_tensors(tmp_path, monkeypatch):
    """Both ranks on one GPU: kernel pack, packed bytes staged through the
    host, kernel decode-combine.  The script holds the result to the one-hop
    bound and to bit equality with the torch codec on the same inputs."""
    monkeypatch.setenv("MXINT8_DEVICE", "cuda")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    out = _torchrun("tests/mxint8_pair_script.py", 2, tmp_path, timeout=180)
    assert "MXINT8-PAIR-OK" in out
