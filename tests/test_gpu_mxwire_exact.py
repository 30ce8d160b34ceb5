"""The five MXFP8 device code paths (lz_mx8_pack, lz_mx8_unpack,
lz_mx8_axpby, both directions of lz_segcodec) on MI355X (gfx950), bit for
bit against the references of tests/kernel_refs.py, which are written from
docs/mxwire.md in float64 and share nothing with the codec under test.

Inputs are the scale set (every scale byte, both sides of every boundary of
the scale rule), the tie set (every e4m3 code, every tie, both sides of
each) and the decode set (every payload code under every scale byte); their
coverage is asserted where they are built.  NaN is compared by position,
everything else as bits, so the sign of a zero counts.  These tests REQUIRE
the native extension: a missing libhipops.so fails loudly."""
import itertools
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import kernel_refs as kr
from mxwire_util import assert_wire_equal

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
IDS = [NAMES[d] for d in DTYPES]
RUNS = ["default", "capped2", "view"]
GUARD = 256


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


def _offset_view(t_cpu):
    """``t_cpu`` on the device as a view one element into a larger buffer:
    only element-aligned, which takes the kernels' guarded path."""
    base = torch.empty(t_cpu.numel() + 1, dtype=t_cpu.dtype, device="cuda")
    base[1:] = t_cpu.cuda()
    view = base[1:]
    assert view.data_ptr() % 16 != 0
    return view


def _guarded(nbytes, fill=0xCD):
    """(whole buffer, its middle ``nbytes``) of sentinel bytes."""
    big = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    return big, big[GUARD: GUARD + nbytes]


def _guards_untouched(big, nbytes, fill=0xCD):
    host = big.cpu()
    return bool((host[:GUARD] == fill).all() and (host[GUARD + nbytes:] == fill).all())


# ---------------------------------------------------------------------------
# mx8_pack
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("kind", ["scale", "tie"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_bit_exact(dtype, kind, run):
    from lzy_amd.ops import mx8_nbytes, mx8_pack

    x, want = kr.mx_encode_case(kind, dtype)
    what = f"mx8_pack {kind} set {NAMES[dtype]} {run}"
    src = _offset_view(x) if run == "view" else x.cuda()
    big, out = _guarded(mx8_nbytes(x.numel()))
    with _capped(2 if run == "capped2" else 0):
        got = mx8_pack(src)
        assert mx8_pack(src, out=out) is out
        torch.cuda.synchronize()
    assert_wire_equal(x, got.cpu(), want, what)
    assert_wire_equal(x, out.cpu(), want, what + " out=")
    assert _guards_untouched(big, out.numel()), what


# ---------------------------------------------------------------------------
# mx8_unpack
# ---------------------------------------------------------------------------

def _unpack_guarded(wire_dev, n, dtype, lead_elems):
    """mx8_unpack into the middle of a sentinel buffer, ``lead_elems``
    elements past an aligned start; (decoded CPU tensor, guards intact)."""
    from lzy_amd.ops import mx8_unpack

    isz = torch.empty(0, dtype=dtype).element_size()
    big = torch.full(((n + lead_elems) * isz + 2 * GUARD,), 0xCD,
                     dtype=torch.uint8, device="cuda")
    lo = GUARD + lead_elems * isz
    out = big[lo: lo + n * isz].view(dtype)
    assert mx8_unpack(wire_dev, n, dtype, out=out) is out
    host = big.cpu()
    intact = bool((host[:lo] == 0xCD).all() and (host[lo + n * isz:] == 0xCD).all())
    return host[lo: lo + n * isz].view(dtype), intact


@requires_gpu
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_bit_exact(dtype, run):
    from lzy_amd.ops import mx8_unpack

    wire, n, bits, nan = kr.mx_decode_case(dtype)
    what = f"mx8_unpack decode set {NAMES[dtype]} {run}"
    src = _offset_view(wire) if run == "view" else wire.cuda()
    with _capped(2 if run == "capped2" else 0):
        got = mx8_unpack(src, n, dtype)
        out, intact = _unpack_guarded(src, n, dtype, 1 if run == "view" else 0)
        torch.cuda.synchronize()
    kr.assert_bits_equal(got.cpu(), bits, nan, what)
    kr.assert_bits_equal(out, bits, nan, what + " out=")
    assert intact, what


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unpack_sizes_that_cut_a_block(dtype):
    """n = 1, 31, 33, 257 on a run of the decode set that starts at payload
    code 0xA0 under scale byte 110 (negative values that underflow f16),
    aligned and element-aligned: exact bits, nothing written past n."""
    wire, n_all, _, _ = kr.mx_decode_case(dtype)
    first = 8 * 110 + 5
    for n in (1, 31, 33, 257):
        nblk = (n + 31) // 32
        payload = wire[32 * first: 32 * (first + nblk)]
        scales = wire[n_all + first: n_all + first + nblk]
        bits, nan = kr.mx8_unpack_ref(payload.numpy(), scales.numpy(), n, dtype)
        sub = torch.cat([payload, scales]).cuda()
        for lead in (0, 1):
            what = f"mx8_unpack {NAMES[dtype]} n={n} lead={lead}"
            out, intact = _unpack_guarded(sub, n, dtype, lead)
            kr.assert_bits_equal(out, bits, nan, what)
            assert intact, what


# ---------------------------------------------------------------------------
# pack_tensors_wire / unpack_tensors_wire
# ---------------------------------------------------------------------------

SLICE = 3 * 8192 + 37
# where the slice of each scale set starts (a block boundary): the run that
# ends among the Inf and NaN leaders
_SLICE_BLOCK = {F32: 1533 - 770, BF16: 0x7F80 - 400, F16: 0x7C00 - 400}

_SLICES = {}


def _scale_slice(dtype):
    if dtype not in _SLICES:
        x, _ = kr.mx_encode_case("scale", dtype)
        s = 32 * _SLICE_BLOCK[dtype]
        part = x[s: s + SLICE].clone()
        assert part.numel() == SLICE and torch.isnan(part.float()).any()
        _SLICES[dtype] = (part, kr.mx8_wire_ref(part))
    return _SLICES[dtype]


def _raw(nbytes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)


@requires_gpu
@pytest.mark.parametrize("cap", [0, 2], ids=["default", "capped2"])
def test_bundle_encode_bit_exact(cap):
    from lzy_amd import ops

    leaves, wired, refs = [], [], []
    for dtype in DTYPES:
        for x, want in (kr.mx_encode_case("tie", dtype), _scale_slice(dtype)):
            raw = _raw(1 + 131 * len(leaves), 40 + len(leaves))
            leaves += [raw, x]
            wired += [False, True]
            refs += [raw, want]
    leaves.append(_raw(4099, 50))
    wired.append(False)
    refs.append(leaves[-1])
    with _capped(cap):
        buf, offs = ops.pack_tensors_wire([t.cuda() for t in leaves], wired)
        torch.cuda.synchronize()
    host = buf.cpu()
    covered = torch.zeros(host.numel(), dtype=torch.bool)
    for x, w, ref, off in zip(leaves, wired, refs, offs):
        seg = host[off: off + ref.numel()]
        covered[off: off + ref.numel()] = True
        if w:
            assert_wire_equal(x, seg, ref, f"wired leaf {NAMES[x.dtype]} n={x.numel()}")
        else:
            assert torch.equal(seg, ref)
    assert host[~covered].eq(0).all()              # the gaps are zeroed


@requires_gpu
@pytest.mark.parametrize("cap", [0, 2], ids=["default", "capped2"])
def test_bundle_decode_bit_exact(cap):
    from lzy_amd import ops

    wire, n, _, _ = kr.mx_decode_case(F32)
    head, mid, tail = _raw(77, 60), _raw(1000, 61), _raw(300, 62)
    segs = [head, wire, mid, wire, wire, tail]
    wired = [False, True, False, True, True, False]
    shapes = [(77,), (n,), (1000,), (n,), (n,), (75,)]
    dtypes = [torch.uint8, F32, torch.uint8, BF16, F16, torch.int32]
    woffs, total = ops.segcopy_layout([s.numel() for s in segs], 128)
    wbuf = torch.zeros(total, dtype=torch.uint8)
    for seg, off in zip(segs, woffs):
        wbuf[off: off + seg.numel()] = seg
    with _capped(cap):
        out, offs = ops.unpack_tensors_wire(wbuf.cuda(), wired, shapes, dtypes)
        torch.cuda.synchronize()
    got = [t.cpu() for t in ops.unpack_tensors(out, offs, shapes, dtypes)]
    assert torch.equal(got[0], head) and torch.equal(got[2], mid)
    assert torch.equal(got[5], tail.view(torch.int32))
    for k in (1, 3, 4):
        _, _, bits, nan = kr.mx_decode_case(dtypes[k])
        kr.assert_bits_equal(got[k], bits, nan, f"bundle decode {NAMES[dtypes[k]]}")


# ---------------------------------------------------------------------------
# mx8_axpby
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("pair", list(itertools.product(DTYPES, DTYPES)),
                         ids=lambda p: f"{NAMES[p[0]]}-{NAMES[p[1]]}")
def test_axpby_decodes_every_code_under_every_scale(pair):
    """a = 0, alpha = 0, beta = 1 leaves fma(0, 0, x^) = x^: the f32 decode,
    rounded to the destination.  The f32 decode is exact or Inf, so that is
    the reference's decode straight to the destination dtype.  By value: the
    fma turns -0.0 into +0.0, which is the documented formula.  NaN and Inf
    positions must match (Inf == Inf as values)."""
    from lzy_amd.ops import mx8_axpby

    a_dtype, dst_dtype = pair
    wire, n, bits, nan = kr.mx_decode_case(dst_dtype)
    want = kr.from_bits(bits, dst_dtype).double()
    if dst_dtype == F16:
        assert torch.isinf(want).sum().item() == 28342
    a = torch.zeros(n, dtype=a_dtype, device="cuda")
    dst = torch.empty(n, dtype=dst_dtype, device="cuda")
    assert mx8_axpby(a, wire.cuda(), 0.0, 1.0, dst=dst) is dst
    got = dst.cpu()
    gn = torch.isnan(got.float()).numpy()
    assert (gn == nan).all(), np.nonzero(gn != nan)[0][:8].tolist()
    keep = torch.from_numpy(~nan)
    bad = (got.double() != want) & keep
    assert not bad.any(), (
        f"{int(bad.sum())} elements differ; first at "
        f"{bad.nonzero().flatten()[:8].tolist()}: got "
        f"{got[bad][:8].tolist()} want {want[bad][:8].tolist()}")
