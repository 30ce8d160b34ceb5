"""The MXFP8 references of tests/kernel_refs.py (written from
docs/mxwire.md in float64) checked on cases worked by hand, and the torch
codecs of lzy_amd.channels.mxwire held to them, bit for bit, on the scale,
tie and decode sets.  No GPU."""
import numpy as np
import pytest
import torch

import kernel_refs as kr
from mxwire_util import assert_wire_equal, special_vector

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = ["f32", "bf16", "f16"]


# ---------------------------------------------------------------------------
# the references on cases worked by hand
# ---------------------------------------------------------------------------

def test_e4m3_table_by_hand():
    t = kr.e4m3_table()
    assert t[0x00] == 0 and not np.signbit(t[0x00])
    assert t[0x80] == 0 and np.signbit(t[0x80])
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9   # subnormals
    assert t[0x08] == 2.0 ** -6                               # smallest normal
    assert t[0x38] == 1.0 and t[0x3C] == 1.5 and t[0x46] == 3.5
    assert t[0x76] == 224 and t[0x78] == 256 and t[0x7E] == 448
    assert t[0xFE] == -448 and t[0xB8] == -1.0
    assert np.isnan(t[[0x7F, 0xFF]]).all() and np.isnan(t).sum() == 2
    fin = t[:0x7F]
    assert (np.diff(fin) > 0).all()                            # byte order = value order


def test_pack_ref_special_vector_by_hand():
    """[zeros] [nan,1,0..] [inf,-inf,2,0..] [896,-1.75,3e38,1e-45,0..]:
    amax 0, 1, 2 and 3e38.  1 * 2^8 = 256 <= 448 < 1 * 2^9: b = 119;
    2 * 2^7: b = 120; 3e38 * 2^-120 = 225.7 lies in (224, 448]: b = 247."""
    payload, scales = kr.mx8_pack_ref(special_vector())
    assert scales.tolist() == [0, 119, 120, 247]
    p = payload.tolist()
    assert p[:32] == [0] * 32
    assert p[32:35] == [0x7F, 0x78, 0x00]          # NaN, 256, +0
    assert p[64:68] == [0x7E, 0xFE, 0x78, 0x00]    # +-Inf saturate, 2 * 2^7 = 256
    # 896 * 2^-120 and 1e-45 * 2^-120 vanish, -1.75 * 2^-120 keeps its sign,
    # 225.7 is nearer 224 than 240
    assert p[96:101] == [0x00, 0x80, 0x76, 0x00, 0x00]


def test_pack_ref_amax_448_and_the_next_f32_by_hand():
    up = float(np.nextafter(np.float32(448), np.float32(np.inf)))
    a = torch.zeros(32)
    a[:10] = torch.tensor([448.0, -448.0, 1.0, 2.0 ** -10, -(2.0 ** -10),
                           1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 447.0, 0.0, -0.0])
    b = torch.zeros(32)
    b[:6] = torch.tensor([up, 1.0, -3.0, 2.0 ** -9, 3 * 2.0 ** -9, -448.0])
    payload, scales = kr.mx8_pack_ref(torch.cat([a, b]))
    # amax == 448 needs no scaling; one ulp more and everything is halved
    assert scales.tolist() == [127, 128]
    # 2^-10 ties between 0 and 2^-9: even code 0, the sign kept; 1.5 * 2^-9
    # and 2.5 * 2^-9 both tie to code 2; 447 is nearer 448 than 416
    assert payload[:10].tolist() == [0x7E, 0xFE, 0x38, 0x00, 0x80, 0x02, 0x02,
                                     0x7E, 0x00, 0x80]
    assert payload[10:32].eq(0).all()
    # 224 + 2^-16 -> 224; 0.5; -1.5; 2^-10 tie -> 0; 1.5 * 2^-9 tie -> 2; -224
    assert payload[32:38].tolist() == [0x76, 0x30, 0xBC, 0x00, 0x02, 0xF6]


def test_pack_ref_pads_with_zero_and_ignores_non_finite_for_amax():
    x = torch.tensor([float("inf"), float("nan"), float("-inf"), 3.0, -0.0])
    payload, scales = kr.mx8_pack_ref(x)
    assert scales.tolist() == [120]                # amax 3: 3 * 2^7 = 384 <= 448 < 768
    assert payload[:5].tolist() == [0x7E, 0x7F, 0xFE, 0x7C, 0x80]   # 384 = 12 * 2^5
    assert payload.numel() == 32 and payload[5:].eq(0).all()
    w = torch.full((32,), float("inf"))
    w[3] = float("nan")
    assert kr.mx8_pack_ref(w)[1].tolist() == [0]   # no finite element: b = 0


def test_pack_one_nan_byte_whatever_the_sign_or_payload():
    """The wire has one NaN byte, 0x7f: quiet and signalling NaNs of both
    signs (the device convert would keep the sign: 0xff)."""
    from lzy_amd.channels.mxwire import mx8_pack_torch

    bits = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0xFFFFFFFF]
    x = torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32)).view(F32)
    x = torch.cat([x, torch.tensor([1.0])])
    payload, scales = kr.mx8_pack_ref(x)
    assert payload[:6].tolist() == [0x7F] * 5 + [0x78] and scales.tolist() == [119]
    assert torch.equal(mx8_pack_torch(x), torch.cat([payload, scales]))
    for dtype, neg_nan in ((BF16, 0xFFC0), (F16, 0xFE00)):
        h = torch.tensor(np.array([neg_nan, neg_nan | 1], dtype=np.uint16)
                         .view(np.int16)).view(dtype)
        assert kr.mx8_wire_ref(h)[:2].tolist() == [0x7F, 0x7F]
        assert mx8_pack_torch(h)[:2].tolist() == [0x7F, 0x7F]


_DECODE_BY_HAND = [
    # code, scale byte, dtype, expected bits
    (0x78, 119, F32, 0x3F800000),    # 256 * 2^-8 = 1
    (0x80, 200, F32, 0x80000000),    # -0 under any scale
    (0x80, 200, F16, 0x8000),
    (0x80, 200, BF16, 0x8000),
    (0x7E, 254, F32, 0x7F800000),    # 448 * 2^127 overflows
    (0x7E, 254, BF16, 0x7F80),
    (0xFE, 247, F32, 0xFF800000),    # -1.75 * 2^128
    (0x77, 247, F32, 0x7F700000),    # 240 * 2^120 = 1.875 * 2^127
    (0x01, 0, F32, 0x00002000),      # 2^-9 * 2^-127 = 2^13 * 2^-149
    (0x7E, 134, F16, 0x7B00),        # 57344 = 1.75 * 2^15
    (0x7E, 135, F16, 0x7C00),        # 114688 -> Inf
    (0x77, 135, F16, 0x7B80),        # 61440 = 1.875 * 2^15
    (0x70, 135, F16, 0x7800),        # 128 * 256 = 2^15
    # f16 subnormals are multiples of 2^-24; scale byte 110 is 2^-17
    (0x09, 110, F16, 0x0002),        # 9 * 2^-26 = 2.25 units
    (0x0A, 110, F16, 0x0002),        # 2.5: tie to even
    (0x0B, 110, F16, 0x0003),        # 2.75
    (0x0E, 110, F16, 0x0004),        # 3.5: tie to even
    (0x8E, 110, F16, 0x8004),
    (0x01, 111, F16, 0x0000),        # 2^-25: tie between 0 and 2^-24
    (0x81, 111, F16, 0x8000),        # ... and the zero keeps its sign
    (0x02, 111, F16, 0x0001),
    (0x03, 111, F16, 0x0002),        # 1.5 units: tie to even
    (0x81, 100, F16, 0x8000),        # -2^-36 underflows to -0
    (0x79, 127, BF16, 0x4390),       # 288 = 1.125 * 2^8
    # bf16 subnormals are multiples of 2^-133
    (0x0A, 1, BF16, 0x0002),         # 10 * 2^-135 = 2.5 units: tie to even
    (0x0E, 1, BF16, 0x0004),         # 3.5 units
    (0x0C, 0, BF16, 0x0002),         # b == 0 is 2^-127: 12 * 2^-136 = 1.5 units
    (0x8C, 0, BF16, 0x8002),
    (0x04, 0, BF16, 0x0000),         # 0.5 units: tie to 0
    (0x05, 0, BF16, 0x0001),         # 0.625 units
    (0x81, 0, BF16, 0x8000),         # -0.125 units -> -0
]


def test_unpack_ref_by_hand():
    for code, b, dtype, want in _DECODE_BY_HAND:
        payload = np.zeros(32, dtype=np.uint8)
        payload[0] = code
        bits, nan = kr.mx8_unpack_ref(payload, [b], 1, dtype)
        assert bits.shape == (1,) and not nan[0]
        assert int(bits[0]) == want, (hex(code), b, dtype, hex(int(bits[0])))
    for dtype in DTYPES:
        for code in (0x7F, 0xFF):
            payload = np.full(32, code, dtype=np.uint8)
            assert kr.mx8_unpack_ref(payload, [127], 32, dtype)[1].all()


def test_decode_set_counts():
    """What the decode set holds, counted on the reference's output."""
    sign = {F32: 0x80000000, BF16: 0x8000, F16: 0x8000}
    inf = {F32: 0x7F800000, BF16: 0x7F80, F16: 0x7C00}
    counts = {}
    for dtype in DTYPES:
        wire, n, bits, nan = kr.mx_decode_case(dtype)
        assert n == 65280 and wire.numel() == 33 * 255 * 8
        mag = bits & (sign[dtype] - 1)
        counts[dtype] = (int(((bits == sign[dtype]) & ~nan).sum()),
                         int(((mag == inf[dtype]) & ~nan).sum()))
    # one 0x80 per scale byte, plus what underflows the destination
    assert counts == {F32: (255, 560), BF16: (262, 560), F16: (13066, 28342)}


# ---------------------------------------------------------------------------
# the torch codecs against the references
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["scale", "tie"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_torch_pack_equals_ref(dtype, kind):
    from lzy_amd.channels.mxwire import mx8_pack_torch

    x, want = kr.mx_encode_case(kind, dtype)
    assert x.dtype == dtype
    if kind == "scale":
        assert x.numel() == (49056 if dtype == F32 else 2097152)
    assert_wire_equal(x, mx8_pack_torch(x), want, f"{kind} set")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_torch_unpack_equals_ref(dtype):
    from lzy_amd.channels.mxwire import mx8_unpack_torch

    wire, n, bits, nan = kr.mx_decode_case(dtype)
    got = mx8_unpack_torch(wire, n, dtype)
    assert got.dtype == dtype and got.shape == (n,)
    kr.assert_bits_equal(got, bits, nan, "decode set")
    # and the wires of the tie sets of every source dtype, cut mid-block
    for src in DTYPES:
        x, w = kr.mx_encode_case("tie", src)
        m = x.numel() - 13                          # same blocks, the last cut
        sb, sn = kr.mx8_unpack_ref(w[: x.numel()].numpy(), w[x.numel():].numpy(),
                                   m, dtype)
        kr.assert_bits_equal(mx8_unpack_torch(w, m, dtype), sb, sn, "tie wire")


def _raw(nbytes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)


def test_torch_bundle_codecs_equal_ref():
    """A bundle whose wired leaves are the tie sets (encode) and the decode
    set as a leaf of each dtype (decode), between two raw leaves."""
    from lzy_amd import ops

    head, tail = _raw(77, 1), _raw(300, 2).view(torch.int32)
    ties = [kr.mx_encode_case("tie", d) for d in DTYPES]
    leaves = [head] + [x for x, _ in ties] + [tail]
    wired = [False, True, True, True, False]
    buf, offs = ops.pack_tensors_wire_torch(leaves, wired)
    for (x, want), off in zip(ties, offs[1:4]):
        assert off % 128 == 0
        assert_wire_equal(x, buf[off: off + want.numel()], want, "bundle segment")
    assert torch.equal(buf[offs[0]: offs[0] + 77], head)
    assert torch.equal(buf[offs[4]: offs[4] + 300], tail.view(torch.uint8))

    wire, n, _, _ = kr.mx_decode_case(F32)
    sizes = [77] + [wire.numel()] * 3 + [300]
    woffs, total = ops.segcopy_layout(sizes, 128)
    wbuf = torch.zeros(total, dtype=torch.uint8)
    for seg, off in zip([head, wire, wire, wire, tail.view(torch.uint8)], woffs):
        wbuf[off: off + seg.numel()] = seg
    shapes = [(77,), (n,), (n,), (n,), (75,)]
    dtypes = [torch.uint8] + DTYPES + [torch.int32]
    out, eoffs = ops.unpack_tensors_wire_torch(wbuf, wired, shapes, dtypes)
    got = ops.unpack_tensors(out, eoffs, shapes, dtypes)
    assert torch.equal(got[0], head) and torch.equal(got[4], tail)
    for leaf, dtype in zip(got[1:4], DTYPES):
        _, _, bits, nan = kr.mx_decode_case(dtype)
        kr.assert_bits_equal(leaf, bits, nan, f"bundle decode {dtype}")
