"""Host references for the data-plane kernels in lzy_amd/ops/hipops.hip.

Every function here is written from the operation's definition (the comments
and bodies of the kernels), with numpy / torch on the CPU only: no GPU and
no import of lzy_amd.ops.  The GPU tests compare the kernels with these and
tests/test_kernel_refs.py checks the references themselves."""
import functools

import numpy as np
import torch

MASK64 = (1 << 64) - 1
LZ_BLOCK = 256            # threads per block, hipops.hip
LZ_MAX_BLOCKS = 1024      # default grid cap, hipops.hip

FP8_MAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def splitmix64(x):
    """splitmix64 output function, vectorised over uint64 (wrapping)."""
    with np.errstate(over="ignore"):
        x = _u64(x) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _wsum(a) -> int:
    """Wrapping 64-bit sum of a uint64 array as a python int."""
    with np.errstate(over="ignore"):
        return int(np.sum(_u64(a), dtype=np.uint64)) & MASK64


def _le_bytes_to_int(b: bytes) -> int:
    return int.from_bytes(b, "little")


def checksum_valu_ref(data: bytes) -> int:
    """checksum_kernel: every full u64 word i contributes
    splitmix64(word ^ splitmix64(i)) (the kernel reads them in pairs and
    takes an odd last word on its own; the salt is the word index either
    way), the <= 7 tail bytes one term with the 0xA5A5A5A5 marker, the
    length one term; all summed modulo 2^64."""
    data = bytes(data)
    nbytes = len(data)
    nwords = nbytes >> 3
    words = np.frombuffer(data, dtype="<u8", count=nwords)
    acc = _wsum(splitmix64(words ^ splitmix64(np.arange(nwords, dtype=np.uint64))))
    if nbytes & 7:
        last = _le_bytes_to_int(data[nwords << 3:])
        acc += int(splitmix64(_u64(last) ^ splitmix64(nwords) ^ np.uint64(0xA5A5A5A5)))
    acc += int(splitmix64(_u64(nbytes) ^ np.uint64(0x1234567890ABCDEF)))
    return acc & MASK64


def mfma_grid_blocks(nbytes: int, max_blocks: int = LZ_MAX_BLOCKS) -> int:
    """Blocks lz_checksum_mfma launches (4 waves each)."""
    want = ((nbytes >> 10) // 4 + 3) // 4
    return max(1, min(want, max_blocks))


def _mfma_a_bytes() -> np.ndarray:
    """A operand: lane l, dword r = low32(splitmix64(0x5EED*131 + 4l + r))
    | 0x01010101; as signed bytes [64 lanes, 16]."""
    idx = np.uint64(0x5EED * 131) + np.arange(256, dtype=np.uint64)
    dw = (splitmix64(idx) & np.uint64(0xFFFFFFFF)).astype("<u4") | np.uint32(0x01010101)
    return dw.view(np.int8).reshape(64, 16)


def checksum_mfma_ref(data: bytes, max_blocks: int = LZ_MAX_BLOCKS) -> int:
    """checksum_mfma_kernel.

    Per 1 KiB tile t, lane l owns bytes [16l, 16l+16); dword r of it is
    XORed with low32(splitmix64(t) >> ((13 r) & 31)).  One
    v_mfma_i32_32x32x32_i8 adds, over Z_2^32,
        D[i][j] += sum_{h in {0,1}} sum_{b<16} A8[i+32h][b] * B8[j+32h][b]
    (A and B use the same (half, byte) -> k map, so it cancels).  Register r
    of lane l holds D[(r&3) + 8(r>>2) + 4(l>>5)][l&31].

    Each wave keeps its own accumulator over the tiles t = wave (mod number
    of waves) and folds its 16 registers per lane with position salts, so
    the digest is a function of the bytes AND of the launch grid
    (mfma_grid_blocks); waves without tiles fold zeros.  Then the sub-1-KiB
    tail (u64 words salted with 128*ntiles + i, the byte tail unsalted), the
    length term, wrapping sum."""
    data = bytes(data)
    nbytes = len(data)
    ntiles = nbytes >> 10
    nwaves = 4 * mfma_grid_blocks(nbytes, max_blocks)

    a8 = _mfma_a_bytes().astype(np.int64)                      # [64, 16]
    tiles = np.frombuffer(data, dtype="<u4", count=ntiles * 256).reshape(ntiles, 64, 4)
    s = splitmix64(np.arange(ntiles, dtype=np.uint64))         # [ntiles]
    shifts = _u64([(13 * r) & 31 for r in range(4)])           # [4]
    salt = ((s[:, None] >> shifts[None, :]) & np.uint64(0xFFFFFFFF)).astype("<u4")
    b8 = (tiles ^ salt[:, None, :]).astype("<u4").view(np.int8).reshape(ntiles, 64, 16)

    lane = np.arange(64)
    reg = np.arange(16)
    row = (reg[None, :] & 3) + 8 * (reg[None, :] >> 2) + 4 * (lane[:, None] >> 5)
    col = np.broadcast_to((lane & 31)[:, None], (64, 16))
    fold_salt = splitmix64((lane[:, None] * 16 + reg[None, :]).astype(np.uint64))

    h = 0
    for w in range(nwaves):
        bsum = b8[w::nwaves].astype(np.int64).sum(axis=0)      # [64, 16]
        d = a8[:32] @ bsum[:32].T + a8[32:] @ bsum[32:].T      # [32, 32] int64
        acc = (d[row, col] & 0xFFFFFFFF).astype(np.uint64)     # [64, 16]
        h += _wsum(splitmix64(acc ^ fold_salt))

    tail = data[ntiles << 10:]
    nwords = len(tail) >> 3
    words = np.frombuffer(tail, dtype="<u8", count=nwords)
    idx = np.uint64(ntiles * 128) + np.arange(nwords, dtype=np.uint64)
    h += _wsum(splitmix64(words ^ splitmix64(idx)))
    if len(tail) & 7:
        last = _le_bytes_to_int(tail[nwords << 3:])
        h += int(splitmix64(_u64(last) ^ np.uint64(0xA5A5A5A5)))
    h += int(splitmix64(_u64(nbytes) ^ np.uint64(0x1234567890ABCDEF)))
    return h & MASK64


def fill_pattern_ref(nbytes: int, seed: int, mask16: int = 0) -> bytes:
    """fill_pattern_kernel: u64 word i = splitmix64(seed ^ i), every 16-bit
    lane ANDed with mask16 when it is non-zero; the trailing nbytes % 8
    bytes are the low bytes of word nbytes // 8."""
    nwords = (nbytes + 7) >> 3
    w = splitmix64(_u64(seed & MASK64) ^ np.arange(nwords, dtype=np.uint64))
    if mask16:
        w = w & _u64((mask16 & 0xFFFF) * 0x0001000100010001)
    return w.astype("<u8").tobytes()[:nbytes]


def fp8_cast_ref(x_f32: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """f32 -> fp8 as __hip_fp8_e4m3 / __hip_fp8_e5m2 define it with their
    default finite saturation: round to nearest even of clamp(x, -max, max);
    NaN stays NaN.  (torch's own cast does not clamp: it yields NaN / Inf
    beyond the range.)  +-Inf clamps to +-max here; the hardware's answer
    for Inf is not part of the contract, callers compare it separately."""
    x = x_f32.to(torch.float32)
    m = FP8_MAX[dtype]
    return torch.clamp(x, -m, m).to(dtype)


# ---------------------------------------------------------------------------
# boundary-value generators (all CPU tensors)
# ---------------------------------------------------------------------------

def all_bits16(dtype: torch.dtype) -> torch.Tensor:
    """All 65536 bit patterns of a 16-bit float format."""
    assert dtype in (torch.float16, torch.bfloat16)
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)  # wraps
    return bits.view(dtype)


def all_codes8(dtype: torch.dtype) -> torch.Tensor:
    """All 256 codes of an fp8 format."""
    assert dtype in FP8_MAX
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(dtype)


def _finite_values_f64(dtype: torch.dtype) -> np.ndarray:
    """Sorted distinct finite non-negative values of a narrow format."""
    if dtype in FP8_MAX:
        v = all_codes8(dtype).to(torch.float32)
    else:
        v = all_bits16(dtype).to(torch.float32)
    v = v[torch.isfinite(v)].double().numpy()
    return np.unique(v[v >= 0])


def special_values_f32() -> torch.Tensor:
    sub = [1e-45, 3e-45, 1e-42, 1e-40, 5.877e-39, 1.1754942e-38]
    big = [1e30, 1e38, 3.4028234663852886e38]
    pos = torch.tensor(sub + big, dtype=torch.float32)
    return torch.cat([
        pos, -pos,
        torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf")]),
    ])


def narrowing_boundaries(dtype: torch.dtype) -> torch.Tensor:
    """f32 inputs at which an f32 -> dtype narrowing can go wrong: every
    representable value of the target, every midpoint between neighbours
    and both f32 neighbours of each midpoint; the first values beyond max
    (the would-be next value, the midpoint before it and that midpoint's
    neighbours), huge finite values, +-0, NaN, +-Inf and f32 subnormals.
    Both signs throughout."""
    vals = _finite_values_f64(dtype)                 # exact in f64
    top = 2 * vals[-1] - vals[-2]                    # next value past max
    grid = np.concatenate([vals, [top, 2 * vals[-1], 4 * vals[-1]]])
    mids = (grid[:-1] + grid[1:]) / 2
    f32_max = float(np.finfo(np.float32).max)        # bf16 reaches past it
    grid, mids = grid[grid <= f32_max], mids[mids <= f32_max]
    mids32 = mids.astype(np.float32)
    assert (mids32.astype(np.float64) == mids).all(), "midpoints must be exact in f32"
    grid32 = grid.astype(np.float32)
    assert (grid32.astype(np.float64) == grid).all()
    up = np.nextafter(mids32, np.float32(np.inf))
    dn = np.nextafter(mids32, np.float32(-np.inf))
    pos = torch.from_numpy(np.concatenate([grid32, mids32, up, dn]))
    return torch.cat([pos, -pos, special_values_f32()])


def fp8_nearest_bruteforce(x_f32: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Independent check of fp8_cast_ref: nearest of the decoded finite codes
    in f64, ties to the even code, saturating; returns uint8 codes.  NaN
    inputs give the format's canonical NaN code 0x7f | sign-less."""
    codes = torch.arange(128, dtype=torch.int32).to(torch.uint8)
    dec = codes.view(dtype).to(torch.float32).double()
    keep = torch.isfinite(dec)
    codes, dec = codes[keep].to(torch.int64), dec[keep]        # ascending
    x = x_f32.double()
    finite_x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    mag = finite_x.abs().clamp(max=float(dec[-1]))              # saturation
    dist = (mag[:, None] - dec[None, :]).abs()                  # [N, C]
    best = dist.min(dim=1, keepdim=True).values
    cand = dist == best                                         # 1 or 2 codes
    even = cand & ((codes & 1) == 0)[None, :]
    two = cand.sum(dim=1) > 1
    pick = torch.where(two[:, None], even, cand)
    assert (pick.sum(dim=1) == 1).all()
    out = codes[pick.to(torch.int64).argmax(dim=1)]
    out = out | (torch.signbit(x).to(torch.int64) << 7)
    out = torch.where(torch.isnan(x), torch.full_like(out, 0x7F), out)
    return out.to(torch.uint8)


# ---------------------------------------------------------------------------
# block-scaled FP8 wire format (docs/mxwire.md), written from the spec
#
# Plain float64 arithmetic: no torch fp8 dtype, no bit formula for the scale
# byte, nothing shared with lzy_amd.channels.mxwire.
# ---------------------------------------------------------------------------

MX_BLOCK = 32
MX_B_MAX = 247            # largest scale byte an encoder produces
MX_TIE_B = (0, 1, 8, 119, 127, 134, 246, 247)


def _np_f32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        assert x.dtype == torch.float32
        x = x.detach().reshape(-1).numpy()
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    return x


def e4m3_table() -> np.ndarray:
    """float64 value of every e4m3fn code, from its bit fields: sign, 4
    exponent bits (bias 7), 3 mantissa bits; exponent 0 is the subnormal
    m * 2^-9; 0x7f and 0xff are NaN (the format has no Inf)."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    mag = np.where(e == 0, m * 2.0 ** -9, np.ldexp(8 + m, e - 10))
    v = np.where(c >> 7 == 1, -mag, mag)
    v[[0x7F, 0xFF]] = np.nan
    return v


def mx8_pack_parts(x_f32) -> dict:
    """The encode of docs/mxwire.md step by step, float64 throughout:
    ``amax`` [nblk] over the finite elements, ``scales`` [nblk], ``scaled``
    [32*nblk] = x * 2^(127-b) and ``payload`` [32*nblk] (numpy arrays)."""
    x = _np_f32(x_f32)
    n = x.size
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    xp = np.zeros(nblk * MX_BLOCK, dtype=np.float64)     # padded tail: +0.0
    with np.errstate(invalid="ignore"):                  # signalling NaNs
        xp[:n] = x
    blk = xp.reshape(nblk, MX_BLOCK)
    amax = np.where(np.isfinite(blk), np.abs(blk), 0.0).max(axis=1, initial=0.0)
    # b: the smallest integer >= 0 with amax * 2^(127-b) <= 448.  With
    # amax/448 = f * 2^e, f in [0.5, 1), the smallest power of two that is
    # >= amax/448 is 2^e, or 2^(e-1) when f is exactly 0.5.  (The quotient
    # is rounded, but monotonically, and an f32 amax is never within 2^-53
    # relative of 448 * 2^k without being equal to it; the two checks below
    # do not depend on the division at all.)
    f, e = np.frexp(amax / 448.0)
    b = np.where(amax > 0, np.maximum(127 + e - (f == 0.5), 0), 0).astype(np.int64)
    assert (np.ldexp(amax, 127 - b) <= 448.0).all()
    assert ((b == 0) | (np.ldexp(amax, 128 - b) > 448.0)).all()
    assert b.max(initial=0) <= MX_B_MAX
    scaled = np.ldexp(blk, (127 - b)[:, None]).reshape(-1)
    # the scaled value is exact in f32 (a power-of-two multiple of an f32)
    # unless it falls below the f32 normal range, and there it is far under
    # 2^-10, half the smallest e4m3 step: a signed zero whichever way an
    # encoder's f32 multiply rounds or flushes it
    fin = np.isfinite(scaled)
    with np.errstate(over="ignore", under="ignore"):
        exact = scaled.astype(np.float32).astype(np.float64) == scaled
    assert (exact | (np.abs(scaled) < 2.0 ** -126))[fin].all()
    assert (np.abs(scaled[fin]) <= 448.0).all()
    # nearest finite e4m3 value, ties to the even code, +-Inf saturating to
    # +-448, NaN -> 0x7f, the sign bit from the input's sign (so a zero
    # result keeps it): brute force over the distinct bit patterns
    uniq, inv = np.unique(scaled.view(np.int64), return_inverse=True)
    codes = np.empty(uniq.size, dtype=np.uint8)
    for s in range(0, uniq.size, 1 << 16):
        part = torch.from_numpy(uniq[s: s + (1 << 16)].view(np.float64).copy())
        codes[s: s + (1 << 16)] = fp8_nearest_bruteforce(
            part, torch.float8_e4m3fn).numpy()
    payload = codes[inv.reshape(-1)]
    assert (payload[n:] == 0).all()
    return {"amax": amax, "scales": b.astype(np.uint8), "scaled": scaled,
            "payload": payload}


def mx8_pack_ref(x_f32):
    """(payload uint8[32*nblk], scales uint8[nblk]) of an f32 tensor; a
    16-bit input is widened to f32 (exactly) by the caller."""
    p = mx8_pack_parts(x_f32)
    return torch.from_numpy(p["payload"]), torch.from_numpy(p["scales"])


def mx8_wire_ref(x: torch.Tensor) -> torch.Tensor:
    """The whole wire buffer of a f32/bf16/f16 tensor: payload, then scales."""
    return torch.cat(mx8_pack_ref(x.detach().reshape(-1).to(torch.float32)))


_MX_BITS = {torch.float32: np.uint32, torch.float16: np.uint16,
            torch.bfloat16: np.uint16}


def mx8_unpack_ref(payload, scales, n: int, dtype: torch.dtype):
    """Decode: table value * 2^(b-127) in float64 (exact; b == 0 is 2^-127),
    then ONE round-to-nearest-even to ``dtype``.  Returns (bit patterns as a
    numpy unsigned array of the dtype's width, NaN mask); the bits at NaN
    positions are not part of the contract."""
    payload = np.asarray(payload, dtype=np.uint8).reshape(-1)
    scales = np.asarray(scales, dtype=np.int64).reshape(-1)
    nblk = (n + MX_BLOCK - 1) // MX_BLOCK
    assert payload.size == MX_BLOCK * nblk and scales.size == nblk
    q = e4m3_table()[payload].reshape(nblk, MX_BLOCK)
    v = np.ldexp(q, (scales - 127)[:, None]).reshape(-1)[:n]
    nan = np.isnan(v)
    v = np.where(nan, 0.0, v)
    with np.errstate(over="ignore"):
        if dtype == torch.float16:
            bits = v.astype(np.float16).view(np.uint16)   # numpy rounds f64 -> f16 once
        else:
            # 4 significant bits at 2^-136 or above: exact in f32 unless it
            # overflows (>= 2^128 -> Inf), so narrowing f32 on is still one
            # rounding of the exact value
            f = v.astype(np.float32)
            assert ((f.astype(np.float64) == v) | (np.abs(v) >= 2.0 ** 128)).all()
            bits = f.view(np.uint32)
            if dtype == torch.bfloat16:
                # RNE on the f32 bits; the carry may run into the exponent,
                # up to Inf, which is what rounding does; Inf stays Inf
                b64 = bits.astype(np.uint64)
                b64 = (b64 + np.uint64(0x7FFF) + ((b64 >> np.uint64(16)) & np.uint64(1)))
                bits = (b64 >> np.uint64(16)).astype(np.uint16)
            else:
                assert dtype == torch.float32
    return bits.astype(_MX_BITS[dtype]), nan


def bits_of(t: torch.Tensor) -> np.ndarray:
    """Bit patterns of a CPU f32/bf16/f16 tensor as a flat unsigned array."""
    t = t.detach().reshape(-1).contiguous()
    if t.element_size() == 4:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def is_nan_bits(bits: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    ebits, mbits = {torch.float32: (8, 23), torch.float16: (5, 10),
                    torch.bfloat16: (8, 7)}[dtype]
    b = bits.astype(np.int64)
    return ((b >> mbits) & ((1 << ebits) - 1) == (1 << ebits) - 1) & \
        (b & ((1 << mbits) - 1) != 0)


def from_bits(bits: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    if dtype == torch.float32:
        return torch.from_numpy(bits.astype(np.uint32).view(np.int32).copy()).view(dtype)
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(dtype)


# --- input sets -------------------------------------------------------------

# element k of a scale-set block is element 0 times _SCALE_FRACS[k], signs
# alternating; the rest of the block is zeros of both signs (times element
# 0, so a NaN or Inf block has no zero in it)
_SCALE_FRACS = [1.0, 1.0, 15 / 16, 9 / 16, 17 / 32, 3 / 32, 17 * 2.0 ** -10,
                2.0 ** -9, 1.5 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -11]


def _scale_leaders(dtype: torch.dtype) -> torch.Tensor:
    if dtype != torch.float32:
        return all_bits16(dtype)
    e = np.arange(255, dtype=np.int64)[:, None] << 23
    m = np.array([0, 1, 0x5FFFFF, 0x600000, 0x600001, 0x7FFFFF], dtype=np.int64)
    bits = np.concatenate([(e | m[None, :]).reshape(-1),
                           [0x7F800000, 0xFF800000, 0x7FC00000]])
    return torch.from_numpy(bits.astype(np.uint32).view(np.int32).copy()).view(dtype)


def mx_scale_set(dtype: torch.dtype) -> torch.Tensor:
    """One block per leading value: every bit pattern of a 16-bit dtype
    (65536 blocks, 2,097,152 elements); for f32 every exponent 0..254 with
    the mantissas {0, 1, 0x5FFFFF, 0x600000, 0x600001, 0x7FFFFF}, then +Inf,
    -Inf and NaN (1533 blocks, 49,056 elements).  The leader is the block's
    amax when finite; the fractions put elements on e4m3 ties, in the e4m3
    subnormal range and below it."""
    lead = _scale_leaders(dtype).to(torch.float64)
    frac = torch.zeros(MX_BLOCK, dtype=torch.float64)
    frac[: len(_SCALE_FRACS)] = torch.tensor(_SCALE_FRACS, dtype=torch.float64)
    frac[1::2] *= -1.0                                    # -0.0 in the zero slots
    out = (lead[:, None] * frac[None, :]).to(dtype)
    out[:, 0] = _scale_leaders(dtype)                     # the pattern itself
    return out.reshape(-1)


def check_scale_set(x: torch.Tensor, parts: dict) -> None:
    """Coverage of a scale set, from the reference's own amax and scale
    bytes.  Every scale byte the dtype can reach occurs: all of 0..247 for
    f32 and bf16; for f16 byte 0 (the zero blocks) and 95..135, 42 in all.
    And the boundary of the scale rule is hit from both sides: for every
    occurring b whose upper end 1.75 * 2^(b-119) (amax mantissa 0x600000)
    and the value after it are finite values of the dtype, one block has
    exactly that amax, with scale byte b, and one the next representable
    amax, with scale byte b + 1.  (Not representable: b = 247 everywhere
    -- past every maximum; f16's b = 0 and 95, 96, whose upper ends fall
    between f16 subnormals, and 135, past 65504.)"""
    dtype = x.dtype
    amax, b = parts["amax"], parts["scales"].astype(np.int64)
    occurring = sorted(set(b.tolist()))
    if dtype == torch.float16:
        assert occurring == [0] + list(range(95, 136)), occurring
    else:
        assert occurring == list(range(MX_B_MAX + 1)), occurring
    where = {}
    for a, s in zip(amax.tolist(), b.tolist()):
        where.setdefault(a, s)
    pos = all_bits16(dtype) if dtype != torch.float32 else None
    skipped = []
    for s in occurring:
        edge = 1.75 * 2.0 ** (s - 119)
        if dtype == torch.float32:
            ok = s < MX_B_MAX
            nxt = float(np.nextafter(np.float32(edge), np.float32(np.inf))) if ok else None
        else:
            e = torch.tensor(edge, dtype=torch.float64).to(dtype)
            ok = e.double().item() == edge and edge > 0
            nxt = None
            if ok:
                nb = pos[(int(e.view(torch.int16).item()) & 0xFFFF) + 1].double().item()
                ok, nxt = np.isfinite(nb), nb
        if not ok:
            skipped.append(s)
            continue
        assert np.frexp(edge)[0] == 0.875                 # mantissa 0x600000
        assert where.get(edge) == s, (s, edge, where.get(edge))
        assert where.get(nxt) == s + 1, (s, nxt, where.get(nxt))
    want_skipped = [0, 95, 96, 135] if dtype == torch.float16 else [MX_B_MAX]
    assert skipped == want_skipped, skipped


def _next_up_down(x64: np.ndarray, dtype: torch.dtype):
    """For positive float64 values: (x if the dtype holds it exactly else
    NaN, the largest dtype value below x, the smallest above x) as float64."""
    r = torch.from_numpy(x64).to(dtype)
    if dtype == torch.float32:
        rn = r.numpy()
        up = np.nextafter(rn, np.float32(np.inf)).astype(np.float64)
        dn = np.nextafter(rn, np.float32(-np.inf)).astype(np.float64)
    else:
        i = r.view(torch.int16).to(torch.int32)
        up = (i + 1).to(torch.int16).view(dtype).double().numpy()
        dn = (i - 1).clamp(min=0).to(torch.int16).view(dtype).double().numpy()
    rd = r.double().numpy()
    exact = rd == x64
    lo = np.where(rd < x64, rd, dn)
    hi = np.where(rd > x64, rd, up)
    return np.where(exact, x64, np.nan), lo, hi


def mx_tie_b(dtype: torch.dtype):
    """The scale bytes of the tie set.  f16 keeps those b of MX_TIE_B at
    which the element that fixes the block's scale, 448 * 2^(b-127) =
    7 * 2^(b-121), is a finite f16 value: a multiple of 2^-24 (b >= 97) not
    above 65504 (b <= 134) -- 119, 127 and 134."""
    if dtype != torch.float16:
        return MX_TIE_B
    return tuple(b for b in MX_TIE_B if 97 <= b <= 134)


def mx_tie_set(dtype: torch.dtype) -> torch.Tensor:
    """x = t * 2^(b-127) for b in mx_tie_b(dtype), t over every e4m3 value
    up to 448, every midpoint between neighbours and the nearest value of
    ``dtype`` on each side of each scaled midpoint, both signs; candidates
    the dtype does not hold exactly are dropped.  31 to a block, the 32nd
    element (its slot moving from block to block) is +-448 * 2^(b-127) and
    fixes the block's scale byte at b; candidates above it are dropped."""
    vals = np.unique(np.abs(e4m3_table()[:0x7F]))
    mids = (vals[:-1] + vals[1:]) / 2
    blocks = []
    for b in mx_tie_b(dtype):
        sc = 2.0 ** (b - 127)
        # b = 247: 448 * 2^120 is past every maximum; the largest finite
        # value of the dtype fixes the scale there (check_tie_set confirms)
        top = min(448.0 * sc, float(torch.finfo(dtype).max))
        ve, _, _ = _next_up_down(vals[1:] * sc, dtype)
        me, lo, hi = _next_up_down(mids * sc, dtype)
        cand = np.concatenate([[0.0], ve, me, lo, hi])
        cand = np.unique(cand[~np.isnan(cand) & (cand <= top)])
        cand = np.concatenate([cand, -cand])              # -0.0 included
        cand = np.concatenate([cand, np.zeros(-cand.size % 31)])
        for k, row in enumerate(cand.reshape(-1, 31)):
            slot = (7 * len(blocks)) % MX_BLOCK
            fix = top if k % 2 == 0 else -top
            blocks.append(np.concatenate([row[:slot], [fix], row[slot:]]))
    x64 = torch.from_numpy(np.concatenate(blocks))
    x = x64.to(dtype)
    assert torch.equal(x.double(), x64)                   # nothing was rounded
    return x


def check_tie_set(x: torch.Tensor, parts: dict) -> None:
    """Coverage of a tie set, from the reference's scaled values and bytes."""
    s, payload = parts["scaled"], parts["payload"]
    assert set(parts["scales"].tolist()) == set(mx_tie_b(x.dtype))
    present = set(payload.tolist())
    finite = set(range(0x7F)) | set(range(0x80, 0xFF))
    assert finite <= present, sorted(finite - present)
    table = e4m3_table()
    svals = np.unique(s)
    for c in range(0x7E):                                 # codes c, c+1 >= 0
        lo, hi = table[c], table[c + 1]
        mid = (lo + hi) / 2
        assert (svals == mid).any(), f"no tie between codes {c} and {c + 1}"
        assert ((svals > lo) & (svals < mid)).any(), f"nothing below tie {c}"
        assert ((svals > mid) & (svals < hi)).any(), f"nothing above tie {c}"
    tiny = (s == -2.0 ** -10) & np.signbit(s)
    assert tiny.any() and (payload[tiny] == 0x80).all()   # rounds to -0.0


def mx_decode_set():
    """(wire uint8 tensor, n): every payload code 0..255 under every scale
    byte 0..254 -- 8 blocks per scale byte, 255*8 blocks, 65,280 elements.
    Scale byte 255 is outside the format."""
    nblk = 255 * 8
    payload = np.tile(np.arange(256, dtype=np.uint8), 255)
    scales = np.repeat(np.arange(255, dtype=np.uint8), 8)
    assert payload.size == 32 * nblk and scales.size == nblk
    return torch.from_numpy(np.concatenate([payload, scales])), 32 * nblk


# --- the sets with their references, computed once and shared ---------------

@functools.lru_cache(maxsize=None)
def mx_encode_case(kind: str, dtype: torch.dtype):
    """(input tensor, reference wire buffer) of the "scale" or "tie" set of
    ``dtype``, its coverage checked.  Shared between tests: do not modify."""
    gen, check = {"scale": (mx_scale_set, check_scale_set),
                  "tie": (mx_tie_set, check_tie_set)}[kind]
    x = gen(dtype)
    parts = mx8_pack_parts(x.to(torch.float32))
    check(x, parts)
    wire = torch.from_numpy(np.concatenate([parts["payload"], parts["scales"]]))
    return x, wire


@functools.lru_cache(maxsize=None)
def mx_decode_case(dtype: torch.dtype):
    """(wire, n, expected bits, NaN mask) of the decode set in ``dtype``."""
    wire, n = mx_decode_set()
    w = wire.numpy()
    bits, nan = mx8_unpack_ref(w[:n], w[n:], n, dtype)
    assert nan.sum() == 2 * 255 * 8 // 8                  # 0x7f, 0xff per scale byte
    return wire, n, bits, nan


def assert_bits_equal(got: torch.Tensor, bits: np.ndarray, nan: np.ndarray,
                      what: str = "") -> None:
    """A decoded CPU tensor against expected bit patterns: NaN by position,
    everything else bit for bit (so the sign of a zero counts)."""
    dtype = got.dtype
    gb = bits_of(got)
    assert gb.shape == bits.shape and gb.dtype == bits.dtype, what
    gn = is_nan_bits(gb, dtype)
    assert (gn == nan).all(), (
        f"{what}: NaN positions differ at {np.nonzero(gn != nan)[0][:8].tolist()}")
    bad = (gb != bits) & ~nan
    if bad.any():
        idx = np.nonzero(bad)[0][:8]
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at "
            f"{idx.tolist()}: got {[hex(v) for v in gb[idx].tolist()]} "
            f"want {[hex(v) for v in bits[idx].tolist()]}")
