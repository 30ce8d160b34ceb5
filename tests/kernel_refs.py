"""Host references for the data-plane kernels in lzy_amd/ops/hipops.hip.

Every function here is written from the operation's definition (the comments
and bodies of the kernels), with numpy / torch on the CPU only: no GPU and
no import of lzy_amd.ops.  The GPU tests compare the kernels with these and
tests/test_kernel_refs.py checks the references themselves."""
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
