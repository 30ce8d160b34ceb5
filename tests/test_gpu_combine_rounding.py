"""Every combine kernel on MI355X against the exactly rounded contract
dst = round_dst(round_f32(a*alpha + fl32(x*beta))) (kernel_refs.fma_ref):
axpby, scale_shift (plain and emitting), the four decode-combines and the six
fused forwarding ops, on inputs where rounding the exact sum once, or summing
in another order, gives other bits (the sets of kernel_refs.py, checked on
the CPU by test_kernel_refs.py).  No kernel is compared with a sibling: the
reference is the only oracle.  REQUIRES the native extension."""
import functools
import itertools

import numpy as np
import pytest
import torch

import kernel_refs as kr
from kernel_refs import BF16, F16, F32, FLOATS3
from test_gpu_mxwire_exact import _capped, _offset_view

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

PAIRS = list(itertools.product(FLOATS3, repeat=2))
PAIR_IDS = [f"{kr.DT_NAMES[s]}-{kr.DT_NAMES[d]}" for s, d in PAIRS]

# (op, codec of the second operand or None, codec of wire_out or None)
COMBINE_OPS = (
    [("axpby", None, None)]
    + [(f"{c}_axpby", c, None) for c in kr.MX_CODECS]
    + [(f"{c}_axpby_pack", c, c) for c in ("mx8", "mxi8", "mx4")]
    + [(f"{c}_axpby2_pack", None, c) for c in ("mx8", "mxi8", "mx4")]
)
OP_IDS = [o[0] for o in COMBINE_OPS]
IN_PLACE = {o[0] for o in COMBINE_OPS} - {"axpby"}      # documented: dst may be a

# (n, grid cap, element-aligned views, dst is a): the smallest that reach
# every store path -- tail only, one whole group, a group and a tail, a
# partial second block, whole groups plus a cut one over several blocks of
# threads, a second grid-stride trip, the guarded (unaligned) path, in place
SHAPES = [(7, 0, False, False), (8, 0, False, False), (9, 0, False, False),
          (33, 0, False, False), (4101, 0, False, False), (2500, 1, False, False),
          (4101, 0, True, False), (4101, 0, False, True)]
PREFIXES = (4096, 4097, 4101 - 13)


@pytest.fixture(scope="module", autouse=True)
def _native():
    import lzy_amd.ops as ops

    if torch.cuda.is_available():
        assert ops.NATIVE, "HIP ops must be built+loadable on a GPU box"
    yield


# --- cases, operands and references: computed once, shared, never modified ---

@functools.lru_cache(maxsize=None)
def _cases(kind, src):
    """((name, a, x, alpha, beta), ...) with a, x CPU tensors of ``src``."""
    if kind == "dr":
        out = []
        for mid in (F16, BF16):
            a, alpha, x, beta = kr.dr_axpby_set(mid)
            out.append((f"dr-{kr.DT_NAMES[mid]}", torch.from_numpy(a).to(src),
                        torch.from_numpy(x).to(src), alpha, beta))
        return tuple(out)
    if kind == "inexact":
        a, x = kr.inexact_set(src)
        return tuple((f"inexact{al:.2f}", a, x, al, be) for al, be in kr.INEXACT_SCALARS)
    return tuple(("sp-" + r[0],) + r[1:] for r in kr.specials_runs(src))


def _same(u, v):
    return np.array_equal(u, v, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _second(kind, src, ci, codec, n):
    """The second operand of the first n elements of a case: (what the op is
    given -- a tensor of ``src`` or a reference wire --, its values as the
    kernel sees them, float64).  A wire carries what the reference decode
    makes of the reference pack of x; the prefix of it packs to a wire that
    decodes to the same values (asserted), so a prefix run sees a prefix."""
    name, _, x, _, _ = _cases(kind, src)[ci]
    if codec is None:
        return x[:n], x[:n].double().numpy()
    N = x.numel()
    full = kr.mx_pack_ref(codec, x)
    # the decoded operand is an fp32 value: a block scale past fp32's range
    # (the maxima of the specials) makes it Inf, as the formats' decode says
    with np.errstate(over="ignore"):
        xd = kr.mx_decode_ref(codec, full, N).astype(np.float32).astype(np.float64)
    if n == N:
        return full, xd
    if kind == "dr":
        assert _same(xd, x.double().numpy()), "the wire must hold x exactly"
    wire = kr.mx_pack_ref(codec, torch.from_numpy(xd[:n].astype(np.float32)))
    assert _same(kr.mx_decode_ref(codec, wire, n), xd[:n]), (codec, name, n)   # finite sets
    return wire, xd[:n]


@functools.lru_cache(maxsize=None)
def _want(kind, src, ci, codec, dst_dtype):
    """(bits, NaN mask) of the whole case; a shape checks a prefix of it."""
    _, a, x, alpha, beta = _cases(kind, src)[ci]
    return kr.fma_ref(a, alpha, _second(kind, src, ci, codec, x.numel())[1], beta, dst_dtype)


def _call(op, a, second, alpha, beta, dst):
    import lzy_amd.ops as ops

    out = getattr(ops, op)(a, second, alpha, beta, dst=dst)
    dst_out, wire_out = out if isinstance(out, tuple) else (out, None)
    assert dst_out is dst
    return wire_out


def _check(op, codec_in, codec_out, kind, src, dst_dtype, ci, n, cap=0, view=False,
           in_place=False):
    name, a, _, alpha, beta = _cases(kind, src)[ci]
    what = f"{op} {name} n={n} cap={cap} view={view} in_place={in_place}"
    second, _ = _second(kind, src, ci, codec_in, n)
    bits, nan = _want(kind, src, ci, codec_in, dst_dtype)
    bits, nan = bits[:n], nan[:n]
    dev = _offset_view if view else torch.Tensor.cuda
    a_dev = dev(a[:n].contiguous())
    # a wire is handed over as it is made: a fresh, aligned buffer
    s_dev = second.cuda() if codec_in else dev(second.contiguous())
    dst = a_dev if in_place else dev(torch.full((n,), 7.0, dtype=dst_dtype))
    with _capped(cap):
        wire_out = _call(op, a_dev, s_dev, alpha, beta, dst)
    got = dst.cpu()
    kr.assert_bits_equal(got, bits, nan, what)
    if codec_out:
        # the encoder is handed the stored value: the reference pack of the
        # reference dst (NaN payloads do not reach the wire)
        want = kr.from_bits(np.where(nan, 0x7FC0 if bits.itemsize == 2 else 0x7FC00000,
                                     bits).astype(bits.dtype), dst_dtype)
        assert torch.equal(wire_out.cpu(), kr.mx_pack_ref(codec_out, want)), what + " wire_out"


def _run_kind(op3, pair, kind):
    op, codec_in, codec_out = op3
    src, dst_dtype = pair
    for ci, case in enumerate(_cases(kind, src)):
        if kind == "specials":
            n = case[1].numel()
            _check(op, codec_in, codec_out, kind, src, dst_dtype, ci, n)
            _check(op, codec_in, codec_out, kind, src, dst_dtype, ci, n, view=True)
            continue
        for n, cap, view, in_place in SHAPES:
            if in_place and (op not in IN_PLACE or src != dst_dtype):
                continue
            _check(op, codec_in, codec_out, kind, src, dst_dtype, ci, n, cap, view, in_place)


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("op3", COMBINE_OPS, ids=OP_IDS)
def test_double_rounding_sets(op3, pair):
    """The exact sum sits just off a midpoint of f16 (of bf16): fp32 rounds
    it onto the tie, which then goes to the even neighbour, on every path of
    every kernel.  A fused FMA-and-convert rounds about half of them the
    other way."""
    _run_kind(op3, pair, "dr")


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("op3", COMBINE_OPS, ids=OP_IDS)
def test_inexact_operands(op3, pair):
    """x*beta is rounded to fp32 before it enters the FMA, and nothing else
    is: equality with the exact reference, not a bound."""
    _run_kind(op3, pair, "inexact")


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("op3", COMBINE_OPS, ids=OP_IDS)
def test_specials(op3, pair):
    """Inf, NaN, signed zeros, subnormal operands and results, the f16
    overflow boundary, fp32 overflow of the sum, 0 * Inf."""
    _run_kind(op3, pair, "specials")


@requires_gpu
@pytest.mark.parametrize("src", FLOATS3, ids=[kr.DT_NAMES[d] for d in FLOATS3])
@pytest.mark.parametrize("op3", COMBINE_OPS, ids=OP_IDS)
def test_prefix_invariance(op3, src):
    """A run on the first m elements gives the first m of the full run, bit
    for bit: how a stream is cut into chunks cannot change a value.  Stated
    on the kernels' own outputs (and each of them equals the reference)."""
    op, codec_in, codec_out = op3
    _, a, _, alpha, beta = _cases("dr", src)[0]          # the f16 midpoints

    def run(m):
        second, _ = _second("dr", src, 0, codec_in, m)
        dst = torch.full((m,), 7.0, dtype=F16, device="cuda")
        _call(op, a[:m].cuda(), second.cuda(), alpha, beta, dst)
        return dst.cpu()

    full = run(4101)
    kr.assert_bits_equal(full, *[v[:4101] for v in _want("dr", src, 0, codec_in, F16)], op)
    for m in PREFIXES:
        assert torch.equal(run(m).view(torch.int16), full[:m].view(torch.int16)), (op, m)


# --- scale_shift: dst = x*a + b, the scalar b in the place of fl32(x*beta) ---

EMIT_N = 40000            # the emitting kernel takes outputs of 64 KiB and more


@functools.lru_cache(maxsize=None)
def _ss_cases(kind, src):
    """((name, x, a, b), ...) with x a CPU tensor of ``src``."""
    if kind == "dr":
        return tuple((f"dr-{kr.DT_NAMES[mid]}-{i}", torch.from_numpy(x).to(src), a, b)
                     for mid in (F16, BF16)
                     for i, (x, a, b) in enumerate(kr.dr_scale_shift_sets(mid, src)))
    if kind == "inexact":
        x = kr.inexact_set(src)[0]
        return tuple((f"inexact{a:.2f}", x, a, b) for a, b in kr.INEXACT_SCALARS)
    inf = float("inf")
    runs = {r[0]: r for r in kr.specials_runs(src)}
    v, ints, ones = runs["cross"][1][::11], runs["f16sub"][1][::9], runs["edge"][1][::9]
    big = float(torch.finfo(src).max)
    k = 128 - int(np.frexp(big)[1])
    return (
        ("sp-id", v, 1.0, 0.0), ("sp-zero", v, 0.0, -0.0), ("sp-neg", v, -1.0, -0.0),
        ("sp-ainf", v, inf, 1.0), ("sp-binf", v, 1.0, -inf), ("sp-bnan", v, 1.0, float("nan")),
        ("sp-f16sub", ints, 2.0 ** -24, 2.0 ** -25), ("sp-bf16sub", ints, 2.0 ** -133, 2.0 ** -134),
        ("sp-edge", ones, 65504.0, 16.0), ("sp-edge-below", ones, 65504.0, 15.99),
        ("sp-edge-neg", ones, 65504.0, -16.0),
        ("sp-ovf", v, 2.0 ** k, 2.0 ** 127), ("sp-ovf-neg", v, 2.0 ** k, -(2.0 ** 127)),
    )


@functools.lru_cache(maxsize=None)
def _ss_want(kind, src, ci, dst_dtype):
    _, x, a, b = _ss_cases(kind, src)[ci]
    return kr.fma_ref(x, a, np.full(x.numel(), np.float64(np.float32(b))), 1.0, dst_dtype)


def _ss_check(kind, src, dst_dtype, ci, n, cap=0, view=False, in_place=False):
    from lzy_amd.ops import scale_shift

    name, x, a, b = _ss_cases(kind, src)[ci]
    what = f"scale_shift {name} n={n} cap={cap} view={view} in_place={in_place}"
    bits, nan = _ss_want(kind, src, ci, dst_dtype)
    dev = _offset_view if view else torch.Tensor.cuda
    x_dev = dev(x[:n].contiguous())
    dst = x_dev if in_place else dev(torch.full((n,), 7.0, dtype=dst_dtype))
    with _capped(cap):
        assert scale_shift(x_dev, a, b, dst=dst) is dst
    kr.assert_bits_equal(dst.cpu(), bits[:n], nan[:n], what)


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("kind", ["dr", "inexact", "specials"])
def test_scale_shift(kind, pair):
    src, dst_dtype = pair
    for ci, case in enumerate(_ss_cases(kind, src)):
        if kind == "specials":
            _ss_check(kind, src, dst_dtype, ci, case[1].numel())
            _ss_check(kind, src, dst_dtype, ci, case[1].numel(), view=True)
            continue
        for n, cap, view, in_place in SHAPES:
            if in_place and src != dst_dtype:
                continue
            _ss_check(kind, src, dst_dtype, ci, n, cap, view, in_place)


@requires_gpu
@pytest.mark.parametrize("dtype", FLOATS3, ids=[kr.DT_NAMES[d] for d in FLOATS3])
@pytest.mark.parametrize("kind", ["dr", "inexact", "specials"])
def test_scale_shift_emitting_path(kind, dtype):
    """A new output of 64 KiB or more comes from scale_shift_emit_kernel
    (same-width pairs; with dst=None the same dtype): each set tiled to
    40000 elements, the whole-tile loop and the scalar tail of thread 0."""
    import lzy_amd.ops as ops

    for ci, (name, x, a, b) in enumerate(_ss_cases(kind, dtype)):
        reps = -(-EMIT_N // x.numel())
        bits, nan = _ss_want(kind, dtype, ci, dtype)
        got = ops.scale_shift(x.repeat(reps)[:EMIT_N].cuda(), a, b)
        assert ops._EMIT_ATTR in got.__dict__, "the emitting kernel must have run"
        kr.assert_bits_equal(got.cpu(), np.tile(bits, reps)[:EMIT_N],
                             np.tile(nan, reps)[:EMIT_N], f"emit {name}")


@requires_gpu
@pytest.mark.parametrize("src", FLOATS3, ids=[kr.DT_NAMES[d] for d in FLOATS3])
def test_scale_shift_prefix_invariance(src):
    from lzy_amd.ops import scale_shift

    _, x, a, b = _ss_cases("dr", src)[0]

    def run(m):
        dst = torch.full((m,), 7.0, dtype=F16, device="cuda")
        return scale_shift(x[:m].cuda(), a, b, dst=dst).cpu()

    full = run(4101)
    for m in PREFIXES:
        assert torch.equal(run(m).view(torch.int16), full[:m].view(torch.int16)), m
