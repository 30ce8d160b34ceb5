"""scale_shift that emits its output's mfma digest and |x| moments in the same
pass (lz_scale_shift_emit), and the record the public ops keep of them.

Kernel cases run under lz_set_max_blocks(k), k in {1, 2, 3}, so buffers of a
few KiB reach every loop of the kernel: with W = 4k waves the sizes (bytes of
dst) are below one tile (2, 16, 1022), one tile, one full unrolled trip
(1 KiB * 4W), an unrolled trip + the remainder loop + an uneven last round
(1 KiB * (4W + W + 1)), and each of these plus a 6-byte and a 1018-byte
tail.  An f32 buffer cannot have a size that is not a multiple of 4, so there
each size is rounded down to one (2 -> dropped, 6 -> 4, 1018 -> 1016, ...).

Per case:
  * dst bit for bit what lz_scale_shift writes from the same input;
  * the digest equal to device_checksum(dst, "mfma") and to the host
    reference under the same cap;
  * moments on integer-valued data (every output an integer, |y| <= 63)
    EXACTLY the integer sums;
  * moments on randn within (m + 2) * 2^-24 * sum|y| (resp. sum y^2) of the
    float64 sums of the stored values, m = the most elements any one f32
    accumulator takes at that size and grid (computed here from the work
    decomposition): m - 1 roundings of recursive summation (m with the fma
    of the squares), unit roundoff 2^-24 each, the f64 folds exact at these
    sizes.
"""
import ctypes
import os
import subprocess
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

from kernel_refs import (
    assert_bits_equal,
    bits_of,
    checksum_mfma_ref,
    checksum_valu_ref,
    is_nan_bits,
    mfma_grid_blocks,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
PAIRS = [(BF16, BF16), (F16, F16), (F32, F32), (BF16, F16), (F16, BF16)]
CAPS = [1, 2, 3]
# the flagship's augment constants: the product is inexact, so the single
# rounding of the FMA shows
A, B = 1.0009765625, 0.125


def _pair_id(p):
    return "-".join(NAMES[d] for d in p)


@pytest.fixture(scope="module", autouse=True)
def _native():
    import lzy_amd.ops as ops

    if torch.cuda.is_available():
        assert ops.NATIVE, "HIP ops must be built+loadable on a GPU box"
        assert ops._EMIT, "libhipops.so lacks lz_scale_shift_emit"
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


def _sizes(k, itemsize):
    w = 4 * k
    base = [2, 16, 1022, 1024, 1024 * w * 4, 1024 * (w * 4 + w + 1)]
    out = []
    for s in base:
        for tail in (0, 6, 1018):
            nb = (s + tail) // itemsize * itemsize
            if nb and nb not in out:
                out.append(nb)
    return out


def _max_per_accumulator(nbytes, k, itemsize):
    """Most elements one f32 accumulator of the kernel takes: wave w owns
    tiles w, w + S, ...; four at a time go to accumulators 0..3, the rest
    (< 4) to accumulator 0; a lane has 16 bytes of each tile; thread 0 of
    wave 0 adds the sub-tile tail to its accumulator 0."""
    per_lane = 16 // itemsize
    ntiles = nbytes >> 10
    nwaves = 4 * mfma_grid_blocks(nbytes, k)
    tail = (nbytes - (ntiles << 10)) // itemsize
    m = 0
    for w in range(nwaves):
        cnt = len(range(w, ntiles, nwaves))
        acc0 = per_lane * (cnt // 4 + cnt % 4) + (tail if w == 0 else 0)
        m = max(m, acc0)
    return m


def _emit_raw(src, dst_dtype, a, b):
    """The export itself: (dst, digest, moments as two python floats)."""
    import lzy_amd.ops as ops

    lib = ops._require_native()
    dst = torch.empty(src.numel(), dtype=dst_dtype, device=src.device)
    buf = torch.full((3,), -1, dtype=torch.int64, device=src.device)
    err = lib.lz_scale_shift_emit(
        ctypes.c_void_p(src.data_ptr()), ops._dtype_code(src.dtype),
        ctypes.c_void_p(dst.data_ptr()), ops._dtype_code(dst_dtype),
        src.numel(), ctypes.c_float(a), ctypes.c_float(b),
        ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 8),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
    )
    assert err == 0, err
    host = buf.cpu()
    mom = host[1:3].view(torch.float64)
    return dst, int(host[0]) & 0xFFFFFFFFFFFFFFFF, float(mom[0]), float(mom[1])


def _plain(src, dst_dtype, a, b):
    import lzy_amd.ops as ops

    ref = torch.empty(src.numel(), dtype=dst_dtype, device=src.device)
    ops.scale_shift(src, a, b, dst=ref)
    return ref


def _check_dst_and_digest(src, dst_dtype, a, b, k, what):
    import lzy_amd.ops as ops

    dst, digest, s_abs, s_sq = _emit_raw(src, dst_dtype, a, b)
    ref = _plain(src, dst_dtype, a, b).cpu()
    got = dst.cpu()
    rb = bits_of(ref)
    assert_bits_equal(got, rb, is_nan_bits(rb, dst_dtype), what)
    assert digest == ops.device_checksum(dst, method="mfma"), what
    raw = got.view(torch.uint8).numpy().tobytes()
    assert digest == checksum_mfma_ref(raw, max_blocks=k), what
    return got, s_abs, s_sq


@requires_gpu
@pytest.mark.parametrize("k", CAPS)
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_emit_kernel_matches_plain_kernels(pair, k):
    sd, dd = pair
    itemsize = torch.empty(0, dtype=dd).element_size()
    g = torch.Generator().manual_seed(1000 * k + PAIRS.index(pair))
    with _capped(k):
        for nbytes in _sizes(k, itemsize):
            n = nbytes // itemsize
            what = f"{_pair_id(pair)} cap={k} nbytes={nbytes}"
            m = _max_per_accumulator(nbytes, k, itemsize)

            # integer-valued: y = 2x + 1, x in [-31, 31] -> |y| <= 63
            xi = torch.randint(-31, 32, (n,), generator=g).to(sd).cuda()
            got, s_abs, s_sq = _check_dst_and_digest(xi, dd, 2.0, 1.0, k, what)
            yi = got.double().numpy().astype(np.int64)
            assert np.array_equal(yi, 2 * xi.cpu().double().numpy().astype(np.int64) + 1), what
            assert s_abs == float(np.abs(yi).sum()), what
            assert s_sq == float((yi * yi).sum()), what

            xr = torch.randn(n, generator=g).to(sd).cuda()
            got, s_abs, s_sq = _check_dst_and_digest(xr, dd, A, B, k, what)
            y = got.double().numpy()
            ref_abs, ref_sq = float(np.abs(y).sum()), float((y * y).sum())
            bound = (m + 2) * 2.0 ** -24
            err_abs, err_sq = abs(s_abs - ref_abs), abs(s_sq - ref_sq)
            print(f"{what}: m={m} err|y|={err_abs:.3e} (<= {bound * ref_abs:.3e}) "
                  f"err y^2={err_sq:.3e} (<= {bound * ref_sq:.3e})")
            assert err_abs <= bound * ref_abs, what
            assert err_sq <= bound * ref_sq, what


@requires_gpu
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_emit_kernel_special_values(pair):
    """Infinities, NaN, signed zeros, subnormals and the format's extremes
    take the same FMA and the same rounding as in the plain kernel, in the
    vector body and in the scalar tail."""
    sd, dd = pair
    fi = torch.finfo(sd)
    specials = torch.tensor(
        [float("inf"), float("-inf"), float("nan"), 0.0, -0.0, fi.tiny,
         -fi.tiny, fi.tiny / 4, fi.max, -fi.max, fi.eps, 1.0, -1.0, 65504.0,
         -0.125 / A, 3.0e38], dtype=torch.float64)
    itemsize = torch.empty(0, dtype=dd).element_size()
    n = (2 * 1024 + 1018 // itemsize * itemsize) // itemsize
    x = specials.repeat(n // specials.numel() + 1)[:n].to(sd).cuda()
    with _capped(1):
        _check_dst_and_digest(x, dd, A, B, 1, f"specials {_pair_id(pair)}")


@requires_gpu
def test_emit_export_rejects_what_it_does_not_take():
    import lzy_amd.ops as ops

    lib = ops._require_native()
    invalid = 1  # hipErrorInvalidValue

    def call(src, dst, buf, moments_off=8, n=None):
        return lib.lz_scale_shift_emit(
            ctypes.c_void_p(src.data_ptr()), ops._dtype_code(src.dtype),
            ctypes.c_void_p(dst.data_ptr()), ops._dtype_code(dst.dtype),
            dst.numel() if n is None else n, ctypes.c_float(1.0), ctypes.c_float(0.0),
            ctypes.c_void_p(buf.data_ptr()),
            ctypes.c_void_p(buf.data_ptr() + moments_off),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
        )

    buf = torch.zeros(4, dtype=torch.int64, device="cuda")
    x32 = torch.zeros(64, dtype=F32, device="cuda")
    x16 = torch.zeros(64, dtype=BF16, device="cuda")
    assert call(x32, torch.empty_like(x16), buf) == invalid          # widths differ
    assert call(x16, torch.empty_like(x32), buf) == invalid
    u8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert call(u8, torch.empty_like(u8), buf) == invalid            # not a float pair
    assert call(x16[1:], torch.empty(63, dtype=BF16, device="cuda"), buf) == invalid
    assert call(x16[:63], torch.empty(64, dtype=BF16, device="cuda")[1:], buf) == invalid
    assert call(x16, torch.empty_like(x16), buf, moments_off=16) == invalid
    torch.cuda.synchronize()
    assert call(x16, torch.empty_like(x16), buf) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# the record on the public ops
# ---------------------------------------------------------------------------

N_REC = 40000  # bf16: 80000 bytes >= 64 KiB, 78 tiles + a 128-byte tail


def _fresh(dtype=BF16, seed=5):
    import lzy_amd.ops as ops

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N_REC, generator=g).to(dtype).cuda()
    return x, ops.scale_shift(x, A, B)


def _hits():
    import lzy_amd.ops as ops

    return ops._emit_hits


def _kernel_values(t):
    """What the plain kernels give for t's contents (a clone has no record)."""
    import lzy_amd.ops as ops

    c = t.detach().clone()
    assert not hasattr(c, ops._EMIT_ATTR)
    h0 = _hits()
    out = (ops.device_checksum(c), ops.stats(c, use_abs=True).cpu())
    assert _hits() == h0
    return out


@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=lambda d: NAMES[d])
def test_record_used_when_valid(dtype):
    import lzy_amd.ops as ops

    x, t = _fresh(dtype)
    assert hasattr(t, ops._EMIT_ATTR)
    ref = _plain(x, dtype, A, B)
    assert torch.equal(t.view(torch.uint8), ref.view(torch.uint8))
    want_sum, want_stats = _kernel_values(t)
    raw = t.cpu().view(torch.uint8).numpy().tobytes()
    assert want_sum == checksum_mfma_ref(raw)

    h0 = _hits()
    assert ops.device_checksum(t) == want_sum
    assert ops.device_checksum(t, method="mfma") == want_sum
    assert _hits() == h0 + 2
    st = ops.stats(t, use_abs=True)
    assert st.dtype == torch.float64 and st.shape == (2,) and st.is_cuda
    assert st.data_ptr() != getattr(t, ops._EMIT_ATTR).buf.data_ptr() + 8  # a copy
    am = ops.abs_mean(t)
    assert _hits() == h0 + 4
    # two summation orders of the same values: each within its own bound of
    # the exact sum; 1e-6 relative is far above both at 40000 elements
    y = t.cpu().double()
    exact = torch.stack([y.abs().sum(), (y * y).sum()])
    assert torch.allclose(st.cpu(), exact, rtol=1e-6, atol=0)
    assert torch.allclose(want_stats, exact, rtol=1e-6, atol=0)
    assert abs(am - float(exact[0]) / N_REC) <= 1e-6 * float(exact[0]) / N_REC
    # plain stats (no abs) is not what the record holds
    h1 = _hits()
    ops.stats(t, use_abs=False)
    assert _hits() == h1


def _assert_ignored_and_right(t):
    import lzy_amd.ops as ops

    want_sum, want_stats = _kernel_values(t)
    h0 = _hits()
    assert ops.device_checksum(t) == want_sum
    # the same kernel on the same values: only the order of its per-wave f64
    # atomics differs from run to run (a few units of 2^-53)
    assert torch.allclose(ops.stats(t, use_abs=True).cpu(), want_stats,
                          rtol=1e-12, atol=0)
    assert _hits() == h0


@requires_gpu
def test_record_ignored_after_torch_inplace():
    _, t = _fresh()
    t.add_(1)
    _assert_ignored_and_right(t)


@requires_gpu
def test_record_ignored_after_scale_shift_into_it():
    import lzy_amd.ops as ops

    x, t = _fresh()
    assert ops.scale_shift(x, 2.0, 1.0, dst=t) is t
    _assert_ignored_and_right(t)


@requires_gpu
def test_record_ignored_after_pointer_write_through_a_view():
    """forget() of a view reaches the record of its base: they share the
    version counter."""
    import lzy_amd.ops as ops

    x, t = _fresh()
    ops.scale_shift(x[:1024], 2.0, 1.0, dst=t[1024:2048])
    _assert_ignored_and_right(t)


@requires_gpu
def test_record_ignored_after_fill_pattern():
    import lzy_amd.ops as ops

    _, t = _fresh()
    ops.fill_pattern(t, seed=3, mask16=0x3FFF)
    _assert_ignored_and_right(t)


@requires_gpu
def test_record_ignored_after_forget():
    import lzy_amd.ops as ops

    _, t = _fresh()
    ops.forget(t)
    assert not hasattr(t, ops._EMIT_ATTR)
    _assert_ignored_and_right(t)


@requires_gpu
def test_views_and_detach_have_no_record():
    import lzy_amd.ops as ops

    # f32, so that t[1:] stays 4-byte aligned: the checksum kernels read
    # dwords, and a 2-byte-aligned bf16 view is not theirs to hash
    _, t = _fresh(F32)
    for alias in (t[1:], t.detach(), t.view(-1, 8)):
        assert not hasattr(alias, ops._EMIT_ATTR)
        _assert_ignored_and_right(alias)
    # and looking at aliases did not cost t its own
    h0 = _hits()
    ops.device_checksum(t)
    assert _hits() == h0 + 1


@requires_gpu
def test_record_ignored_after_cap_change():
    import lzy_amd.ops as ops

    _, t = _fresh()
    raw = t.cpu().view(torch.uint8).numpy().tobytes()
    assert mfma_grid_blocks(len(raw), 3) != mfma_grid_blocks(len(raw))
    with _capped(3):
        h0 = _hits()
        assert ops.device_checksum(t, method="mfma") == checksum_mfma_ref(raw, max_blocks=3)
        assert _hits() == h0
    # the recorded grid is the current one again
    h0 = _hits()
    assert ops.device_checksum(t) == checksum_mfma_ref(raw)
    assert _hits() == h0 + 1


@requires_gpu
def test_valu_method_never_uses_the_record():
    import lzy_amd.ops as ops

    _, t = _fresh()
    raw = t.cpu().view(torch.uint8).numpy().tobytes()
    h0 = _hits()
    assert ops.device_checksum(t, method="valu") == checksum_valu_ref(raw)
    assert _hits() == h0


@requires_gpu
def test_switch_off(monkeypatch):
    import lzy_amd.ops as ops

    _, t = _fresh()
    monkeypatch.setenv("LZY_HIP_EMIT", "0")
    _assert_ignored_and_right(t)            # an existing record is not used
    x, u = _fresh(seed=6)
    assert not hasattr(u, ops._EMIT_ATTR)   # and none is made
    assert torch.equal(u, _plain(x, BF16, A, B))
    monkeypatch.delenv("LZY_HIP_EMIT")
    h0 = _hits()
    ops.device_checksum(t)
    assert _hits() == h0 + 1


@requires_gpu
def test_small_or_mixed_width_outputs_get_no_record():
    import lzy_amd.ops as ops

    x = torch.randn(1000).to(BF16).cuda()           # 2000 bytes < 64 KiB
    assert not hasattr(ops.scale_shift(x, A, B), ops._EMIT_ATTR)
    big = torch.randn(N_REC).cuda()
    out = torch.empty(N_REC, dtype=BF16, device="cuda")
    assert not hasattr(ops.scale_shift(big, A, B, dst=out), ops._EMIT_ATTR)


@requires_gpu
def test_pool_augment_then_checksum_and_evaluate(tmp_path):
    """The flagship's augment -> {checksum, evaluate} under GpuPoolRuntime at
    N=1, recording on and off in one process, with the stream-race checker
    on: same digest, same score, and the record is hit only when on."""
    root = Path(__file__).resolve().parent.parent
    env = {
        **os.environ,
        "LZY_AMD_STORAGE": str(tmp_path / "s"),
        "PYTHONPATH": str(root),
        "LZY_BENCH_SHARD_MB": "2",
        "LZY_STREAM_CHECK": "1",
    }
    env.pop("LZY_HIP_EMIT", None)
    res = subprocess.run(
        [sys.executable, "tests/pool_script_emit.py"],
        cwd=root, env=env, capture_output=True, text=True, timeout=300,
    )
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "EMIT-POOL-OK" in res.stdout
