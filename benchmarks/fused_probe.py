"""Probe target for rocprofv3 PMC capture of the fused data-plane kernels.

Usage: python benchmarks/fused_probe.py [stats|abs_mean|normalize|scale_shift|axpby] [iters]
Runs the selected fused kernel on 512 MiB bf16 device buffers and prints
un-profiled effective bandwidth.

       python benchmarks/fused_probe.py scale_shift_emit
The emitting scale_shift against what it replaces, on the same 1 GiB bf16
buffers: plain scale_shift, then checksum_mfma + stats(abs) of its output,
then the one emitting kernel, every round in that order (so the two sides
alternate in one process), device events around each part, 5 warm-up and 30
timed rounds, median [min .. max] per part.
"""
import ctypes
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import torch

import lzy_amd.ops as ops


def emit_probe(warmup: int = 5, rounds: int = 30) -> None:
    lib = ops._require_native()
    assert ops._EMIT, "libhipops.so lacks lz_scale_shift_emit"
    n = 512 << 20  # 1 GiB of bf16: the flagship's shard
    src = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    src.normal_()
    out = torch.empty_like(src)
    buf = torch.zeros(3, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.float64, device="cuda")
    bf16 = ops._dtype_code(torch.bfloat16)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    a, b = ctypes.c_float(1.0009765625), ctypes.c_float(0.125)

    def plain(stream):
        ops._check(lib.lz_scale_shift(p(src), bf16, p(out), bf16, n, a, b, stream))

    def readers(stream):
        ops._check(lib.lz_checksum_mfma(p(out), 2 * n, p(buf), stream))
        ops._check(lib.lz_stats(p(out), bf16, n, 1, p(st), stream))

    def emit(stream):
        ops._check(lib.lz_scale_shift_emit(p(src), bf16, p(out), bf16, n, a, b,
                                           p(buf), p(buf, 8), stream))

    parts = {"scale_shift": [], "checksum_mfma+stats": [], "scale_shift_emit": []}
    for r in range(warmup + rounds):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        plain(stream)
        ev[1].record()
        readers(stream)
        ev[2].record()
        emit(stream)
        ev[3].record()
        torch.cuda.synchronize()
        if r >= warmup:
            for k, name in enumerate(parts):
                parts[name].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
    three = [x + y for x, y in zip(parts["scale_shift"], parts["checksum_mfma+stats"])]

    def line(name, xs, moved_gib):
        med = statistics.median(xs)
        print(f"{name:34s} {med:7.1f} us [{min(xs):7.1f} .. {max(xs):7.1f}]  "
              f"{moved_gib * (1 << 30) / med / 1e6:5.2f} TB/s over {moved_gib} GiB")

    print(f"scale_shift_emit probe: 1 GiB bf16, {rounds} rounds after {warmup} warm-up")
    line("scale_shift", parts["scale_shift"], 2)
    line("checksum_mfma + stats(abs)", parts["checksum_mfma+stats"], 2)
    line("three-kernel sequence", three, 4)
    line("scale_shift_emit", parts["scale_shift_emit"], 2)


def main() -> None:
    which = sys.argv[1] if len(sys.argv) > 1 else "normalize"
    if which == "scale_shift_emit":
        emit_probe()
        return
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    n = 256 << 20
    t = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    t.normal_()
    nbytes = n * 2
    out = torch.empty_like(t)

    if which == "stats":
        fn = lambda: ops.stats(t)  # noqa: E731
        moved = nbytes
    elif which == "abs_mean":
        fn = lambda: ops.abs_mean(t)  # noqa: E731
        moved = nbytes
    elif which == "normalize":
        fn = lambda: ops.normalize(t, dst=out)  # noqa: E731
        moved = 3 * nbytes
    elif which == "scale_shift":
        fn = lambda: ops.scale_shift(t, 1.001, 0.125, dst=out)  # noqa: E731
        moved = 2 * nbytes
    elif which == "axpby":
        b = torch.empty_like(t)
        b.normal_()
        fn = lambda: ops.axpby(t, b, 0.5, 0.5, dst=out)  # noqa: E731
        moved = 3 * nbytes
    else:
        raise SystemExit(f"unknown probe {which}")

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"{which}: {moved / dt / 1e9:.0f} GB/s effective ({iters}x)")


if __name__ == "__main__":
    main()
