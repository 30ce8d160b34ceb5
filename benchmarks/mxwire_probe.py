"""Byte-rate probe for the block-scaled FP8 (mxfp8) wire kernels (run on
an MI355X).

On a 1 GiB bf16 buffer (``--dtype f16`` / ``f32``: as many bytes of that
type), times in one process, interleaved round-robin:

  * ops.mx8_pack     bf16 -> mxfp8 wire      (reads 2 B, writes 33/32 B / elem)
  * ops.mx8_unpack   mxfp8 wire -> bf16
  * ops.cast_copy    bf16 -> fp8e4m3         (the yardstick: reads 2 B, writes 1 B)
  * ops.cast_copy    fp8e4m3 -> bf16

``--compare-lib PATH`` adds the ``lz_mx8_pack`` and ``lz_mx8_unpack`` of
another build of libhipops.so (say, the parent commit's) to the same rounds,
on the same source buffers, so that two builds are compared call by call in
one process.

Each call is timed with device events; the figure reported is
(bytes read + bytes written) / median time.  Also reports the fraction of
payload bytes on which the kernel and the torch codec disagree, over a
1M-element sample.  Prints one JSON line last.

``--mode axpby`` times the fused decode-combine of a wired merge-tree edge
against the two-kernel sequence it replaces, on the same buffers, for bf16
and f32 accumulators of ``--melems`` Mi elements (default 64), alternating
the two in one process:

  * fused     ops.mx8_axpby(a, wire, dst=out)           2+33/32 B read, 2 B written (bf16)
  * sequence  ops.mx8_unpack(wire -> tmp); ops.axpby(a, tmp, dst=out)
                                                        33/32+4 B read, 4 B written (bf16)

and checks that both give the same values to one unit in the last place.
"""
import argparse
import ctypes
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import torch

import lzy_amd.ops as ops
from lzy_amd.channels.mxwire import mx8_pack_torch


def _time_alternating(cases, iters, warmup):
    """Median/min/max seconds per case, cases alternated round-robin and
    each call bracketed by device events."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(iters):
        for name, fn in cases.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3)
    return {k: sorted(v) for k, v in times.items()}


def axpby_mode(args) -> None:
    n = args.melems << 20
    alpha, beta = 0.5, 0.5
    wire = torch.empty(ops.mx8_nbytes(n), device="cuda", dtype=torch.uint8)
    src = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    ops.fill_pattern(src, seed=3, mask16=0x3FFF)  # finite positive bf16
    ops.mx8_pack(src, out=wire)
    del src
    result = {"mode": "axpby", "melems": args.melems, "iters": args.iters}
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        es = 2 if dtype == torch.bfloat16 else 4
        torch.manual_seed(5)
        a = (torch.rand(n, device="cuda") + 0.5).to(dtype)  # positive, like the wire
        out_f = torch.empty_like(a)
        out_s = torch.empty_like(a)
        tmp = torch.empty_like(a)

        def fused():
            ops.mx8_axpby(a, wire, alpha, beta, dst=out_f)

        def sequence():
            ops.mx8_unpack(wire, n, dtype, out=tmp)
            ops.axpby(a, tmp, alpha, beta, dst=out_s)

        ts = _time_alternating({"fused": fused, "sequence": sequence},
                               args.iters, args.warmup)
        nbytes = {"fused": n * es + wire.numel() + n * es,
                  "sequence": wire.numel() + n * es + 2 * n * es + n * es}
        entry = {}
        for k, t in ts.items():
            med = statistics.median(t)
            entry[k] = {
                "median_us": round(med * 1e6, 1),
                "min_us": round(t[0] * 1e6, 1),
                "max_us": round(t[-1] * 1e6, 1),
                "gb_per_s": round(nbytes[k] / med / 1e9, 1),
            }
            print(f"{name} {k:9s} median {med*1e6:9.1f} us  "
                  f"[{t[0]*1e6:.1f} .. {t[-1]*1e6:.1f}]  "
                  f"{nbytes[k]/med/1e9:7.0f} GB/s (read+written)")
        entry["sequence_over_fused"] = round(
            statistics.median(ts["sequence"]) / statistics.median(ts["fused"]), 3)
        print(f"{name} sequence/fused: {entry['sequence_over_fused']}")
        # same values: bf16 may differ where the sequence rounded the
        # decoded operand to bf16 first — report, and bound by the wire's
        # own bf16 rounding step
        d = (out_f.float() - out_s.float()).abs()
        entry["max_abs_diff"] = d.max().item()
        entry["differing_fraction"] = d.ne(0).float().mean().item()
        rel = (d / out_s.float().abs().clamp_min(1e-30)).max().item()
        entry["max_rel_diff"] = rel
        print(f"{name} fused vs sequence: max rel diff {rel:.3e}, "
              f"{entry['differing_fraction']:.3e} of elements differ")
        assert rel <= (2.0 ** -7 if es == 2 else 2.0 ** -22), rel
        result[name] = entry
        del a, out_f, out_s, tmp
    print(json.dumps(result))


_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["codec", "axpby"], default="codec")
    ap.add_argument("--melems", type=int, default=64,
                    help="axpby mode: Mi elements per buffer")
    ap.add_argument("--mib", type=int, default=1024, help="tensor buffer size")
    ap.add_argument("--dtype", choices=sorted(_DTYPES), default="bf16",
                    help="codec mode: element type of the tensor side")
    ap.add_argument("--compare-lib", default=None,
                    help="codec mode: another build of libhipops.so whose "
                         "lz_mx8_unpack is timed in the same rounds")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    assert torch.cuda.is_available(), "the probe needs a GPU"
    ops._require_native()
    if args.mode == "axpby":
        axpby_mode(args)
        return
    dtype, dname = _DTYPES[args.dtype], args.dtype
    es = torch.empty(0, dtype=dtype).element_size()
    n = (args.mib << 20) // es
    src = torch.empty(n, device="cuda", dtype=dtype)
    # every 16-bit lane <= 0x3FFF: finite and positive in all three types
    ops.fill_pattern(src, seed=3, mask16=0x3FFF)
    wire = torch.empty(ops.mx8_nbytes(n), device="cuda", dtype=torch.uint8)
    fp8 = torch.empty(n, device="cuda", dtype=torch.float8_e4m3fn)
    back = torch.empty(n, device="cuda", dtype=dtype)
    ops.mx8_pack(src, out=wire)
    ops.cast_copy(src, fp8)

    cases = {
        "mx8_pack": (lambda: ops.mx8_pack(src, out=wire), es * n + wire.numel()),
        "mx8_unpack": (lambda: ops.mx8_unpack(wire, n, dtype, out=back),
                       wire.numel() + es * n),
        f"cast_{dname}_to_e4m3": (lambda: ops.cast_copy(src, fp8), es * n + n),
        f"cast_e4m3_to_{dname}": (lambda: ops.cast_copy(fp8, back), n + es * n),
    }
    if args.compare_lib:
        other = ctypes.CDLL(args.compare_lib)
        other.lz_mx8_unpack.restype = ctypes.c_int
        other.lz_mx8_unpack.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_int64,
                                        ctypes.c_void_p]
        other.lz_mx8_pack.restype = ctypes.c_int
        other.lz_mx8_pack.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_int64,
                                      ctypes.c_void_p]
        back2 = torch.empty_like(back)
        wire2 = torch.empty_like(wire)
        code = ops._dtype_code(dtype)

        def other_pack():
            err = other.lz_mx8_pack(src.data_ptr(), code, wire2.data_ptr(), n,
                                    ops._current_stream_ptr())
            assert err == 0, err

        def other_unpack():
            err = other.lz_mx8_unpack(wire.data_ptr(), back2.data_ptr(), code, n,
                                      ops._current_stream_ptr())
            assert err == 0, err

        cases["mx8_pack@compare-lib"] = (other_pack, es * n + wire.numel())
        cases["mx8_unpack@compare-lib"] = (other_unpack, wire.numel() + es * n)
    for _ in range(args.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in cases}
    for _ in range(args.iters):
        for name, (fn, _b) in cases.items():  # alternate the four
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3)

    result = {"buffer_mib": args.mib, "dtype": dname, "iters": args.iters}
    if args.compare_lib:
        ops.mx8_unpack(wire, n, dtype, out=back)
        other_unpack()
        torch.cuda.synchronize()
        bits = torch.int32 if es == 4 else torch.int16
        result["compare_lib_differing_elements"] = int(
            (back.view(bits) != back2.view(bits)).sum().item())
        result["compare_lib_differing_wire_bytes"] = int(
            (wire != wire2).sum().item())
    for name, (_fn, nbytes) in cases.items():
        ts = sorted(times[name])
        med = statistics.median(ts)
        result[name] = {
            "median_us": round(med * 1e6, 1),
            "min_us": round(ts[0] * 1e6, 1),
            "max_us": round(ts[-1] * 1e6, 1),
            "gb_per_s": round(nbytes / med / 1e9, 1),
        }
        print(f"{name:20s} median {med*1e6:9.1f} us  "
              f"[{ts[0]*1e6:.1f} .. {ts[-1]*1e6:.1f}]  "
              f"{nbytes/med/1e9:7.0f} GB/s (read+written)")

    # kernel vs torch codec on a 1M-element sample of randn * 3 magnitudes
    m = 1 << 20
    g = torch.Generator().manual_seed(0)
    x = torch.randn(m, generator=g)
    x[: m // 3] *= 1e-4
    x[-(m // 3):] *= 3e3
    x = x.to(dtype)
    got = ops.mx8_pack(x.cuda()).cpu()
    want = mx8_pack_torch(x)
    result["payload_mismatch_fraction"] = (got[:m] != want[:m]).float().mean().item()
    result["scale_mismatches"] = int((got[m:] != want[m:]).sum().item())
    print(f"payload mismatch fraction vs torch codec: "
          f"{result['payload_mismatch_fraction']}; scale byte mismatches: "
          f"{result['scale_mismatches']}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
