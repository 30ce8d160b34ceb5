"""Byte-rate probe for the block-scaled wire kernels (run on an MI355X).
``--codec mxint8`` times the ``mxi8_*`` kernels in place of the ``mx8_*``
ones named below; ``--compare-lib`` always adds the other build's
``lz_mx8_*``, which move the same bytes.  ``--codec mxfp4`` times
``mx4_pack``, ``mx4_unpack`` and ``mx4_axpby`` (17/32 B per element on the
wire side) and, in the same rounds, this build's ``mx8_*`` three.
``--codec mxfp6`` does the same for ``mx6_pack``, ``mx6_unpack`` and
``mx6_axpby`` (25/32 B per element on the wire side), with the ``mx8_*`` and
the ``mx4_*`` three in its rounds.

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

``--mode forward`` times the step of a merge-tree node that forwards, for
every codec (``--forward-codec`` picks one), bf16 and f32, at a plan's chunk
size and on a 1 GiB operand:

  * pair   ops.mx8_axpby(a, wire_in, dst=out); ops.mx8_pack(out, out=wire_out)
                                                        4+33/32 B read, 2+33/32 B written (bf16)
  * fused  ops.mx8_axpby_pack(a, wire_in, dst=out, wire_out=wire_out)
                                                        2+33/32 B read, 2+33/32 B written (bf16)

and checks that both leave the same bytes in ``out`` and ``wire_out``.  For
``mxfp4`` and ``mxfp6`` (17/32 and 25/32 B per element on each wire side) it
also times the node whose two inputs are local: ``ops.axpby`` then
``ops.mx4_pack`` against ``ops.mx4_axpby2_pack`` (the ``_plain`` keys).
"""
import argparse
import ctypes
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import torch

import lzy_amd.ops as ops
from lzy_amd.channels import mxwire


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
    wire = torch.empty(_nbytes(args.codec, n), device="cuda", dtype=torch.uint8)
    src = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    ops.fill_pattern(src, seed=3, mask16=0x3FFF)  # finite positive bf16
    pre = _PREFIX[args.codec]
    pack, unpack, axpby = (getattr(ops, f"{pre}_{k}") for k in ("pack", "unpack", "axpby"))
    pack(src, out=wire)
    del src
    result = {"mode": "axpby", "codec": args.codec, "melems": args.melems,
              "iters": args.iters}
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        es = 2 if dtype == torch.bfloat16 else 4
        torch.manual_seed(5)
        a = (torch.rand(n, device="cuda") + 0.5).to(dtype)  # positive, like the wire
        out_f = torch.empty_like(a)
        out_s = torch.empty_like(a)
        tmp = torch.empty_like(a)

        def fused():
            axpby(a, wire, alpha, beta, dst=out_f)

        def sequence():
            unpack(wire, n, dtype, out=tmp)
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


def forward_mode(args) -> None:
    """The step of a forwarding merge-tree node, per codec and accumulator
    dtype, at the chunk a 64 MiB bf16 wired plan is cut into (8 Mi elements
    at the default stream_chunk_mb) and on a 1 GiB operand."""
    alpha, beta = 0.5, 0.5
    result = {"mode": "forward", "iters": args.iters}
    codecs = _FORWARD if args.forward_codec == "all" else (args.forward_codec,)
    for codec in codecs:
        pre = _PREFIX[codec]
        pack, axpby, axpby_pack, axpby2_pack = (
            getattr(ops, f"{pre}_{k}") for k in ("pack", "axpby", "axpby_pack", "axpby2_pack"))
        # the second operand: a received wire chunk, or (mxfp4 and mxfp6, the
        # node whose two inputs are local) a plain tensor
        for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            es = 2 if dtype == torch.bfloat16 else 4
            for label, n in (("chunk", 8 << 20), ("1GiB", (1 << 30) // es)):
                for plain in ((False, True) if codec in ("mxfp4", "mxfp6") else (False,)):
                    torch.manual_seed(5)
                    a = (torch.rand(n, device="cuda") + 0.5).to(dtype)
                    b = (torch.rand(n, device="cuda") + 0.5).to(dtype)
                    second = b if plain else pack(b)
                    w = _nbytes(codec, n)
                    out_p, out_f = torch.empty_like(a), torch.empty_like(a)
                    wire_p, wire_f = (torch.empty(w, device="cuda", dtype=torch.uint8)
                                      for _ in range(2))
                    combine, fused_op = (ops.axpby, axpby2_pack) if plain \
                        else (axpby, axpby_pack)

                    def pair():
                        combine(a, second, alpha, beta, dst=out_p)
                        pack(out_p, out=wire_p)

                    def fused():
                        fused_op(a, second, alpha, beta, dst=out_f, wire_out=wire_f)

                    iters = args.iters * (8 if label == "chunk" else 1)
                    ts = _time_alternating({"pair": pair, "fused": fused}, iters,
                                           args.warmup)
                    rd = n * es + (n * es if plain else w)  # the fused op's reads
                    nbytes = {"pair": rd + 2 * n * es + w, "fused": rd + n * es + w}
                    key = f"{codec}_{name}_{label}" + ("_plain" if plain else "")
                    entry = {"elems": n}
                    for k, t in ts.items():
                        med = statistics.median(t)
                        entry[k] = {"median_us": round(med * 1e6, 1),
                                    "min_us": round(t[0] * 1e6, 1),
                                    "max_us": round(t[-1] * 1e6, 1),
                                    "gb_per_s": round(nbytes[k] / med / 1e9, 1)}
                        print(f"{key:24s} {k:5s} median {med*1e6:9.1f} us  "
                              f"[{t[0]*1e6:.1f} .. {t[-1]*1e6:.1f}]  "
                              f"{nbytes[k]/med/1e9:7.0f} GB/s (read+written)", flush=True)
                    entry["pair_over_fused"] = round(
                        statistics.median(ts["pair"]) / statistics.median(ts["fused"]), 3)
                    # the plan relies on identity, not closeness
                    bits = torch.int16 if es == 2 else torch.int32
                    assert torch.equal(out_p.view(bits), out_f.view(bits))
                    assert torch.equal(wire_p, wire_f)
                    result[key] = entry
                    del a, b, second, out_p, out_f, wire_p, wire_f
    print(json.dumps(result))


_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
_PREFIX = {"mxfp8": "mx8", "mxint8": "mxi8", "mxfp4": "mx4", "mxfp6": "mx6"}
# the codecs with a fused forwarding kernel
_FORWARD = ("mxfp8", "mxint8", "mxfp4", "mxfp6")


def _nbytes(codec: str, n: int) -> int:
    if codec == "mxfp6":
        return ops.mx6_nbytes(n)
    return ops.mx4_nbytes(n) if codec == "mxfp4" else ops.mx8_nbytes(n)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["codec", "axpby", "forward"], default="codec")
    ap.add_argument("--codec", choices=sorted(_PREFIX), default="mxfp8")
    ap.add_argument("--forward-codec", choices=sorted(_FORWARD) + ["all"], default="all",
                    help="forward mode: the codec to time")
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
    if args.mode == "forward":
        forward_mode(args)
        return
    dtype, dname = _DTYPES[args.dtype], args.dtype
    es = torch.empty(0, dtype=dtype).element_size()
    n = (args.mib << 20) // es
    src = torch.empty(n, device="cuda", dtype=dtype)
    # every 16-bit lane <= 0x3FFF: finite and positive in all three types
    ops.fill_pattern(src, seed=3, mask16=0x3FFF)
    wire = torch.empty(_nbytes(args.codec, n), device="cuda", dtype=torch.uint8)
    fp8 = torch.empty(n, device="cuda", dtype=torch.float8_e4m3fn)
    back = torch.empty(n, device="cuda", dtype=dtype)
    pre = _PREFIX[args.codec]
    pack, unpack = getattr(ops, f"{pre}_pack"), getattr(ops, f"{pre}_unpack")
    pack(src, out=wire)
    ops.cast_copy(src, fp8)

    cases = {
        f"{pre}_pack": (lambda: pack(src, out=wire), es * n + wire.numel()),
        f"{pre}_unpack": (lambda: unpack(wire, n, dtype, out=back),
                          wire.numel() + es * n),
        f"cast_{dname}_to_e4m3": (lambda: ops.cast_copy(src, fp8), es * n + n),
        f"cast_e4m3_to_{dname}": (lambda: ops.cast_copy(fp8, back), n + es * n),
    }
    if args.codec in ("mxfp4", "mxfp6"):
        # the 8-bit kernels (mxfp6: the 4-bit ones too) and every
        # decode-combine, in the same rounds
        acc = torch.empty_like(src)
        axpby = getattr(ops, f"{pre}_axpby")
        cases[f"{pre}_axpby"] = (lambda: axpby(src, wire, 0.5, 0.5, dst=acc),
                                 2 * es * n + wire.numel())

        def add_codec(o, wire_o):
            o_pack, o_unpack, o_axpby = (getattr(ops, f"{o}_{k}")
                                         for k in ("pack", "unpack", "axpby"))
            cases.update({
                f"{o}_pack": (lambda: o_pack(src, out=wire_o), es * n + wire_o.numel()),
                f"{o}_unpack": (lambda: o_unpack(wire_o, n, dtype, out=back),
                                wire_o.numel() + es * n),
                f"{o}_axpby": (lambda: o_axpby(src, wire_o, 0.5, 0.5, dst=acc),
                               2 * es * n + wire_o.numel()),
            })

        add_codec("mx8", ops.mx8_pack(src))
        if args.codec == "mxfp6":
            add_codec("mx4", ops.mx4_pack(src))
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
        wire2 = torch.empty(ops.mx8_nbytes(n), device="cuda", dtype=torch.uint8)
        ops.mx8_pack(src, out=wire2)  # what the other build's unpack reads
        code = ops._dtype_code(dtype)

        def other_pack():
            err = other.lz_mx8_pack(src.data_ptr(), code, wire2.data_ptr(), n,
                                    ops._current_stream_ptr())
            assert err == 0, err

        def other_unpack():
            err = other.lz_mx8_unpack(wire2.data_ptr(), back2.data_ptr(), code, n,
                                      ops._current_stream_ptr())
            assert err == 0, err

        cases["mx8_pack@compare-lib"] = (other_pack, es * n + wire2.numel())
        cases["mx8_unpack@compare-lib"] = (other_unpack, wire2.numel() + es * n)
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

    result = {"buffer_mib": args.mib, "dtype": dname, "iters": args.iters,
              "codec": args.codec}
    if args.compare_lib and args.codec == "mxfp8":
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
    got = pack(x.cuda()).cpu()
    want = getattr(mxwire, f"{pre}_pack_torch")(x)
    m = got.numel() - m // 32  # payload bytes; the scale bytes follow
    result["payload_mismatch_fraction"] = (got[:m] != want[:m]).float().mean().item()
    result["scale_mismatches"] = int((got[m:] != want[m:]).sum().item())
    print(f"payload mismatch fraction vs torch codec: "
          f"{result['payload_mismatch_fraction']}; scale byte mismatches: "
          f"{result['scale_mismatches']}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
