"""Byte-rate probe for the block-scaled FP8 (mxfp8) wire kernels (run on
an MI355X).

On a 1 GiB bf16 buffer, times in one process, interleaved round-robin:

  * ops.mx8_pack     bf16 -> mxfp8 wire      (reads 2 B, writes 33/32 B / elem)
  * ops.mx8_unpack   mxfp8 wire -> bf16
  * ops.cast_copy    bf16 -> fp8e4m3         (the yardstick: reads 2 B, writes 1 B)
  * ops.cast_copy    fp8e4m3 -> bf16

Each call is timed with device events; the figure reported is
(bytes read + bytes written) / median time.  Also reports the fraction of
payload bytes on which the kernel and the torch codec disagree, over a
1M-element sample.  Prints one JSON line last.
"""
import argparse
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import torch

import lzy_amd.ops as ops
from lzy_amd.channels.mxwire import mx8_pack_torch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024, help="bf16 buffer size")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    assert torch.cuda.is_available(), "the probe needs a GPU"
    ops._require_native()
    n = (args.mib << 20) // 2
    src = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    ops.fill_pattern(src, seed=3, mask16=0x3FFF)  # finite positive bf16
    wire = torch.empty(ops.mx8_nbytes(n), device="cuda", dtype=torch.uint8)
    fp8 = torch.empty(n, device="cuda", dtype=torch.float8_e4m3fn)
    back = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    ops.mx8_pack(src, out=wire)
    ops.cast_copy(src, fp8)

    cases = {
        "mx8_pack": (lambda: ops.mx8_pack(src, out=wire), 2 * n + wire.numel()),
        "mx8_unpack": (lambda: ops.mx8_unpack(wire, n, torch.bfloat16, out=back),
                       wire.numel() + 2 * n),
        "cast_bf16_to_e4m3": (lambda: ops.cast_copy(src, fp8), 2 * n + n),
        "cast_e4m3_to_bf16": (lambda: ops.cast_copy(fp8, back), n + 2 * n),
    }
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

    result = {"buffer_mib": args.mib, "iters": args.iters}
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
    x = x.to(torch.bfloat16)
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
