"""Probe for the packed-bundle gather kernel (run by hand on an MI355X; the
test suite never runs it).

Packs a list of device tensors into one uint8 buffer three ways, alternated
round-robin in one process and timed with device events per call AND as
host wall time per call (launch overhead is the point of one launch vs
many):

  * segcopy   ops.pack_tensors(leaves, out=buf)         one launch
  * kernel    the same launch with the table already on the device: the
              kernel alone, without the host's per-leaf table building
  * cat       torch.cat of the leaves' byte views       one launch, no padding
  * copy_loop per-leaf buf[off:off+n].copy_(leaf bytes) one launch per leaf

on two inputs:

  * state_dict  lzy_amd.models.transformer.TransformerLM() at its default
                size (f32 leaves)
  * synthetic   512 segments of mixed sizes, 1 GiB in all (--gib)
  * one_leaf    a single f32 leaf of the same total: the plain-copy yardstick,
                with ``ops.cast_copy`` f32 -> f32 (the repository's streaming
                copy kernel) as a fourth case

``--mode completion`` times op completion for one op that returns the
transformer state_dict: ``TaskResult.elapsed_s`` minus the op body, with
bundles on (this commit) and with ``channel_bundles`` off (the pickling
path of the parent commit), alternated.

``--mode wire`` times the MXFP8 bundle wire (``bundle_wire_cast``) on the
state_dict and on a synthetic bf16 bundle of the same segment mix, again
alternated in one process:

  * wire        ops.pack_tensors_wire(leaves, wired, out=buf)   one launch
  * wire_kernel the same launch with the table already on the device
  * per_leaf    what the parent commit can do: ops.mx8_pack per wired leaf
                plus one ops.pack_tensors of the other leaves
  * exact       ops.pack_tensors of all leaves, for context
  * decode / decode_kernel / decode_per_leaf   the receive side likewise:
                one ops.unpack_tensors_wire launch against ops.mx8_unpack
                per wired leaf
  * mx8_pack_one / mx8_unpack_one   the single-tensor kernels on ONE tensor
                of as many elements as the wired leaves hold together: the
                yardstick of the kernel-alone rate

Prints one JSON line last.
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import torch

import lzy_amd.ops as ops


def _summary(ts):
    ts = sorted(ts)
    return {
        "median_us": round(statistics.median(ts) * 1e6, 1),
        "min_us": round(ts[0] * 1e6, 1),
        "max_us": round(ts[-1] * 1e6, 1),
    }


def _time_alternating(cases, iters, warmup):
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    dev = {k: [] for k in cases}
    wall = {k: [] for k in cases}
    for _ in range(iters):
        for name, fn in cases.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            wall[name].append(time.perf_counter() - t0)
            dev[name].append(e0.elapsed_time(e1) * 1e-3)
    return dev, wall


def _pack_cases(leaves):
    sizes = [t.numel() * t.element_size() for t in leaves]
    offsets, total = ops.segcopy_layout(sizes, 128)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf_loop = torch.zeros(total, dtype=torch.uint8, device="cuda")
    byte_views = [t.reshape(-1).view(torch.uint8) for t in leaves]
    dst_views = [buf_loop[o: o + n] for o, n in zip(offsets, sizes)]
    cat_out = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")

    def segcopy():
        ops.pack_tensors(leaves, out=buf)

    def cat():
        torch.cat(byte_views, out=cat_out)

    def copy_loop():
        for d, s in zip(dst_views, byte_views):
            d.copy_(s)

    table, ntiles = ops.segcopy_table(
        [t.data_ptr() for t in leaves],
        [buf.data_ptr() + o for o in offsets], sizes)
    dev_table = ops._segcopy_upload(table, buf.device)
    lib = ops._require_segcopy()

    def kernel():
        ops._segcopy_run(lib, dev_table, len(sizes), ntiles, 128, buf.device)

    cases = {"segcopy": segcopy, "kernel": kernel, "cat": cat,
             "copy_loop": copy_loop}
    if len(leaves) == 1:
        cast_out = torch.empty_like(leaves[0])
        cases["cast_copy"] = lambda: ops.cast_copy(leaves[0], cast_out)
    segcopy()
    copy_loop()
    torch.cuda.synchronize()
    assert torch.equal(buf, buf_loop), "segcopy and the copy_ loop disagree"
    return cases, sum(sizes)


def _report(name, leaves, args):
    cases, payload = _pack_cases(leaves)
    dev, wall = _time_alternating(cases, args.iters, args.warmup)
    out = {"segments": len(leaves), "payload_mib": round(payload / 2**20, 2)}
    for k in cases:
        d, w = _summary(dev[k]), _summary(wall[k])
        out[k] = {
            "device": d, "wall": w,
            "gb_per_s": round(2 * payload / (d["median_us"] * 1e-6) / 1e9, 1),
        }
        print(f"{name:10s} {k:9s} device {d['median_us']:10.1f} us "
              f"[{d['min_us']} .. {d['max_us']}]  wall {w['median_us']:10.1f} us "
              f"[{w['min_us']} .. {w['max_us']}]  "
              f"{out[k]['gb_per_s']:8.1f} GB/s (read+written)")
    return out


def _state_dict_leaves():
    from lzy_amd.models.transformer import TransformerLM

    model = TransformerLM().to("cuda")
    return model, [v for v in model.state_dict().values()]


def _synthetic_leaves(gib: float, nseg: int = 512):
    import random

    rng = random.Random(0)
    # mixed sizes over three decades, odd byte counts included, scaled to
    # the requested total
    weights = [10 ** rng.uniform(0, 3) for _ in range(nseg)]
    scale = gib * 2**30 / sum(weights)
    sizes = [max(1, int(w * scale)) for w in weights]
    pool = torch.empty(max(sizes) + 64, dtype=torch.uint8, device="cuda")
    ops.fill_pattern(pool, seed=9)
    # distinct allocations, like real leaves
    return [pool[: n].clone() for n in sizes]


def _synthetic_float_leaves(gib: float, nseg: int = 512):
    """The segment mix of ``_synthetic_leaves`` as bf16 leaves (finite,
    positive values), ``gib`` GiB in all."""
    import random

    rng = random.Random(0)
    weights = [10 ** rng.uniform(0, 3) for _ in range(nseg)]
    scale = gib * 2**30 / sum(weights)
    numels = [max(1, int(w * scale) // 2) for w in weights]
    pool = torch.empty(max(numels) + 64, dtype=torch.bfloat16, device="cuda")
    ops.fill_pattern(pool, seed=9, mask16=0x3FFF)
    return [pool[: n].clone() for n in numels]


def _wire_cases(leaves):
    from lzy_amd.channels.transport import _WIRE_MIN_ELEMS

    floats = (torch.float32, torch.bfloat16, torch.float16)
    wired = [t.dtype in floats and t.numel() >= _WIRE_MIN_ELEMS for t in leaves]
    shapes, dtypes = [t.shape for t in leaves], [t.dtype for t in leaves]
    numels = [t.numel() for t in leaves]
    sizes = [t.numel() * t.element_size() for t in leaves]
    wsizes = [ops.mx8_nbytes(n) if w else s
              for n, s, w in zip(numels, sizes, wired)]
    woffs, wtotal = ops.segcopy_layout(wsizes, 128)
    offs, total = ops.segcopy_layout(sizes, 128)
    dev = leaves[0].device
    wbuf = torch.empty(wtotal, dtype=torch.uint8, device=dev)
    wbuf_loop = torch.zeros(wtotal, dtype=torch.uint8, device=dev)
    ebuf = torch.empty(total, dtype=torch.uint8, device=dev)
    dbuf = torch.empty(total, dtype=torch.uint8, device=dev)
    lib = ops._require_segcodec()

    def wire():
        ops.pack_tensors_wire(leaves, wired, out=wbuf)

    def exact():
        ops.pack_tensors(leaves, out=ebuf)

    # the parent commit's means: one mx8_pack per wired leaf, one segcopy
    # of the rest (into a buffer of its own: the parent has no mixed layout)
    wired_leaves = [t for t, w in zip(leaves, wired) if w]
    wired_out = [wbuf_loop[o: o + n] for o, n, w in zip(woffs, wsizes, wired) if w]
    rest = [t for t, w in zip(leaves, wired) if not w]
    rest_buf = torch.empty(
        ops.segcopy_nbytes([t.numel() * t.element_size() for t in rest], 128),
        dtype=torch.uint8, device=dev) if rest else None

    def per_leaf():
        for t, o in zip(wired_leaves, wired_out):
            ops.mx8_pack(t, out=o)
        if rest:
            ops.pack_tensors(rest, out=rest_buf)

    modes = [ops.SEGCODEC_ENCODE + ops._dtype_code(t.dtype) if w
             else ops.SEGCODEC_RAW for t, w in zip(leaves, wired)]
    counts = [n if w else s for n, s, w in zip(numels, sizes, wired)]
    etab, entiles = ops.segcodec_table(
        [t.data_ptr() for t in leaves], [wbuf.data_ptr() + o for o in woffs],
        counts, modes)
    etab_dev = ops._segcopy_upload(etab, dev)
    dmodes = [ops.SEGCODEC_DECODE + ops._dtype_code(t.dtype) if w
              else ops.SEGCODEC_RAW for t, w in zip(leaves, wired)]
    dtab, dntiles = ops.segcodec_table(
        [wbuf.data_ptr() + o for o in woffs], [dbuf.data_ptr() + o for o in offs],
        counts, dmodes)
    dtab_dev = ops._segcopy_upload(dtab, dev)

    import ctypes

    def _run(tab, ntiles):
        ops._check(lib.lz_segcodec(
            ctypes.c_void_p(tab.data_ptr()), len(leaves), ntiles, 128,
            ctypes.c_void_p(ops._current_stream_ptr())))

    def wire_kernel():
        _run(etab_dev, entiles)

    def decode():
        ops.unpack_tensors_wire(wbuf, wired, shapes, dtypes, out=dbuf)

    def decode_kernel():
        _run(dtab_dev, dntiles)

    dec_out = [torch.empty_like(t) for t in wired_leaves]
    dec_src = [wbuf[o: o + n] for o, n, w in zip(woffs, wsizes, wired) if w]

    def decode_per_leaf():
        for s, o in zip(dec_src, dec_out):
            ops.mx8_unpack(s, o.shape, o.dtype, out=o)

    n_wired = sum(t.numel() for t in wired_leaves)
    one = torch.empty(n_wired, dtype=wired_leaves[0].dtype, device=dev)
    ops.fill_pattern(one, seed=4, mask16=0x3FFF)
    one_wire = torch.empty(ops.mx8_nbytes(n_wired), dtype=torch.uint8, device=dev)
    one_back = torch.empty_like(one)

    def mx8_pack_one():
        ops.mx8_pack(one, out=one_wire)

    def mx8_unpack_one():
        ops.mx8_unpack(one_wire, one.shape, one.dtype, out=one_back)

    cases = {"wire": wire, "wire_kernel": wire_kernel, "per_leaf": per_leaf,
             "exact": exact, "decode": decode, "decode_kernel": decode_kernel,
             "decode_per_leaf": decode_per_leaf, "mx8_pack_one": mx8_pack_one,
             "mx8_unpack_one": mx8_unpack_one}
    # the two ways must agree before either is timed
    wire()
    per_leaf()
    torch.cuda.synchronize()
    for o, n, w in zip(woffs, wsizes, wired):
        if w:
            assert torch.equal(wbuf[o: o + n], wbuf_loop[o: o + n]), \
                "one launch and per-leaf mx8_pack disagree"
    decode()
    decode_per_leaf()
    torch.cuda.synchronize()
    k = 0
    for o, t, w in zip(offs, leaves, wired):
        if w:
            got = dbuf[o: o + t.numel() * t.element_size()]
            assert torch.equal(got, dec_out[k].reshape(-1).view(torch.uint8)), \
                "one-launch decode and per-leaf mx8_unpack disagree"
            k += 1
    wired_bytes = sum(s for s, w in zip(sizes, wired) if w)
    wired_wire = sum(s for s, w in zip(wsizes, wired) if w)
    rest_bytes = sum(sizes) - wired_bytes
    # bytes read + written per case, for the GB/s column
    moved = {
        "wire": wired_bytes + wired_wire + 2 * rest_bytes,
        "exact": 2 * sum(sizes),
        "mx8_pack_one": wired_bytes + one_wire.numel(),
    }
    moved["wire_kernel"] = moved["per_leaf"] = moved["wire"]
    moved["decode"] = moved["decode_kernel"] = moved["wire"]
    moved["decode_per_leaf"] = wired_bytes + wired_wire
    moved["mx8_unpack_one"] = moved["mx8_pack_one"]
    info = {"segments": len(leaves), "wired_segments": len(wired_leaves),
            "payload_mib": round(sum(sizes) / 2**20, 2),
            "wire_mib": round(wtotal / 2**20, 2),
            "wired_elems": n_wired}
    return cases, moved, info


def _report_wire(name, leaves, args):
    cases, moved, out = _wire_cases(leaves)
    dev, wall = _time_alternating(cases, args.iters, args.warmup)
    for k in cases:
        d, w = _summary(dev[k]), _summary(wall[k])
        out[k] = {
            "device": d, "wall": w,
            "gb_per_s": round(moved[k] / (d["median_us"] * 1e-6) / 1e9, 1),
        }
        print(f"{name:10s} {k:15s} device {d['median_us']:10.1f} us "
              f"[{d['min_us']} .. {d['max_us']}]  wall {w['median_us']:10.1f} us "
              f"[{w['min_us']} .. {w['max_us']}]  "
              f"{out[k]['gb_per_s']:8.1f} GB/s (read+written)")
    return out


def wire_mode(args) -> dict:
    ops._require_segcodec()
    result = {"tile_elems": ops.SEGCODEC_TILE_ELEMS}
    model, leaves = _state_dict_leaves()
    result["state_dict"] = _report_wire("state_dict", leaves, args)
    del model, leaves
    leaves = _synthetic_float_leaves(args.gib)
    result["synthetic"] = _report_wire("synthetic", leaves, args)
    return result


def completion_mode(args) -> dict:
    from lzy_amd.config import Config
    from lzy_amd.runtime.taskspec import TaskSpec, WorkerStore, run_taskspec

    model, _ = _state_dict_leaves()
    body_s = []

    def op_body():
        t0 = time.perf_counter()
        sd = model.state_dict()
        body_s.append(time.perf_counter() - t0)
        return sd

    # hand the worker the live function (a pickled copy would carry its own
    # model and its own ``body_s``): seed the unpickle memo under the bytes
    from lzy_amd.runtime import taskspec as _ts
    from lzy_amd.sched import xxhash64

    func_bytes = b"bundle-probe-op"
    _ts._FUNC_CACHE[xxhash64(func_bytes)] = op_body
    times = {"bundles_on": [], "bundles_off": []}
    kinds = {}
    for it in range(args.warmup + args.iters):
        for name, on in (("bundles_on", True), ("bundles_off", False)):
            Config.reset(channel_bundles=on)
            store = WorkerStore(device=torch.device("cuda", 0))
            spec = TaskSpec(
                task_id=f"t{it}{name}", name="train", func_bytes=func_bytes,
                arg_entries=[], kwarg_entries={},
                output_entries=[(f"e{it}{name}", "")], exception_entry="x",
            )
            torch.cuda.synchronize()
            res = run_taskspec(spec, store, None, None, echo_logs=False)
            assert res.ok, res
            kinds[name] = res.outputs[0]["kind"]
            if it >= args.warmup:
                times[name].append(res.elapsed_s - body_s[-1])
            store.drop(f"e{it}{name}")
    Config.reset()
    out = {k: {**_summary(v), "kind": kinds[k]} for k, v in times.items()}
    for k, v in out.items():
        print(f"op completion {k:11s} ({v['kind']:6s}) median {v['median_us']:10.1f} us "
              f"[{v['min_us']} .. {v['max_us']}]")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["pack", "completion", "wire", "all"], default="all")
    ap.add_argument("--gib", type=float, default=1.0, help="synthetic bundle size")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    assert torch.cuda.is_available(), "the probe needs a GPU"
    ops._require_segcopy()
    result = {"iters": args.iters, "tile": ops.SEGCOPY_TILE}
    if args.mode in ("pack", "all"):
        model, leaves = _state_dict_leaves()
        result["state_dict"] = _report("state_dict", leaves, args)
        del model, leaves
        leaves = _synthetic_leaves(args.gib)
        result["synthetic"] = _report("synthetic", leaves, args)
        del leaves
        one = torch.empty(int(args.gib * 2**28), dtype=torch.float32, device="cuda")
        ops.fill_pattern(one, seed=4)
        result["one_leaf"] = _report("one_leaf", [one], args)
        del one
    if args.mode in ("completion", "all"):
        result["completion"] = completion_mode(args)
    if args.mode == "wire":  # "all" stays what it was
        result["wire"] = wire_mode(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
