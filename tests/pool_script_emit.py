"""ws=1 pool scenario: the flagship's augment -> {checksum, evaluate} with the
scale_shift record on and off (LZY_HIP_EMIT), op bodies from bench.py, shard
size from their own LZY_BENCH_SHARD_MB.  Prints EMIT-POOL-OK."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (repo-root bench.py)
import lzy_amd.ops as ops  # noqa: E402
from lzy_amd import Lzy  # noqa: E402
from lzy_amd.runtime.pool import GpuPoolRuntime  # noqa: E402
from lzy_amd.utils.metrics import METRICS  # noqa: E402


def run(lzy: Lzy, name: str):
    h0 = ops._emit_hits
    with lzy.workflow(name):
        aug = bench.augment(bench.preprocess(bench.ingest(0, 7)))
        c = bench.checksum(aug)
        e = bench.evaluate(aug)
        out = int(c), float(e)
    return out, ops._emit_hits - h0


def main() -> None:
    assert ops._EMIT
    lzy = Lzy(runtime=GpuPoolRuntime())
    on, hits_on = run(lzy, "emit-on")
    os.environ["LZY_HIP_EMIT"] = "0"
    off, hits_off = run(lzy, "emit-off")
    del os.environ["LZY_HIP_EMIT"]
    on2, hits_on2 = run(lzy, "emit-on-again")
    print(f"on={on} hits={hits_on} off={off} hits={hits_off}", flush=True)
    assert hits_on == 2 and hits_off == 0 and hits_on2 == 2
    assert on[0] == off[0] == on2[0]            # the digest: bit for bit
    assert on == on2
    # two summation orders of ~1M positive values (docs/api.md)
    assert abs(on[1] - off[1]) <= 1e-5 * abs(off[1])
    assert METRICS.counter_value("lzy_stream_races") == 0
    print("EMIT-POOL-OK", flush=True)


if __name__ == "__main__":
    main()
