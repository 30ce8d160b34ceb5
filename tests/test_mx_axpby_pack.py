"""The forwarding-node dispatchers of channels/mxwire.py on CPU tensors: the
composition of the torch combine and the torch pack, bit for bit (the GPU
kernels behind them: tests/test_gpu_mx_axpby_pack.py)."""
import pytest
import torch

from lzy_amd.channels import mxwire

ALPHA, BETA = 0.5, -1.5


@pytest.mark.parametrize("wire", mxwire.MX_WIRES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16],
                         ids=["f32", "bf16", "f16"])
def test_cpu_dispatch_is_combine_then_pack(wire, dtype):
    n = 4101
    g = torch.Generator().manual_seed(11)
    a, b = (torch.randn(n, generator=g).to(dtype) for _ in range(2))
    pack, _, axpby = mxwire.wire_codec(wire)
    axpby_pack, axpby2_pack = mxwire.wire_fused(wire)
    win = pack(b)
    want = axpby(a, win, ALPHA, BETA)
    dst, wout = axpby_pack(a, win, ALPHA, BETA)
    assert dst.dtype == dtype and torch.equal(dst.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(wout, pack(want))
    # out= forms, in place: same bits
    acc, buf = a.clone(), torch.empty_like(wout)
    got = axpby_pack(acc, win, ALPHA, BETA, dst=acc, wire_out=buf)
    assert got[0] is acc and got[1] is buf
    assert torch.equal(acc.view(torch.uint8), want.view(torch.uint8)) and torch.equal(buf, wout)
    want2 = torch.add(a * ALPHA, b, alpha=BETA)
    dst2, wout2 = axpby2_pack(a, b, ALPHA, BETA)
    assert torch.equal(dst2.view(torch.uint8), want2.view(torch.uint8))
    assert torch.equal(wout2, pack(want2))


def test_wire_fused_rejects_unknown_name():
    with pytest.raises(ValueError, match="wire must be one of"):
        mxwire.wire_fused("fp8")
