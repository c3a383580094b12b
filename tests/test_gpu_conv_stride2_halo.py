"""3x3 / stride 2 / pad 1 convs (Downsample.conv) on conv_s2_halo_kernel (csrc/igemm.hip): against torch, against the generic kernel
(option s2_halo = 0), statistics slots, the fp32x3 domain, batch invariance and which geometries take the new form."""
import math

import pytest
import torch
import torch.nn.functional as F

from eo_diffusion_amd import _lib
from eo_diffusion_amd.engine import Act, Program
from tests.gpu_util import DEV, TOL
from tests.synth import synth_input

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _ref(x, w, b):
    return F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)


def _run(prec, x, w, b, on=True, stats=False):
    """x NCHW fp32 (cpu) -> the stride-2 conv through a Program -> (NCHW fp32 output, stats tensor or None, kernel of the op table)"""
    L = _lib.lib()
    prev = L.eod_set_option(b"s2_halo", int(on))
    try:
        N, C, H, W = x.shape
        Cout = w.shape[0]
        prog = Program(DEV, prec)
        a = Act(prog.own(x.to(DEV).permute(0, 2, 3, 1).contiguous().to(prog.tdtype)), N, H, W, C)
        y, i = prog.conv(a, prog.pack_conv(w.to(DEV)), prog.f32(b.to(DEV)), Cout, ksize=3, stride=2, pad=1, stats=stats)
        kernel = [o for o in prog.op_stats() if o["kind"] == "conv"][-1]["kernel"]
        prog.run()
        torch.cuda.synchronize()
        out = y.t.float().permute(0, 3, 1, 2).contiguous().cpu()
        st = y.stats[0].clone().cpu() if stats else None
        return out, st, kernel
    finally:
        L.eod_set_option(b"s2_halo", prev)


def _data(tag, N, C, H, W, Cout):
    x = synth_input(f"s2x{tag}", (N, C, H, W), 91)
    w = synth_input(f"s2w{tag}", (Cout, C, 3, 3), 92, scale=1.0 / math.sqrt(C * 9))
    b = synth_input(f"s2b{tag}", (Cout,), 93, scale=0.1)
    return x, w, b


# N, C, H, W, Cout: the three Downsample convs of A0 @ 256 (reduced batch), odd input maps (Ho = ceil(H / 2)) with a half-masked N-tile,
# a ragged Cout (the new form only takes maps the generic kernel would run unsplit in K: 16 x 32 outputs and up at 128 columns)
SHAPES = [(2, 128, 256, 256, 128), (2, 256, 128, 128, 256), (2, 384, 64, 64, 384), (2, 64, 63, 31, 192), (3, 128, 32, 64, 136)]


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_s2_halo_vs_torch_and_generic(prec, shape):
    N, C, H, W, Cout = shape
    x, w, b = _data(shape, N, C, H, W, Cout)
    ref = _ref(x, w, b)
    y, _, kern = _run(prec, x, w, b)
    assert kern == "conv_s2_halo_kernel"
    assert y.shape == ref.shape
    assert _rel(y, ref) < TOL[prec], _rel(y, ref)
    y0, _, kern0 = _run(prec, x, w, b, on=False)
    assert kern0 == "igemm_kernel"
    assert _rel(y, y0) < (1e-6 if prec == "fp32x3" else 2e-3), _rel(y, y0)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_s2_halo_statistics_slots(prec):
    N, C, H, W, Cout = 2, 128, 64, 64, 256
    x, w, b = _data("st", N, C, H, W, Cout)
    y, st, kern = _run(prec, x, w, b, stats=True)
    assert kern == "conv_s2_halo_kernel"
    y0, st0, _ = _run(prec, x, w, b, on=False, stats=True)
    assert st.shape == st0.shape  # the same slots on either kernel
    tot = st.double().sum(dim=1)  # [N][Cout][2]
    yd = y.double()
    s_ref = yd.sum(dim=(2, 3))
    q_ref = (yd * yd).sum(dim=(2, 3))
    assert _rel(tot[..., 0], s_ref) < 1e-5 and _rel(tot[..., 1], q_ref) < 1e-5
    # per-group (32 groups) mean / var as the next GroupNorm derives them, against torch's on the output
    G, cnt = 32, (Cout // 32) * y.shape[2] * y.shape[3]
    gs, gq = tot[..., 0].view(N, G, -1).sum(-1), tot[..., 1].view(N, G, -1).sum(-1)
    mean, var = gs / cnt, gq / cnt - (gs / cnt) ** 2
    yg = yd.view(N, G, -1)
    assert torch.allclose(mean, yg.mean(-1), rtol=1e-6, atol=1e-9)
    assert torch.allclose(var, yg.var(-1, unbiased=False), rtol=1e-5, atol=1e-9)


def test_s2_halo_output_channels_of_any_relative_magnitude():
    N, C, H, W, Cout = 2, 128, 32, 64, 256
    mag = 10.0 ** torch.linspace(-6, 6, Cout)[torch.randperm(Cout, generator=torch.Generator().manual_seed(7))]
    x, w, b = _data("mag", N, C, H, W, Cout)
    w, b = w * mag[:, None, None, None], b * mag
    ref = _ref(x, w, b)
    y, _, kern = _run("fp32x3", x, w, b)
    assert kern == "conv_s2_halo_kernel"
    err = ((y.double() - ref).pow(2).sum(dim=(0, 2, 3)) / ref.pow(2).sum(dim=(0, 2, 3))).sqrt()  # rel-L2 per output channel
    assert float(err.max()) < TOL["fp32x3"], float(err.max())


@pytest.mark.parametrize("scale", [1e-12, 1.0, 3e18])
def test_s2_halo_fp32x3_at_any_input_magnitude(scale):
    N, C, H, W, Cout = 2, 256, 64, 64, 128
    x, w, b = _data(f"am{scale}", N, C, H, W, Cout)
    x = x * scale
    b = b * scale
    ref = _ref(x, w, b)
    y, _, kern = _run("fp32x3", x, w, b)
    assert kern == "conv_s2_halo_kernel"
    assert torch.isfinite(y).all()
    assert _rel(y, ref) < TOL["fp32x3"], _rel(y, ref)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_s2_halo_batch_invariant_and_deterministic(prec):
    N, C, H, W, Cout = 16, 128, 64, 64, 128
    x, w, b = _data("bi", N, C, H, W, Cout)
    y, _, kern = _run(prec, x, w, b)
    assert kern == "conv_s2_halo_kernel"
    y2, _, _ = _run(prec, x, w, b)
    assert torch.equal(y, y2)
    for n in (0, 5, 15):
        yn, _, _ = _run(prec, x[n:n + 1], w, b)
        assert torch.equal(yn[0], y[n]), n


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_s2_halo_kernel_choice(prec):
    # a 7 x 7 output (14 x 14 input) does not tile into 8 x 16 patches: the generic kernel, with or without the option
    x, w, b = _data("c7", 2, 128, 14, 14, 128)
    y, _, kern = _run(prec, x, w, b)
    y0, _, kern0 = _run(prec, x, w, b, on=False)
    assert kern == kern0 == "igemm_kernel"
    assert torch.equal(y, y0)
    assert _rel(y, _ref(x, w, b)) < TOL[prec]
