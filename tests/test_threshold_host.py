"""Dynamic thresholding, host side (no GPU): the rank arithmetic of DynamicThreshold, the emulation tests/threshold_ref.py against
torch.quantile in float64, the two consequences include/eodiff.h states (the static clamp where the quantile is at most 1; idempotence),
and every refusal that needs no device."""
from fractions import Fraction
import inspect
import math

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.threshold import DynamicThreshold, check
from tests import threshold_ref as TR

NS = (1, 2, 77, 768, 4099, 12288, 196608)
QS = (0.0, 0.5, 0.9, 0.995, 0.999, 1.0)


def test_rank_is_exact_in_float64():
    assert DynamicThreshold(0.995).rank(196608)[0] == 195623            # (fp32 would round 0.995 * 196607 = 195623.965 to a multiple of 1 / 64)
    n = 2 ** 31 - 1
    k, frac = DynamicThreshold(0.995).rank(n)
    assert k == math.floor(Fraction(0.995) * (n - 1)) and 0.0 <= frac < 1.0     # (the exact product of the float64 0.995)
    for n in NS + (2 ** 31 - 1,):
        assert DynamicThreshold(0.0).rank(n) == (0, 0.0)
        assert DynamicThreshold(1.0).rank(n) == (n - 1, 0.0)
        for q in QS + (1.0 - 2.0 ** -40, 0.3333333333333333):
            k, frac = DynamicThreshold(q).rank(n)
            assert (k, frac) == TR.rank(q, n)
            assert 0 <= k <= n - 1 and 0.0 <= frac < 1.0
            assert frac == float(np.float32(frac))                       # (an fp32 value)
            assert abs((k + frac) - q * (n - 1)) <= 2.0 ** -22                # (float64 of the product near 2^31, fp32 of frac)


@pytest.mark.parametrize("n", NS)
def test_emulation_against_float64_quantile(n):
    """v = lo + frac * (hi - lo) in fp32 against torch.quantile(|p|.double(), q): within 2 ulp (0.77 ulp measured at worst: the
    interpolation has three fp32 roundings, each at most half an ulp of a value no larger than the result)"""
    g = torch.Generator().manual_seed(n)
    worst = 0.0
    for q in QS:
        for scale in (0.3, 1.0, 2.5):
            p = torch.randn(4, n, generator=g) * scale
            out, s, v = TR.threshold(p, q)
            v64 = torch.quantile(p.abs().double(), q, dim=1)
            ulp = np.spacing(v64.abs().float().numpy()).astype(np.float64)
            worst = max(worst, float(((v.double() - v64).abs().numpy() / ulp).max()))
            if bool((v <= 1).all()):
                assert torch.equal(out, p.clamp(-1, 1)), (n, q, scale)    # (s = 1: the static clamp, division by 1 is exact)
            if q == 1.0:
                assert torch.equal(v, p.abs().amax(dim=1))
            assert float(out.abs().max()) <= 1.0
            out2, s2, _ = TR.threshold(out, q)                           # idempotent: the second application has s = 1
            assert torch.equal(s2, torch.ones_like(s2)) and torch.equal(out2, out)
    print(f"n = {n}: worst |v - quantile64| = {worst:.2f} ulp")
    assert worst <= 2.0


def test_emulation_nan_and_cap():
    p = torch.tensor([[0.5, -3.0, float("nan"), 2.0, float("inf"), -float("inf"), 1.0, -0.25]])
    out, s, v = TR.threshold(p, 0.5, cap=4.0)                            # pos = 3.5: half way between |2.0| and |-3.0|
    assert float(v) == 2.5 and float(s) == 2.5
    f = lambda z: float(np.float32(z) / np.float32(2.5))
    assert torch.equal(out, torch.tensor([[f(0.5), -1.0, -1.0, f(2.0), 1.0, -1.0, f(1.0), f(-0.25)]]))   # (a NaN element becomes -1)
    out, s, v = TR.threshold(p, 1.0)                                     # the rank element is the NaN: s = 1, the static clamp
    assert math.isnan(float(v)) and float(s) == 1.0
    assert torch.equal(out, torch.tensor([[0.5, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -0.25]]))
    out, s, v = TR.threshold(torch.tensor([[4.0, -8.0, 2.0]]), 1.0, cap=3.0)
    assert float(v) == 8.0 and float(s) == 3.0 and torch.equal(out, torch.tensor([[1.0, -1.0, 2.0 / 3.0]]))


def test_constructor_and_bind_refusals():
    for q in (-0.1, 1.0001, float("nan"), "0.9", None, True):
        with pytest.raises(EodError, match="quantile"):
            DynamicThreshold(q)
    for mv in (0.5, 0.0, -1.0, float("nan"), "3", True):
        with pytest.raises(EodError, match="max_value"):
            DynamicThreshold(0.9, mv)
    with pytest.raises(EodError, match="per"):
        DynamicThreshold(0.9, None, "tile")
    t = DynamicThreshold(0.9, 3.0, "channel")
    assert (t.quantile, t.cap, t.per) == (0.9, 3.0, "channel") and DynamicThreshold().cap == math.inf and DynamicThreshold(1, 1).cap == 1.0
    assert DynamicThreshold(max_value=float("inf")).cap == math.inf
    # device None: the refusals alone, nothing allocated
    assert DynamicThreshold().bind("x", (1, 4, 2048, 2048), None) is None
    assert DynamicThreshold().bind("x", (3, 1, 2 ** 16, 2 ** 15 - 1), None) is None        # n = 2^31 - 2^16
    with pytest.raises(EodError, match="2\\^31 - 1"):
        DynamicThreshold().bind("x", (1, 2, 2 ** 15, 2 ** 15), None)                      # n = 2^31
    assert DynamicThreshold(per="channel").bind("x", (1, 2, 2 ** 15, 2 ** 15), None) is None   # (per band: 2^30 each)
    with pytest.raises(EodError, match="2\\^31 - 1"):
        DynamicThreshold(per="channel").bind("x", (1, 2, 2 ** 16, 2 ** 15), None)
    with pytest.raises(EodError, match="B, C, H, W"):
        DynamicThreshold().bind("x", (3, 16, 16), None)
    with pytest.raises(EodError, match="DynamicThreshold or None"):
        check(0.995, "x", (1, 3, 16, 16))
    check(None, "x", (1, 3, 16, 16))


def test_dropin_module_path():
    from eo_diffusion_amd.dropin.diffusion import threshold as D
    import eo_diffusion_amd.diffusion.threshold as M
    assert D.DynamicThreshold is M.DynamicThreshold and D.dynamic_threshold is M.dynamic_threshold and D.MAX_N == 2 ** 31 - 1


def test_every_sampler_and_sharded_function_takes_threshold_last():
    from eo_diffusion_amd import dist
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion
    sharded = [f for name, f in vars(dist).items() if name.startswith("sharded_") and callable(f)]
    assert len(sharded) >= 2
    fns = sharded + [EODiffusion.sampling, EODiffusion.sampling_scene, EODiffusion.check_scene_args, DDIMSampler.ddim_sampling,
                     DDIMSampler.sample_scene, DPMSolverSampler.sample, DPMSolverSampler.sample_scene]
    for f in fns:
        params = [p for p in inspect.signature(f).parameters.values() if p.kind != p.VAR_KEYWORD]
        assert params[-1].name == "threshold" and params[-1].default is None, f.__qualname__
    params = [p for p in inspect.signature(DDIMSampler.sample).parameters.values() if p.kind != p.VAR_KEYWORD]
    assert params[-1].name == "threshold" and params[-1].default is None


def test_check_scene_args_refuses_without_a_device():
    """EODiffusion.check_scene_args: skip_known with a threshold, and an object that is no DynamicThreshold, with nothing launched"""
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, *a, **k):
            raise AssertionError("the UNet must not be called")
    m = EODiffusion(Never(), timesteps=4, image_size=16, in_channels=3, cond_type="sum", device="cpu")
    cond = torch.zeros(1, 4, 24, 24)
    m.check_scene_args((24, 24), "cuda:0", cond=cond, overlap=8, threshold=DynamicThreshold(0.9))
    with pytest.raises(EodError, match="skip_known=True cannot be combined with `threshold`"):
        m.check_scene_args((24, 24), "cuda:0", cond=cond, overlap=8, skip_known=True, threshold=DynamicThreshold(0.9))
    with pytest.raises(EodError, match="DynamicThreshold or None"):
        m.check_scene_args((24, 24), "cuda:0", cond=cond, overlap=8, threshold=0.9)
