"""Host: the observation of diffusion/consistency.py -- every refusal, before anything could be launched -- and the CPU references of
tests/consistency_ref.py: the float64 projector (idempotent, A(Px) = y on observed blocks), the float64 DDIM loop on the Gaussian toy of
tests/dpm_ref.py with the projector, and the fp32 emulation of the two step kernels against the float64 projector and the plain steps."""
import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.consistency import Observation, bind, block_mean
from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
from tests import consistency_ref as CR
from tests import dpm_ref as DR
from tests.helpers import bits_equal
from tests.synth import synth_input

EPS = float(np.finfo(np.float32).eps)


def _v(*shape):
    return torch.zeros(*shape)


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw", [
    dict(factors=(1, 2)),                                   # wrong channel count
    dict(factors=(1, 2, 4, 1)),
    dict(factors=(1, 2, 0)), dict(factors=(1, 2, 9)), dict(factors=(1, 2, -2)),       # outside 1 .. 8
    dict(factors=(1, 2, 2.0)), dict(factors=(1, 2, True)), dict(factors=(1, "2", 4)), dict(factors=3), dict(factors=()),
    dict(factors=(1, 2, 5)),                                # 5 does not divide 12 x 16
    dict(factors=(1, 2, 8)),                                # 8 divides 16, not 12
    dict(factors=(1, 3, 1)),                                # 3 divides 12, not 16
    dict(values=_v(2, 3, 12)), dict(values=_v(3, 12, 16)),  # not [B, C, H, W]
    dict(values=_v(2, 3, 12, 16).double()), dict(values=_v(2, 3, 12, 16).half()),
    dict(mask=_v(2, 2, 12, 16)), dict(mask=_v(2, 3, 12, 15)), dict(mask=_v(12, 16)), dict(mask=_v(3, 1, 12, 16)),
    dict(mask=_v(2, 1, 12, 16).double()),
    dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=-0.1), dict(weight=1.5), dict(weight="1"), dict(weight=True),
    dict(weight=None), dict(weight=[0.5, float("nan")]), dict(weight=[0.5, 2.0]), dict(weight=[0.5, "x"]),
    dict(weight=1.0 + 1e-6),
])
def test_observation_refuses(kw):
    args = dict(values=_v(2, 3, 12, 16), factors=(1, 2, 4), mask=None, weight=1.0)
    Observation(**args)
    args.update(kw)
    with pytest.raises(EodError):
        Observation(**args)


def test_what_is_accepted():
    o = Observation(_v(1, 3, 12, 16), np.asarray([1, 2, 4]), mask=_v(2, 1, 12, 16), weight=np.float32(0.25))
    assert o.factors == (1, 2, 4) and o.weights == [0.25] and not o.per_evaluation
    o = Observation(_v(2, 3, 12, 16), [4, 4, 4], mask=_v(1, 3, 12, 16), weight=(0.0, 1.0, 0.5))
    assert o.per_evaluation and o.weights == [0.0, 1.0, 0.5]
    assert bind(None, "x", (2, 3, 12, 16), 5, "cpu") is None


@pytest.mark.parametrize("shape,n_eval", [((2, 4, 12, 16), 3), ((2, 3, 16, 16), 3), ((2, 3, 12, 12), 3), ((3, 3, 12, 16), 3),
                                          ((2, 3, 12, 16), 2), ((2, 3, 12, 16), 4)])
def test_bind_refuses_what_does_not_fit_the_call(shape, n_eval):
    o = Observation(_v(2, 3, 12, 16), (1, 2, 4), mask=_v(1, 1, 12, 16), weight=[1.0, 0.5, 0.25])
    with pytest.raises(EodError):
        o.bind("call", shape, n_eval, "cpu")
    with pytest.raises(EodError):
        bind("not an observation", "call", shape, n_eval, "cpu")


def test_bind_checks_the_mask_too_and_block_mean_refuses_on_the_host():
    o = Observation(_v(1, 3, 12, 16), (1, 2, 4), mask=_v(2, 1, 12, 16))
    with pytest.raises(EodError):
        o.bind("call", (3, 3, 12, 16), 4, "cpu")
    for x, f in ((_v(1, 3, 12, 16), (1, 2)), (_v(1, 3, 12, 16), (1, 2, 5)), (_v(3, 12, 16), (1, 2, 4)), (_v(1, 3, 12, 16), (1, 2, 9)),
                 (_v(1, 3, 12, 16), (1, 2, 4))):               # (the last one: a CPU tensor -- there is no CPU path)
        with pytest.raises(EodError):
            block_mean(x, f)


# ------------------------------------------------------------------------------------------------------------ the float64 projector
def _case64(seed, B=2, factors=(1, 2, 3, 6), H=12, W=18):
    rng = np.random.default_rng(seed)
    C = len(factors)
    p0 = rng.standard_normal((B, C, H, W))
    values = CR.block_mean64(rng.uniform(-1, 1, (B, C, H, W)), factors)
    cells = rng.integers(0, 2, (B, C, H // 6, W // 6)).astype(np.float64)           # a mask that is constant on every block of every factor
    mask = np.kron(cells, np.ones((6, 6)))
    return p0, values, mask, factors


def test_projector_is_idempotent_and_meets_the_observation_on_masked_blocks():
    p0, values, mask, factors = _case64(0)
    assert 0.2 < mask.mean() < 0.8
    P = CR.project64(p0, values, factors, mask)
    assert np.abs(CR.project64(P, values, factors, mask) - P).max() < 1e-14
    res = np.abs(CR.block_mean64(P, factors) - values)
    assert res[mask == 1].max() < 1e-14
    assert np.array_equal(P[mask == 0], p0[mask == 0])                                # free blocks are left alone
    assert np.abs(P - p0)[mask == 1].max() > 0.1                                      # (and the observed ones are not)
    # the correction is constant on every block: the part of p0 in the null space of A is untouched
    d = P - p0
    assert np.abs(d - CR.block_mean64(d, factors)).max() < 1e-14
    full = CR.project64(p0, values, factors)
    assert np.abs(CR.block_mean64(full, factors) - values).max() < 1e-14
    assert np.array_equal(CR.project64(p0, values, factors, mask, 0.0), p0)


def test_float64_ddim_loop_on_the_toy_ends_on_the_observation():
    """DDIM with eta 0 on tests/dpm_ref.py's Gaussian pixels, seen as a 4 x 32 x 32 image with factors (1, 2, 4, 8): with the projector
    after every prediction the last prediction has the observation's block means, and so has the end state up to what the last step adds:
    x = sqrt(a0) p0 + sqrt(1 - a0) e, so |A x - y| <= (1 - sqrt(a0)) |y|max + sqrt(1 - a0) |e|max with a0 = acp[0]; with weight 0 the loop is the unconstrained one, bit for bit."""
    from oracle import schedule as SCH
    acp = SCH.eo_cosine_tables(1000)["alphas_cumprod"].numpy().astype(np.float64)
    levels = make_dpm_timesteps("uniform", 20, acp)
    values = CR.block_mean64(np.random.default_rng(5).uniform(-1, 1, CR.TOY_SHAPE), CR.TOY_FACTORS)
    x, p0, e = CR.ddim_f64(acp, levels, values)
    free, _, _ = CR.ddim_f64(acp, levels)
    assert np.array_equal(free, DR.ddim_f64(acp, levels))
    assert np.abs(CR.block_mean64(p0.reshape(CR.TOY_SHAPE), CR.TOY_FACTORS) - values).max() < 1e-13
    last = (1.0 - np.sqrt(acp[0])) * np.abs(values).max() + np.sqrt(1.0 - acp[0]) * np.abs(e).max()
    assert last < 0.1
    assert np.abs(CR.block_mean64(x.reshape(CR.TOY_SHAPE), CR.TOY_FACTORS) - values).max() <= last
    assert np.abs(CR.block_mean64(free.reshape(CR.TOY_SHAPE), CR.TOY_FACTORS) - values).max() > 0.3
    zero, _, _ = CR.ddim_f64(acp, levels, values, lam=0.0)
    assert np.array_equal(zero, free)
    _, p_half, _ = CR.ddim_f64(acp, levels, values, lam=0.5)                          # (a soft weight lands in between)
    r = np.abs(CR.block_mean64(p_half.reshape(CR.TOY_SHAPE), CR.TOY_FACTORS) - values).max()
    assert 1e-6 < r < 0.3


# ------------------------------------------------------------------------------------------------------------ the fp32 emulation
def _case32(factors, B=2, H=24, W=48, seed=3, masked=True):
    C = len(factors)
    x, e = synth_input("cx", (B, C, H, W), seed), synth_input("ce", (B, C, H, W), seed + 1)
    d = synth_input("cd", (B, C, H, W), seed + 2)
    values = CR.block_mean(synth_input("cv", (B, C, H, W), seed + 3, uniform=True) * 2 - 1, factors)
    cells = (synth_input("cm", (B, C, H // 24, W // 24), seed + 4, uniform=True) > 0.4).float()
    mask = cells.repeat_interleave(24, 2).repeat_interleave(24, 3) if masked else None
    return x, e, d, values, mask


@pytest.mark.parametrize("factors", [(2, 3, 4), (6, 8, 1)])
def test_emulated_steps_project_to_three_eps(factors):
    """the residual of the fp32 steps: max |A pred_x0 - values| on observed blocks <= 3 eps * max(1, |p0|max) -- the figure the GPU test
    measures the kernels against -- and pred_x0 is the float64 projection of the plain step's prediction to fp32 rounding"""
    x, e, d, values, mask = _case32(factors)
    a_s, s1m, c = 0.37, float(np.sqrt(np.float32(1.0) - np.float32(0.37))), (0.8, 0.3, 1.4, -0.4)
    for name, (xn, p0c), plain in (
            ("ddim", CR.ddim_step(x, e, d, a_s, 0.61, 0.2, s1m, 1.0, values, factors, mask), DR.step(x, e, None, a_s, s1m, *c, False)[1]),
            ("dpm", CR.dpm_step(x, e, d, a_s, s1m, *c, True, values, factors, mask), DR.step(x, e, d, a_s, s1m, *c, True)[1])):
        scale = max(1.0, float(plain.abs().max()))
        res = (CR.block_mean(p0c, factors) - values).abs()[mask == 1].max()
        res64 = np.abs(CR.block_mean64(p0c.numpy(), factors) - values.numpy())[mask.numpy() == 1].max()
        print(f"{name} {factors}: residual {float(res) / EPS:.2f} eps (float64 mean: {res64 / EPS:.2f} eps), |p0|max {scale:.2f}")
        assert float(res) <= 3 * EPS * scale and res64 <= 3 * EPS * scale
        want = CR.project64(plain.numpy(), values.numpy(), factors, mask.numpy())
        assert np.abs(p0c.numpy() - want).max() <= 8 * 64 * EPS * scale      # (a sequential sum of up to 64 terms)
        assert torch.isfinite(xn).all()


@pytest.mark.parametrize("how", ["weight", "mask"])
def test_emulated_steps_with_nothing_observed_are_the_plain_steps(how):
    from oracle import sampler_ref as SR
    factors = (1, 2, 8)
    x, e, d, values, mask = _case32(factors)
    lam, mask = (0.0, mask) if how == "weight" else (1.0, torch.zeros_like(mask))
    a_s, a_prev, sigma = 0.37, 0.61, 0.2
    s1m, c = float(np.sqrt(np.float32(1.0) - np.float32(a_s))), (0.8, 0.3, 1.4, -0.4)
    for clip in (False, True):
        got = CR.dpm_step(x, e, d, a_s, s1m, *c, clip, values, factors, mask, lam)
        want = DR.step(x, e, d, a_s, s1m, *c, clip)
        assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
    got = CR.ddim_step(x, e, d, a_s, a_prev, sigma, s1m, 1.0, values, factors, mask, lam)
    want = SR.ddim_step(x, e, a_s, a_prev, sigma, s1m, d, 1.0)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
