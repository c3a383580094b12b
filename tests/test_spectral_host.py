"""CPU: cross-band observations and chains (diffusion/consistency.py SpectralObservation / bind, tests/spectral_ref.py): every refusal that
needs no GPU; the float64 projector; the chain [pan at f = 1, bands at f = 4] on consistent data; the float64 DDIM loop on the Gaussian toy
with a chain; the fp32 emulation's residual."""
import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.consistency import Observation, SpectralObservation, bind, spectral_response
from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
from tests import consistency_ref as CR
from tests import dpm_ref as DR
from tests import spectral_ref as XR
from tests.helpers import bits_equal
from tests.synth import synth_input

EPS = XR.EPS
PAN4 = np.array([[0.3, 0.4, 0.2, 0.1]])
# (K, C, f, seed) of the matrices the emulation's residual is measured for: the GPU cases' matrices
MATRICES = [(1, 1, 1, 1), (1, 4, 1, 2), (3, 13, 1, 3), (8, 32, 1, 4), (1, 2, 4, 5), (8, 13, 2, 6), (3, 3, 3, 0), (4, 7, 5, 7), (2, 13, 6, 8),
            (2, 5, 8, 9)]


def _v(*shape):
    return torch.zeros(*shape)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw", [
    dict(response=np.ones((2, 3, 1))),                                  # not [K, C]
    dict(response=np.ones(3)),
    dict(response=np.zeros((0, 3))),
    dict(response="pan"),
    dict(response=[[True, False, True]]),                               # dtype
    dict(response=np.ones((1, 3), np.complex64)),
    dict(response=np.random.default_rng(0).random((9, 12)), values=_v(1, 9, 12, 12)),      # K > 8
    dict(response=np.random.default_rng(0).random((4, 3)), values=_v(1, 4, 12, 12)),       # K > C
    dict(response=np.random.default_rng(0).random((1, 33))),            # C > 32
    dict(response=[[0.5, float("nan"), 0.5]]),
    dict(response=[[0.5, float("inf"), 0.5]]),
    dict(response=[[1e300, 0.0, 0.0]]),                                 # not finite as float32
    dict(response=[[0.5, 0.5, 0.0], [0.5, 0.5, 0.0]], values=_v(1, 2, 12, 12)),            # rank 1
    dict(response=[[0.5, 0.5, 0.0], [0.5, 0.5004, 0.0]], values=_v(1, 2, 12, 12)),         # sigma_min / sigma_max about 3e-4
    dict(response=[[0.0, 0.0, 0.0]]),
    dict(values=_v(1, 2, 12, 12)),                                      # one row, two bands of values
    dict(values=_v(1, 12, 12)),
    dict(values=torch.zeros(1, 1, 12, 12, dtype=torch.float64)),
    dict(factor=0), dict(factor=9), dict(factor=2.0), dict(factor=True), dict(factor=5),                       # 5 does not divide 12
    dict(mask=_v(1, 3, 12, 12)),                                        # one mask for all rows
    dict(mask=_v(1, 1, 12, 16)),
    dict(mask=torch.zeros(1, 1, 12, 12, dtype=torch.float64)),
    dict(values=_v(2, 1, 12, 12), mask=_v(3, 1, 12, 12)),
    dict(weight=-0.1), dict(weight=1.5), dict(weight=float("nan")), dict(weight=[0.5, "a"]), dict(weight=None), dict(weight=True),
])
def test_spectral_observation_refuses(kw):
    args = dict(values=_v(1, 1, 12, 12), response=[[0.2, 0.5, 0.3]], factor=1, mask=None, weight=1.0)
    args.update(kw)
    with pytest.raises(EodError):
        SpectralObservation(**args)


def test_what_is_accepted_and_the_pseudo_inverse():
    o = SpectralObservation(_v(1, 1, 12, 12), [[0.2, 0.5, 0.3]], 4, _v(1, 1, 12, 12), [0.0, 1.0])
    assert o.response.dtype == np.float32 and o.pinv.shape == (3, 1) and o.pinv.dtype == np.float32 and o.per_evaluation
    assert np.array_equal(o.pinv, XR.pinv32(o.response))
    SpectralObservation(_v(2, 3, 12, 12), torch.tensor(XR.R3), 3)                                    # a tensor, a square matrix
    SpectralObservation(_v(1, 2, 12, 12), [[1, 0, 0], [0, 0, 1]], 6)                                # integers
    border = np.array([[1.0, 0.0], [0.0, 1.0e-3]])                                                  # right at the threshold
    assert XR.rcond(border) >= 1e-3
    SpectralObservation(_v(1, 2, 12, 12), border)
    for K, C, f, seed in MATRICES:
        assert XR.rcond(XR.response(K, C, seed)) >= XR.MIN_RCOND
        SpectralObservation(_v(1, K, 2 * f, 2 * f), XR.response(K, C, seed), f)


@pytest.mark.parametrize("shape,n_eval", [((2, 4, 12, 16), 3), ((2, 3, 16, 16), 3), ((3, 3, 12, 16), 3), ((2, 3, 12, 16), 4)])
def test_bind_refuses_what_does_not_fit_the_call(shape, n_eval):
    o = SpectralObservation(_v(2, 1, 12, 16), [[0.2, 0.5, 0.3]], 2, _v(1, 1, 12, 16), [1.0, 0.5, 0.25])
    with pytest.raises(EodError):
        bind(o, "call", shape, n_eval, "cpu")
    with pytest.raises(EodError):
        bind([o], "call", shape, n_eval, "cpu")
    ok = Observation(_v(1, shape[1], *shape[2:]), (1,) * shape[1])
    with pytest.raises(EodError):
        bind([ok, o], "call", shape, n_eval, "cpu")


def test_bind_takes_one_object_or_a_list_of_one_to_four():
    from eo_diffusion_amd.diffusion.consistency import BoundChain, BoundObservation, BoundSpectral
    shape = (2, 3, 12, 16)
    s = SpectralObservation(_v(1, 1, 12, 16), [[0.2, 0.5, 0.3]])
    o = Observation(_v(2, 3, 12, 16), (4, 4, 2))
    assert bind(None, "call", shape, 3, "cpu") is None
    assert isinstance(bind(o, "call", shape, 3, "cpu"), BoundObservation) and isinstance(bind(s, "call", shape, 3, "cpu"), BoundSpectral)
    assert isinstance(bind([s], "call", shape, 3, "cpu"), BoundSpectral) and isinstance(bind((o,), "call", shape, 3, "cpu"), BoundObservation)
    chain = bind([s, o, s, o], "call", shape, 3, "cpu")
    assert isinstance(chain, BoundChain) and [type(link) for link in chain.links] == [BoundSpectral, BoundObservation] * 2
    assert chain.links[0].weights == [1.0] * 3
    for bad in ([], [s] * 5, [s, None], [s, "o"], "so", 3, {"a": s}, [[s]]):
        with pytest.raises(EodError):
            bind(bad, "call", shape, 3, "cpu")


def test_spectral_response_refuses_on_the_host():
    x = _v(1, 3, 12, 12)
    for kw in (dict(response=[[1.0, 0.0]]), dict(response=[[0.2, 0.5, 0.3]], factor=5), dict(response=[[0.2, 0.5, 0.3]], factor=0),
               dict(response=np.ones((4, 3))), dict(response=[[0.2, float("nan"), 0.3]])):
        with pytest.raises(EodError):
            spectral_response(x, **kw)
    with pytest.raises(EodError):
        spectral_response(x.numpy(), [[0.2, 0.5, 0.3]])
    with pytest.raises(EodError):                                                                    # (a CPU tensor: the kernel is mandatory)
        spectral_response(x, [[0.2, 0.5, 0.3]])


def test_the_dropin_path_re_exports_the_new_names():
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    assert D.SpectralObservation is SpectralObservation and D.spectral_response is spectral_response


# ------------------------------------------------------------------------------------------------ float64
def _blocks(mask_cells, L):
    return np.repeat(np.repeat(mask_cells, L, 2), L, 3)


@pytest.mark.parametrize("K,C,f,seed", MATRICES)
def test_projector_is_idempotent_and_meets_the_observation_on_observed_blocks(K, C, f, seed):
    rng = np.random.default_rng(seed)
    R = XR.response(K, C, seed).astype(np.float64)
    assert XR.rcond(R) >= XR.MIN_RCOND
    B, H, W = 2, 4 * f, 6 * f
    p = rng.standard_normal((B, C, H, W))
    values = XR.apply64(rng.uniform(-1, 1, (B, C, H, W)), R, f)
    mask = _blocks((rng.random((B, 1, 4, 6)) > 0.4).astype(np.float64), f)
    assert 0.0 < mask.mean() < 1.0
    q = XR.project64(p, values, R, f, mask)
    on = np.broadcast_to(mask == 1, values.shape)
    scale = max(1.0, np.abs(p).max()) / XR.rcond(R)
    assert np.abs(XR.apply64(q, R, f) - values)[on].max() <= 1e-13 * scale                    # A (P x) = y on observed blocks
    assert np.array_equal(q[np.broadcast_to(mask == 0, q.shape)], p[np.broadcast_to(mask == 0, p.shape)])   # a free block is left alone
    assert np.abs(XR.project64(q, values, R, f, mask) - q).max() <= 1e-13 * scale             # idempotent
    assert np.array_equal(XR.project64(p, values, R, f, mask, 0.0), p)
    # what the projection changes lies in the row space of R, block-constant: the block means move by G r, the rest of p is untouched
    dq = q - p
    assert np.abs(dq - CR.block_mean64(dq, (f,) * C)).max() <= 1e-13 * scale


@pytest.mark.parametrize("order", ["pan first", "bands first"])
def test_pan_and_coarse_bands_commute_on_consistent_data(order):
    """the chain [pan at f = 1, bands at f = 4] on observations made from ONE truth image: after one pass in either order both constraint
    sets hold at once, to 1e-12 (the two orthogonal projections commute there)"""
    rng = np.random.default_rng(21)
    B, C, H, W = 2, 4, 16, 24
    truth = rng.uniform(-1, 1, (B, C, H, W))
    pan = XR.apply64(truth, PAN4, 1)
    bands = CR.block_mean64(truth, (4,) * C)
    p = 3.0 * rng.standard_normal((B, C, H, W))
    links = [lambda z: XR.project64(z, pan, PAN4, 1), lambda z: CR.project64(z, bands, (4,) * C)]
    for link in (links if order == "pan first" else links[::-1]):
        p = link(p)
    assert np.abs(XR.apply64(p, PAN4, 1) - pan).max() <= 1e-12
    assert np.abs(CR.block_mean64(p, (4,) * C) - bands).max() <= 1e-12
    assert np.abs(p - truth).max() > 0.1                                    # (the null space is untouched: this is not the truth)


def test_float64_ddim_loop_on_the_toy_with_a_chain_ends_on_both_observations():
    """section 9.4's Gaussian toy as a 4 x 32 x 32 image, the chain [pan at f = 1, bands at f = 4] from one truth image after every
    prediction: the last prediction meets both observations; with all weights 0 the loop is the unconstrained one, bit for bit"""
    from oracle import schedule as SCH
    acp = SCH.eo_cosine_tables(1000)["alphas_cumprod"].numpy().astype(np.float64)
    levels = make_dpm_timesteps("uniform", 20, acp)
    truth = np.random.default_rng(5).uniform(-1, 1, CR.TOY_SHAPE)
    pan, bands, f4 = XR.apply64(truth, PAN4, 1), CR.block_mean64(truth, (4,) * 4), (4,) * 4
    chain = lambda lam: [lambda z: XR.project64(z, pan, PAN4, 1, None, lam), lambda z: CR.project64(z, bands, f4, None, lam)]
    x, p0, e = XR.ddim_f64(acp, levels, chain(1.0))
    free, _, _ = XR.ddim_f64(acp, levels)
    assert np.array_equal(free, DR.ddim_f64(acp, levels))
    p0 = p0.reshape(CR.TOY_SHAPE)
    assert np.abs(XR.apply64(p0, PAN4, 1) - pan).max() <= 1e-12 and np.abs(CR.block_mean64(p0, f4) - bands).max() <= 1e-12
    last = (1.0 - np.sqrt(acp[0])) * 1.0 + np.sqrt(1.0 - acp[0]) * np.abs(e).max()           # what the last step adds; |pan|, |bands| <= 1
    assert last < 0.1
    xs = x.reshape(CR.TOY_SHAPE)
    assert np.abs(XR.apply64(xs, PAN4, 1) - pan).max() <= last and np.abs(CR.block_mean64(xs, f4) - bands).max() <= last
    fr = free.reshape(CR.TOY_SHAPE)
    assert np.abs(XR.apply64(fr, PAN4, 1) - pan).max() > 0.3 and np.abs(CR.block_mean64(fr, f4) - bands).max() > 0.3
    zero, _, _ = XR.ddim_f64(acp, levels, chain(0.0))
    assert np.array_equal(zero, free)


# ------------------------------------------------------------------------------------------------ the emulation
def _case32(K, C, f, seed, B=2, masked=True):
    H, W = 4 * f, 6 * f
    R = XR.response(K, C, seed)
    shape = (B, C, H, W)
    x, e, d = synth_input("hx", shape, seed), synth_input("he", shape, seed + 1), synth_input("hd", shape, seed + 2)
    values = XR.apply(synth_input("hv", shape, seed + 3, uniform=True) * 2 - 1, R, f)
    mask = None
    if masked:
        cells = (synth_input("hm", (B, 1, 4, 6), seed + 4, uniform=True) > 0.4).float()
        mask = cells.repeat_interleave(f, 2).repeat_interleave(f, 3).contiguous()
    return R, x, e, d, values, mask


@pytest.mark.parametrize("K,C,f,seed", MATRICES)
def test_emulated_steps_project_to_three_eps(K, C, f, seed):
    """max |A p0c - y| over the observed blocks <= 3 eps * max(1, |p0|max), A in the emulation's own arithmetic.  Measured on the CPU for these
    matrices (cond(R) <= 15.0; the fixed 3 x 3: 3.4): at most 0.54 of that unit for ddim (|p0|max 4 .. 9) and 1.50 for dpm (clamped, |p0|max 1);
    the fixed 3 x 3 measures 0.24 and 0.62, so it needs no wider gate."""
    R, x, e, d, values, mask = _case32(K, C, f, seed)
    assert XR.rcond(R) >= XR.MIN_RCOND
    a, s1m = 0.37, float(np.sqrt(np.float32(1) - np.float32(0.37)))
    c = (0.8, 0.3, 1.4, -0.4)
    on = None if mask is None else (mask == 1).expand(-1, K, -1, -1)
    for name, (_, p0c), plain in (("ddim", XR.ddim_step(x, e, None, a, 0.61, 0.0, s1m, 1.0, [XR.spec_link(values, R, f, mask)]), XR.pred_x0(x, e, a, s1m)),
                                  ("dpm", XR.dpm_step(x, e, d, a, s1m, *c, True, [XR.spec_link(values, R, f, mask)]), XR.pred_x0(x, e, a, s1m, True))):
        res = float((XR.apply(p0c, R, f) - values).abs()[on].max())
        scale = max(1.0, float(plain.abs().max()))
        print(f"{name} K={K} C={C} f={f}: cond {1 / XR.rcond(R):.1f}, residual {res / EPS / scale:.2f} eps * max(1, |p0|max = {scale:.2f})")
        assert res <= 3 * EPS * scale
        free = (mask == 0).expand(-1, C, -1, -1)
        assert bits_equal(p0c[free], plain[free])


@pytest.mark.parametrize("how", ["weight", "mask"])
def test_emulated_steps_with_nothing_observed_are_the_plain_steps(how):
    R, x, e, d, values, mask = _case32(4, 7, 5, 7)
    if how == "mask":
        mask = torch.zeros_like(mask)
    lam = 0.0 if how == "weight" else 1.0
    a, s1m = 0.37, float(np.sqrt(np.float32(1) - np.float32(0.37)))
    c = (0.8, 0.3, 1.4, -0.4)
    links = [XR.spec_link(values, R, 5, mask, lam), XR.obs_link(values[:, :1].expand(-1, 7, -1, -1), (5,) * 7, mask, lam)]
    got = XR.dpm_step(x, e, d, a, s1m, *c, True, links)
    want = DR.step(x, e, d, a, s1m, *c, True)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])


def test_identity_response_at_full_resolution_is_the_per_channel_observation():
    """R = I, f = 1: d = mean = p0, t = r, so the cross-band emulation has the bits of section 9.5's with factors all 1"""
    R, x, e, d, _, mask = _case32(3, 3, 1, 0)
    I = np.eye(3, dtype=np.float32)
    assert np.array_equal(XR.pinv32(I), I)
    values = synth_input("iv", x.shape, 5, uniform=True) * 2 - 1
    p = XR.pred_x0(x, e, 0.37, 0.79)
    assert bits_equal(XR.project(p, values, I, I, 1, mask, 0.625), CR.project(p, values, (1, 1, 1), mask, 0.625))
