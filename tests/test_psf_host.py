"""CPU: PSF-aware observations (diffusion/consistency.py PsfObservation / gaussian_psf / psf_observe / bind, tests/psf_ref.py): every refusal
that needs no GPU; the Gaussian taps; the float64 operator, its adjoint, its norm against the step size and the Landweber iteration; the
float64 DDIM loop on the Gaussian toy with a PSF link; the fp32 emulation's identities; the kernels' bodies compiled for the host and run
under the address and undefined-behaviour sanitizers as a stand-alone program."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, SpectralObservation, bind, gaussian_psf, psf_observe
from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
from tests import consistency_ref as CR
from tests import dpm_ref as DR
from tests import psf_ref as PR
from tests import spectral_ref as XR
from tests.helpers import bits_equal
from tests.synth import synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = XR.EPS
FACTORS = (1, 2, 3, 4, 6, 8)
MTFS = (0.1, 0.3, 0.6)


def _v(*shape):
    return torch.zeros(*shape)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw", [
    dict(psf=[[0.25, 0.5, 0.25]]),                                      # not 1-D
    dict(psf=[]), dict(psf=[0.5, 0.5]),                                 # an even number of taps
    dict(psf=np.full(27, 1 / 27)),                                      # r = 13
    dict(psf="gauss"), dict(psf=[True]), dict(psf=np.ones(3, np.complex64)),
    dict(psf=[0.25, float("nan"), 0.25]), dict(psf=[float("inf")]), dict(psf=[1e300]),
    dict(psf=[-0.1, 1.2, -0.1]), dict(psf=[-0.0, 1.0, -0.0]),           # negative, and a negative zero
    dict(psf=[0.2, 0.5, 0.3]),                                          # not symmetric
    dict(psf=[0.3, 0.4, np.nextafter(np.float32(0.3), np.float32(1))]), # ... by one bit
    dict(psf=[0.5, 0.0, 0.5]),                                          # centre tap 0
    dict(factor=0), dict(factor=9), dict(factor=2.0), dict(factor=True), dict(factor=None),
    dict(channels=[]), dict(channels=[0, 0]), dict(channels=[2, 1]), dict(channels=[-1, 1]), dict(channels=[0, 32]), dict(channels=[0.0, 1.0]),
    dict(channels=[True, 2]), dict(channels=3), dict(channels=[0, 1, 2]),                     # three channels, two bands of values
    dict(channels=list(range(33))),
    dict(values=_v(2, 3, 4)), dict(values=torch.zeros(1, 2, 3, 4, dtype=torch.float64)), dict(values=_v(1, 33, 3, 4)), dict(values=_v(1, 0, 3, 4)),
    dict(mask=_v(1, 3, 3, 4)), dict(mask=_v(1, 1, 4, 4)), dict(mask=_v(1, 2, 12, 16)),           # (a full-resolution mask: the mask is coarse)
    dict(mask=torch.zeros(1, 1, 3, 4, dtype=torch.float64)), dict(values=_v(2, 2, 3, 4), mask=_v(3, 1, 3, 4)),
    dict(weight=-0.1), dict(weight=1.5), dict(weight=float("nan")), dict(weight=[0.5, "a"]), dict(weight=None), dict(weight=True),
    dict(iters=0), dict(iters=9), dict(iters=1.0), dict(iters=True), dict(iters=None),
])
def test_psf_observation_refuses(kw):
    args = dict(values=_v(1, 2, 3, 4), psf=[0.25, 0.5, 0.25], factor=4, channels=[0, 2], mask=None, weight=1.0, iters=1)
    args.update(kw)
    with pytest.raises(EodError):
        PsfObservation(**args)


def test_what_is_accepted():
    o = PsfObservation(_v(1, 2, 3, 4), [0.25, 0.5, 0.25], 4, [0, 2], _v(1, 1, 3, 4), [0.0, 1.0], 8)
    assert o.taps.dtype == np.float32 and o.taps.tolist() == [0.25, 0.5, 0.25] and o.per_evaluation and o.iters == 8
    PsfObservation(_v(2, 3, 3, 4), torch.tensor([1.0]), 1)                                   # a tensor, r = 0, all channels
    PsfObservation(_v(1, 1, 3, 4), [1, 2, 1], 8, (31,), _v(1, 1, 3, 4))                      # integers; any sum (N renormalises)
    PsfObservation(_v(1, 2, 3, 4), [0.1, 0.8, 0.1], 2, mask=_v(2, 2, 3, 4))
    PsfObservation(_v(1, 2, 3, 4), [0.0, 1.0, 0.0], 2)                                       # zero side taps
    PsfObservation(_v(1, 2, 3, 4), np.full(25, 0.04), 2)                                     # r = 12
    for f in range(1, 9):
        PsfObservation(_v(1, 2, 3, 4), gaussian_psf(f), f)


@pytest.mark.parametrize("shape,n_eval", [
    ((2, 2, 12, 16), 3),           # channel 2 of a state with 2
    ((2, 33, 12, 16), 3),          # C > 32
    ((2, 3, 12, 12), 3), ((2, 3, 16, 16), 3), ((2, 3, 6, 8), 3),      # the coarse grid times f is not the state
    ((3, 3, 12, 16), 3),           # leading dimension 2 of values
    ((2, 3, 12, 16), 4),           # three weights
])
def test_bind_refuses_what_does_not_fit_the_call(shape, n_eval):
    o = PsfObservation(_v(2, 2, 3, 4), [0.25, 0.5, 0.25], 4, [0, 2], _v(1, 1, 3, 4), [1.0, 0.5, 0.25])
    with pytest.raises(EodError):
        bind(o, "call", shape, n_eval, "cpu")
    with pytest.raises(EodError):
        bind([o], "call", shape, n_eval, "cpu")
    if shape[1] <= 32:
        ok = Observation(_v(1, shape[1], *shape[2:]), (1,) * shape[1])
        with pytest.raises(EodError):
            bind([ok, o], "call", shape, n_eval, "cpu")


def test_bind_without_channels_takes_c_from_values():
    o = PsfObservation(_v(1, 3, 3, 4), [1.0], 4)
    assert bind(o, "call", (2, 3, 12, 16), 2, "cpu").links[0].channels == (0, 1, 2)
    with pytest.raises(EodError):
        bind(o, "call", (2, 4, 12, 16), 2, "cpu")


def test_bind_takes_the_new_kind_alone_and_anywhere_in_a_list():
    shape = (2, 3, 12, 16)
    ps = PsfObservation(_v(1, 2, 3, 4), gaussian_psf(4), 4, [0, 2], iters=3)
    s = SpectralObservation(_v(1, 1, 12, 16), [[0.2, 0.5, 0.3]])
    o = Observation(_v(2, 3, 12, 16), (4, 4, 2))
    for form in (ps, [ps], (ps,)):
        one = bind(form, "call", shape, 3, "cpu")
        assert isinstance(one, CO.BoundChain) and [type(link) for link in one.links] == [CO.BoundPsf]        # alone: the unfused ends
    link = one.links[0]
    assert link.weights == [1.0] * 3 and link.iters == 3 and link.K == 2 and link.r == 6
    assert link.step == float(np.float32(PR.tau64(gaussian_psf(4), 4, 12, 16) / 16))
    for chain in ([ps, s], [s, ps], [o, ps, s, ps]):
        b = bind(chain, "call", shape, 3, "cpu")
        assert isinstance(b, CO.BoundChain)
        assert [type(link) for link in b.links] == [{PsfObservation: CO.BoundPsf, SpectralObservation: CO.BoundSpectral,
                                                     Observation: CO.BoundObservation}[type(z)] for z in chain]
    assert isinstance(bind([s], "call", shape, 3, "cpu"), CO.BoundSpectral) and isinstance(bind(o, "call", shape, 3, "cpu"), CO.BoundObservation)
    assert CO.MAX_LINKS == 4
    for bad in ([ps] * 5, [ps, None], [ps, "o"]):
        with pytest.raises(EodError):
            bind(bad, "call", shape, 3, "cpu")


def test_helpers_refuse_on_the_host():
    x = _v(1, 3, 12, 12)
    for kw in (dict(psf=[0.2, 0.5, 0.3], factor=2), dict(psf=[1.0], factor=5), dict(psf=[1.0], factor=0), dict(psf=[1.0], factor=2, channels=[3]),
               dict(psf=[1.0], factor=2, channels=[1, 0]), dict(psf=[[1.0]], factor=2)):
        with pytest.raises(EodError):
            psf_observe(x, **kw)
    with pytest.raises(EodError):
        psf_observe(x.numpy(), [1.0], 2)
    with pytest.raises(EodError):
        psf_observe(_v(1, 33, 12, 12), [1.0], 2)
    with pytest.raises(EodError):                                                                    # (a CPU tensor: the kernel is mandatory)
        psf_observe(x, [1.0], 2)
    for kw in (dict(factor=0), dict(factor=9), dict(factor=2.5), dict(factor=4, mtf_nyquist=0.0), dict(factor=4, mtf_nyquist=1.5),
               dict(factor=4, mtf_nyquist=float("nan")), dict(factor=4, mtf_nyquist="a"), dict(factor=4, radius=13), dict(factor=4, radius=-1),
               dict(factor=4, radius=2.0)):
        with pytest.raises(EodError):
            gaussian_psf(**kw)


def test_the_dropin_path_re_exports_the_new_names():
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    assert D.PsfObservation is PsfObservation and D.psf_observe is psf_observe and D.gaussian_psf is gaussian_psf


# ------------------------------------------------------------------------------------------------ the Gaussian taps
@pytest.mark.parametrize("f", range(1, 9))
@pytest.mark.parametrize("mtf", MTFS)
def test_gaussian_psf(f, mtf):
    h = gaussian_psf(f, mtf)
    sigma = CO.gaussian_sigma(f, mtf)
    r = h.size // 2
    assert h.dtype == np.float32 and r == min(math.ceil(3 * sigma), 12) and np.array_equal(h, PR.gaussian(f, mtf))
    assert h.view(np.uint32).tolist() == h[::-1].view(np.uint32).tolist() and (h > 0).all() and h.argmax() == r
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 2 * EPS
    nu = 1.0 / (2 * f)                                                                             # the coarse grid's Nyquist frequency
    assert abs(math.exp(-2.0 * math.pi ** 2 * sigma ** 2 * nu ** 2) - mtf) <= 1e-12                # the untruncated Gaussian's MTF there
    if f >= 2 and 3 * sigma <= 12:                                  # not truncated early, no aliasing at that frequency: the taps' own MTF, too
        k = np.arange(-r, r + 1)
        assert abs(float((h.astype(np.float64) * np.cos(2 * math.pi * nu * k)).sum()) - mtf) <= 0.02
    assert gaussian_psf(f, mtf, radius=2).size == 5 and gaussian_psf(f, 1.0).tolist() == [1.0]


# ------------------------------------------------------------------------------------------------ float64
ADJOINT_CASES = [(1, 0, 6, 7), (2, 3, 12, 28), (3, 5, 12, 18), (4, 6, 32, 32), (6, 9, 6, 6), (6, 9, 24, 30), (8, 12, 16, 16), (8, 12, 8, 40)]


def _taps(f, r, mtf=0.3):
    return PR.gaussian(f, mtf, radius=r)


@pytest.mark.parametrize("f,r,H,W", ADJOINT_CASES)
def test_adjoint_identity_and_constants(f, r, H, W):
    rng = np.random.default_rng(f * 100 + r)
    h = _taps(f, r)
    p, q = rng.standard_normal((2, 3, H, W)), rng.standard_normal((2, 3, H // f, W // f))
    lhs, rhs = float((PR.apply64(p, h, f) * q).sum()), float((p * PR.adjoint64(q, h, f, H, W)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    # A^T by the formula of the contract: B0((replicate(q) / f^2) / n), B0 symmetric
    Ly, ny = PR.line64(h, H, 1)
    Lx, nx = PR.line64(h, W, 1)
    B0y, B0x = Ly * ny[:, None], Lx * nx[:, None]
    assert np.abs(B0y - B0y.T).max() <= 1e-16 and np.abs(B0x - B0x.T).max() <= 1e-16
    w = np.repeat(np.repeat(q, f, 2), f, 3) / (f * f) / (ny[:, None] * nx[None, :])
    assert np.abs(np.einsum("yh,bkyx,xw->bkhw", B0y, w, B0x) - PR.adjoint64(q, h, f, H, W)).max() <= 1e-13
    assert np.abs(PR.apply64(np.full((1, 2, H, W), 0.625), h, f) - 0.625).max() <= 1e-13        # (a few hundred float64 terms per pixel)


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("mtf", MTFS)
def test_step_size_bounds_the_operator_norm(f, mtf):
    """power iteration on A^T A (the separable operator: the product of the two 1-D norms): ||A||^2 <= 1 / tau with the product's tau"""
    h = PR.gaussian(f, mtf)
    for H, W in ((6 * f, 4 * f), (2 * f, 9 * f), (f, f)):
        tau = CO.psf_tau(h, f, H, W)
        assert abs(tau - PR.tau64(h, f, H, W)) <= 1e-13 * tau
        norm2 = 1.0
        for L in (H, W):
            A1 = PR.line64(h, L, f)[0]
            v = np.ones(L)
            for _ in range(300):
                v = A1.T @ (A1 @ v)
                v /= np.linalg.norm(v)
            norm2 *= float(v @ (A1.T @ (A1 @ v)))
            assert 1.0 - 1e-14 <= PR.cmax64(h, L) <= 1.16
        assert norm2 <= (1.0 / tau) * (1 + 1e-12)
        assert norm2 * tau >= 1.0 / 1.16 ** 2 - 1e-9                                 # ||A1||^2 >= 1 / f (constants) and cmax <= 1.16: the step is not needlessly small


def test_landweber_residual_never_increases_and_falls_as_the_prototype_does():
    """consistent data at f = 4, MTF 0.3, 32 x 32: the residual ||A p - y|| is monotone over 50 steps and after 8 steps at most 1.5 x the 0.16 of
    its start that the numpy prototype of the issue measured"""
    rng = np.random.default_rng(11)
    f, H, W = 4, 32, 32
    h = PR.gaussian(f, 0.3)
    y = PR.apply64(rng.uniform(-1, 1, (1, 2, H, W)), h, f)
    p = rng.standard_normal((1, 2, H, W))
    res = [float(np.linalg.norm(PR.apply64(p, h, f) - y))]
    for _ in range(50):
        p = PR.landweber64(p, y, h, f, tau=CO.psf_tau(h, f, H, W))
        res.append(float(np.linalg.norm(PR.apply64(p, h, f) - y)))
    print("residual / start after 1, 8, 25, 50 steps:", [round(res[k] / res[0], 4) for k in (1, 8, 25, 50)])
    assert all(b <= a * (1 + 1e-12) for a, b in zip(res, res[1:]))
    assert res[8] <= 1.5 * 0.16 * res[0]
    # with a soft mask and lam < 1 it still never increases the masked objective's residual in the m-weighted sense: here just no growth of ||.||
    m = rng.random((1, 1, H // f, W // f))
    p2 = rng.standard_normal((1, 2, H, W))
    before = float(np.linalg.norm(np.sqrt(m) * (PR.apply64(p2, h, f) - y)))
    after = float(np.linalg.norm(np.sqrt(m) * (PR.apply64(PR.landweber64(p2, y, h, f, None, m, 0.7), h, f) - y)))
    assert after <= before


def test_identity_taps_are_the_block_mean_projector():
    rng = np.random.default_rng(3)
    for f in (1, 2, 3, 8):
        p, truth = rng.standard_normal((2, 3, 2 * f, 3 * f)), rng.uniform(-1, 1, (2, 3, 2 * f, 3 * f))
        assert PR.tau64([1.0], f, 2 * f, 3 * f) == f * f == CO.psf_tau([1.0], f, 2 * f, 3 * f)
        y = PR.apply64(truth, [1.0], f)
        cells = (rng.random((2, 1, 2, 3)) > 0.4).astype(np.float64)
        got = PR.landweber64(p, y, [1.0], f, None, cells, 0.75)
        rep = lambda z: np.repeat(np.repeat(z, f, 2), f, 3)
        want = CR.project64(p, rep(y), (f,) * 3, rep(cells), 0.75)
        assert np.abs(got - want).max() <= 1e-14


def test_float64_ddim_loop_on_the_toy_with_a_psf_link():
    """section 9.4's Gaussian toy as a 4 x 32 x 32 image with a PSF link (f = 4, MTF 0.3, 4 Landweber steps per evaluation) after every
    prediction: the end state is closer to the observation than the unconstrained loop's; all weights 0: the unconstrained loop, bit for bit"""
    from oracle import schedule as SCH
    acp = SCH.eo_cosine_tables(1000)["alphas_cumprod"].numpy().astype(np.float64)
    levels = make_dpm_timesteps("uniform", 20, acp)
    truth = np.random.default_rng(5).uniform(-1, 1, CR.TOY_SHAPE)
    h = gaussian_psf(4)
    y = PR.apply64(truth, h, 4)
    dist = lambda z: float(np.linalg.norm(PR.apply64(z.reshape(CR.TOY_SHAPE), h, 4) - y))
    free, _, _ = XR.ddim_f64(acp, levels)
    assert np.array_equal(free, DR.ddim_f64(acp, levels))
    got = {}
    for iters in (1, 4):
        x, p0, _ = XR.ddim_f64(acp, levels, [PR.psf_link64(y, h, 4, iters=iters)])
        got[iters] = dist(x)
    print(f"||A x - y|| at the end: unconstrained {dist(free):.4f}, PSF link iters=1 {got[1]:.4f}, iters=4 {got[4]:.4f}")
    assert got[4] < got[1] < 0.5 * dist(free)
    zero, _, _ = XR.ddim_f64(acp, levels, [PR.psf_link64(y, h, 4, lam=0.0, iters=4)])
    assert np.array_equal(zero, free)


# ------------------------------------------------------------------------------------------------ the emulation
def _case32(f, r, H, W, B=2, C=3, channels=(0, 2)):
    h = _taps(f, r)
    p = synth_input("pp", (B, C, H, W), f + r)
    K = len(channels)
    values = synth_input("pv", (B, K, H // f, W // f), f + r + 1, uniform=True) * 2 - 1
    mask = synth_input("pm", (B, 1, H // f, W // f), f + r + 2, uniform=True)
    return h, p, values, mask


@pytest.mark.parametrize("f,r,H,W", ADJOINT_CASES)
def test_emulation_with_nothing_observed_returns_its_input(f, r, H, W):
    h, p, values, mask = _case32(f, r, H, W)
    assert bits_equal(PR.project(p, values, h, f, (0, 2), mask, 0.0, iters=2), p)
    assert bits_equal(PR.project(p, values, h, f, (0, 2), torch.zeros_like(mask), 1.0, iters=2), p)
    out = PR.project(p, values, h, f, (0, 2), mask, 1.0)
    assert bits_equal(out[:, 1], p[:, 1]) and not torch.equal(out[:, 0], p[:, 0])


@pytest.mark.parametrize("f", range(1, 9))
def test_emulation_with_identity_taps_is_the_block_mean_projection(f):
    h, p, values, mask = _case32(f, 0, 2 * f, 3 * f, channels=(0, 1, 2))
    assert h.tolist() == [1.0] and PR.step32(h, f, 2 * f, 3 * f) == 1.0
    rep = lambda z: z.repeat_interleave(f, 2).repeat_interleave(f, 3).contiguous()
    for m in (None, mask):
        got = PR.project(p, values, h, f, None, m, 0.625)
        assert bits_equal(got, CR.project(p, rep(values), (f,) * 3, None if m is None else rep(m), 0.625))


def test_emulation_follows_float64():
    for f, r, H, W in ADJOINT_CASES:
        h, p, values, mask = _case32(f, r, H, W)
        got = PR.project(p, values, h, f, (0, 2), mask, 0.75, iters=3)
        want = PR.landweber64(p.numpy(), values.numpy(), h, f, (0, 2), mask.numpy(), 0.75, iters=3)
        assert np.abs(got.numpy() - want).max() <= 64 * EPS * max(1.0, float(p.abs().max()))


# ------------------------------------------------------------------------------------------------ the kernels' bodies on the host
def test_kernel_bodies_run_clean_under_sanitizers_and_match_the_contract(tmp_path):
    """tests/psf_host_check.cc: csrc/psf_body.h compiled for the host with -fsanitize=address,undefined and run as a program of its own (nothing
    is loaded into this interpreter) over every f, r in {0, 1, 12}, both access forms, planes inside the halo and exactly sized buffers"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "psf_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "psf_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
