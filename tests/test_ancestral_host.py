"""CPU: observations on the ancestral samplers -- tests/ancestral_ref.py against oracle.sampler_ref and float64, the
float64 ancestral loop on the Gaussian toy, shard() of the three observation classes, every refusal that needs no launch, and the two kernel
bodies (csrc/ddpm_p0_body.h) compiled for the host and run under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, SpectralObservation
from oracle import sampler_ref as SR
from oracle import schedule as SCH
from tests import ancestral_ref as AR
from tests import consistency_ref as CR
from tests.helpers import bits_equal
from tests.synth import synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = AR.EPS


def _v(*shape):
    return torch.zeros(*shape)


def _xez(n, seed, shape=(3, 6, 7), scale=1.0):
    return tuple(synth_input(name, (n,) + shape, seed) * scale for name in ("ax", "ae", "az"))


# ------------------------------------------------------------------------------------------------ the emulation against the oracle
@pytest.mark.parametrize("T", [8, 1000])
def test_split_step_without_links_has_the_bits_of_the_clipped_ddpm_step(T):
    """every t of the schedule, t = 0 included (a batch of two at the same t); and a batch whose minimum is 0"""
    tb = SCH.eo_cosine_tables(T)
    x, e, z = _xez(2, T, scale=2.0)                                  # (|x0| beyond 1: the clamp acts)
    for i in range(T):
        t = torch.full((2,), i, dtype=torch.int64)
        got, p = AR.step(tb, x, e, z, t)
        assert bits_equal(got, SR.ddpm_step_clip(tb, x, t, z, e)), i
        assert float(p.abs().max()) <= 1.0
    x, e, z = _xez(3, T + 1, scale=2.0)
    for t in ([0, 3, 7], [5, 1, T - 1], [T - 1, T - 1, 0]):
        t = torch.tensor(t)
        assert bits_equal(AR.step(tb, x, e, z, t)[0], SR.ddpm_step_clip(tb, x, t, z, e))


def test_a_timestep_out_of_range_fills_its_sample_with_nan_and_leaves_the_others():
    tb = SCH.eo_cosine_tables(8)
    x, e, z = _xez(3, 3)
    for bad in (8, 11, -1):
        t = torch.tensor([5, bad, 3])
        got, p = AR.step(tb, x, e, z, t)
        assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(p[1]).all())
        if bad > 0:                                                  # (a negative member makes the batch minimum negative: the other branch)
            want = SR.ddpm_step_clip(tb, x[[0, 2]], t[[0, 2]], z[[0, 2]], e[[0, 2]])
            assert bits_equal(got[[0, 2]], want)
        else:
            assert bool(torch.isfinite(got[[0, 2]]).all())


# ------------------------------------------------------------------------------------------------ float64
def _exact_tables64(T):
    """float64 tables that satisfy alpha = 1 - beta and acp_t = alpha_t acp_{t-1} to float64 rounding (the fp32 buffers do to 1e-7 only)"""
    betas = SCH.eo_cosine_tables(T)["betas"].numpy().astype(np.float64)
    alphas = 1.0 - betas
    return dict(betas=betas, alphas=alphas, alphas_cumprod=np.cumprod(alphas))


@pytest.mark.parametrize("T", [8, 20])
def test_unclamped_posterior_form_is_the_epsilon_form_in_float64(T):
    """mean of q(x_{t-1} | x_t, x0(x_t, eps)) = (x_t - (1 - alpha) / sqrt(1 - acp) eps) / sqrt(alpha): 1e-12 at every t.  (T = 8 and the
    T = 20 of the whole-call tests: float64 forms 1 - acp_t with an absolute error of 1e-16, at t = 1 of T = 1000 a relative 1e-12 of both
    forms' coefficients, so there the two forms can differ by 1e-12 through rounding alone.)"""
    tb = _exact_tables64(T)
    rng = np.random.default_rng(T)
    x, e, z = (rng.standard_normal((2, 3, 6, 7)) for _ in range(3))
    worst = 0.0
    for i in range(T):
        a = AR.finish64(tb, x, AR.pred_x0_64(tb, x, e, i), z, i)
        b = AR.eps_form64(tb, x, e, z, i)
        worst = max(worst, float(np.abs(a - b).max()))
    print(f"T = {T}: posterior form vs epsilon form, max |difference| over all t = {worst:.3e}")
    assert worst <= 1e-12


def _bound(tb64, x, e, z, i, p0_64, out_64, used_64=None):
    """first-order bound of |fp32 emulation - float64| of (pred_x0, step) at timestep i > 0: every rounded operation contributes half an eps
    of its result's magnitude, carried to the output through the (linear) operations that follow.  Relative errors of the scalars, in units
    of eps: r = 1 / acp 1/2; c_x0 = sqrt(r) 1/4 + 1/2; rm = r - 1: (r / 2 + rm / 2) / rm, c_pred = sqrt(rm) half of that + 1/2; om = 1 - acp
    and omp = 1 - acp_prev 1/2 each; m_x0 = (beta * sqrt(acp_prev)) / om: 1/2 + 1/2 + 1/2 + 1/2; m_xt = (omp * sqrt(alpha)) / om: 5 / 2;
    std = sqrt((beta * omp) / om): (4 / 2) / 2 + 1/2.  used_64: the prediction the step uses when it is not p0_64 itself (the clamped one: the
    clamp is non-expansive, so the prediction's bound holds for it)."""
    used_64 = p0_64 if used_64 is None else used_64
    h = 0.5 * EPS
    acp, acp_prev = tb64["alphas_cumprod"][i], tb64["alphas_cumprod"][i - 1]
    b, a = tb64["betas"][i], tb64["alphas"][i]
    r = 1.0 / acp
    rm = r - 1.0
    c_x0, c_pred = np.sqrt(r), np.sqrt(rm)
    d_cx0 = c_x0 * 1.5 * h
    d_cpred = c_pred * (0.5 * (r + rm) / rm + 1.0) * h
    u, v = c_x0 * x, c_pred * e
    d_p0 = np.abs(x) * d_cx0 + h * np.abs(u) + np.abs(e) * d_cpred + h * np.abs(v) + h * np.abs(p0_64)
    om, omp = 1.0 - acp, 1.0 - acp_prev
    m_x0, m_xt, std = b * np.sqrt(acp_prev) / om, omp * np.sqrt(a) / om, np.sqrt(b * omp / om)
    p, q, sz = m_x0 * used_64, m_xt * x, std * z
    d_out = (m_x0 * d_p0 + np.abs(p) * (4 + 1) * h + np.abs(q) * (5 + 1) * h + h * np.abs(p + q) + np.abs(sz) * (3 + 1) * h + h * np.abs(out_64))
    return d_p0 * (1 + 64 * EPS), d_out * (1 + 64 * EPS)             # (second-order terms)


@pytest.mark.parametrize("T", [8, 1000])
def test_emulation_follows_float64(T):
    tb = SCH.eo_cosine_tables(T)
    tb64 = AR.tables64(tb)
    x, e, z = _xez(2, T + 5)
    x64, e64, z64 = (v.numpy().astype(np.float64) for v in (x, e, z))
    worst = 0.0
    for i in sorted({1, 2, 3, T // 2, T - 2, T - 1}):
        t = torch.full((2,), i, dtype=torch.int64)
        got, p = AR.step(tb, x, e, z, t, clip=False)
        p64 = AR.pred_x0_64(tb64, x64, e64, i)
        out64 = AR.finish64(tb64, x64, p64, z64, i)
        d_p0, d_out = _bound(tb64, x64, e64, z64, i, p64, out64)
        assert (np.abs(p.numpy() - p64) <= d_p0).all() and (np.abs(got.numpy() - out64) <= d_out).all(), i
        worst = max(worst, float((np.abs(got.numpy() - out64) / d_out).max()))
        gotc, pc = AR.step(tb, x, e, z, t, clip=True)                # (the clamp is non-expansive: the same bound)
        pc64 = AR.pred_x0_64(tb64, x64, e64, i, clip=True)
        outc64 = AR.finish64(tb64, x64, pc64, z64, i)
        d_outc = _bound(tb64, x64, e64, z64, i, p64, outc64, pc64)[1]
        assert (np.abs(pc.numpy() - pc64) <= d_p0).all() and (np.abs(gotc.numpy() - outc64) <= d_outc).all(), i
    print(f"T = {T}: largest |fp32 - float64| / bound = {worst:.3f}")
    # t = 0: out = (beta_0 / (1 - acp_0)) * p0c, one division and one product on top of the prediction
    t = torch.zeros(2, dtype=torch.int64)
    got, p = AR.step(tb, x, e, z, t, clip=False)
    p64 = AR.pred_x0_64(tb64, x64, e64, 0)
    assert np.abs(got.numpy() - AR.finish64(tb64, x64, p64, z64, 0)).max() <= float((np.abs(p.numpy() - p64) + 2 * EPS * np.abs(p64)).max())


# ------------------------------------------------------------------------------------------------ the float64 loop on the toy
def test_float64_ancestral_loop_on_the_toy():
    """section 9.4's Gaussian toy as a 4 x 32 x 32 image, factors (1, 2, 4, 8), T = 50, injected noises: with weight 1 the RETURNED sample has
    the observation's block means to 1e-12 (at t = 0 the posterior step returns the prediction); with weight 0 the loop is the unconstrained
    one bit for bit"""
    T = 50
    tb64 = AR.tables64(SCH.eo_cosine_tables(T))
    noises = np.random.default_rng(9).standard_normal((T,) + CR.TOY_SHAPE)
    truth = np.random.default_rng(5).uniform(-1, 1, CR.TOY_SHAPE)
    values = CR.block_mean64(truth, CR.TOY_FACTORS)
    free, _ = AR.ddpm_f64(tb64, noises)
    one, p0 = AR.ddpm_f64(tb64, noises, [lambda p: CR.project64(p, values, CR.TOY_FACTORS, None, 1.0)])
    miss = float(np.abs(CR.block_mean64(one.reshape(CR.TOY_SHAPE), CR.TOY_FACTORS) - values).max())
    miss_free = float(np.abs(CR.block_mean64(free.reshape(CR.TOY_SHAPE), CR.TOY_FACTORS) - values).max())
    print(f"max |block mean - values| of the returned sample: weight 1 {miss:.3e}, unconstrained {miss_free:.3e}")
    assert miss <= 1e-12 and miss_free > 0.1
    zero, _ = AR.ddpm_f64(tb64, noises, [lambda p: CR.project64(p, values, CR.TOY_FACTORS, None, 0.0)])
    assert np.array_equal(zero, free) and bool(np.isfinite(free).all())


# ------------------------------------------------------------------------------------------------ shard()
def _ramp(*shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)


def test_shard_of_the_three_classes():
    full = [Observation(_ramp(4, 3, 8, 8), (1, 2, 4), mask=_ramp(4, 1, 8, 8), weight=[1.0, 0.5]),
            SpectralObservation(_ramp(4, 2, 8, 8), [[.5, .5, 0], [0, .5, .5]], 2, mask=_ramp(4, 1, 8, 8), weight=0.25),
            PsfObservation(_ramp(4, 2, 2, 2), [0.25, 0.5, 0.25], 4, [0, 2], mask=_ramp(4, 2, 2, 2), iters=3)]
    for o in full:
        s = o.shard(4, 1, 3)
        assert type(s) is type(o) and s is not o
        assert torch.equal(s.values, o.values[1:3]) and torch.equal(s.mask, o.mask[1:3])
        assert s.weights == o.weights and s.per_evaluation == o.per_evaluation
        assert o.values.shape[0] == 4 and o.mask.shape[0] == 4                                    # (the original is left as it was)
        assert o.shard(4, 0, 4).values.shape[0] == 4 and o.shard(4, 2, 2).values.shape[0] == 0
        s.bind("call", (2, 3, 8, 8), 2, "cpu")                                                     # ... and fits the shard's call
    assert full[0].shard(4, 1, 3).factors == (1, 2, 4)
    assert full[1].shard(4, 1, 3).factor == 2 and np.array_equal(full[1].shard(4, 1, 3).pinv, full[1].pinv)
    assert full[2].shard(4, 1, 3).iters == 3 and full[2].shard(4, 1, 3).channels == (0, 2)
    # broadcast tensors are kept; a mix of the two
    bc = [Observation(_ramp(1, 3, 8, 8), (1, 2, 4), mask=_ramp(4, 3, 8, 8)), SpectralObservation(_ramp(4, 1, 8, 8), [[.2, .5, .3]], mask=_ramp(1, 1, 8, 8)),
          PsfObservation(_ramp(1, 3, 2, 2), [1.0], 4), Observation(_ramp(1, 3, 8, 8), (1, 1, 1))]
    for o in bc:
        s = o.shard(4, 3, 4)
        for name in ("values", "mask"):
            a, b = getattr(o, name), getattr(s, name)
            assert (a is None and b is None) or torch.equal(b, a if a.shape[0] == 1 else a[3:4])
    one = Observation(_ramp(1, 3, 8, 8), (1, 2, 4))
    assert torch.equal(one.shard(1, 0, 1).values, one.values) and one.shard(1, 0, 0).values.shape[0] == 0    # n_total = 1: cut like any size
    # lists: every link's shard; None stays None
    got = CO.shard(full, 4, 2, 4)
    assert isinstance(got, list) and [type(g) for g in got] == [type(o) for o in full]
    assert all(torch.equal(g.values, o.values[2:4]) for g, o in zip(got, full))
    assert CO.shard(None, 4, 0, 2) is None and torch.equal(CO.shard(full[0], 4, 0, 2).values, full[0].values[:2])
    assert isinstance(CO.shard(tuple(bc), 4, 0, 2), list)
    for bad in ((4, 3, 1), (4, -1, 2), (4, 0, 5), (0, 0, 0), (4, 0.0, 2), (4, True, 2), (5, 0, 2), (2, 0, 1)):
        with pytest.raises(EodError):
            full[0].shard(*bad)


# ------------------------------------------------------------------------------------------------ refusals without a launch
def _diffusion(T=20, s=16):
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")
    return EODiffusion(Never(), timesteps=T, image_size=s, in_channels=3, cond_type="sum")


def test_check_scene_args_refuses_what_sampling_scene_would():
    T, H, W = 20, 32, 48
    m = _diffusion(T)
    ok = Observation(_v(1, 3, H, W), (1, 2, 4))
    psf = lambda *shape, **kw: PsfObservation(_v(*shape), CO.gaussian_psf(4), 4, **kw)
    spec = lambda *shape, **kw: SpectralObservation(_v(*shape), [[.2, .5, .3]], **kw)
    cond = _v(1, 4, H, W)
    for kw in (dict(), dict(observation=[ok, psf(1, 3, H // 4, W // 4), spec(1, 1, H, W)]), dict(observation=Observation(_v(2, 3, H, W), (1, 2, 4)), n_scenes=2),
               dict(observation=Observation(_v(1, 3, H, W), (1, 2, 4), weight=[0.5] * T)),
               dict(observation=spec(1, 1, H, W, weight=[0.5] * 52), resample=(4, 3))):
        m.check_scene_args((H, W), "cuda", cond=cond, **kw)
    for kw in (dict(observation=ok, skip_known=True), dict(observation=[ok], skip_known=True),                 # skip_known with an observation
               dict(observation=Observation(_v(1, 4, H, W), (1, 2, 4, 1))), dict(observation=SpectralObservation(_v(1, 1, H, W), [[.5, .5]])),
               dict(observation=psf(1, 4, H // 4, W // 4)), dict(observation=psf(1, 2, H // 4, W // 4, channels=[1, 3])),   # a wrong channel count
               dict(observation=Observation(_v(2, 3, H, W), (1, 2, 4))), dict(observation=Observation(_v(3, 3, H, W), (1, 2, 4)), n_scenes=2),
               dict(observation=Observation(_v(1, 3, H, W), (1, 2, 4), mask=_v(2, 1, H, W))),                  # a wrong leading dimension
               dict(observation=psf(2, 3, H // 4, W // 4)), dict(observation=spec(3, 1, H, W), n_scenes=2),
               dict(observation=Observation(_v(1, 3, 16, 16), (1, 2, 4))), dict(observation=psf(1, 3, H, W)),    # not scene-sized
               dict(observation=Observation(_v(1, 3, H, W), (1, 2, 4), weight=[0.5] * (T + 1))),               # weights against the walk
               dict(observation=Observation(_v(1, 3, H, W), (1, 2, 4), weight=[0.5] * T), resample=(4, 3)),
               dict(observation=[ok, spec(1, 1, H, W, weight=[0.5] * 51)], resample=(4, 3)),
               dict(observation=[ok] * 5), dict(observation=[ok, None]), dict(observation="obs"), dict(observation=[])):
        with pytest.raises(EodError):
            m.check_scene_args((H, W), "cuda", cond=cond, **kw)


def test_check_copies_nothing_and_binds_nothing():
    o = Observation(_v(2, 3, 16, 16), (1, 2, 4))
    assert CO.check(o, "call", (2, 3, 16, 16), 5) is None and CO.check([o, o], "call", (2, 3, 16, 16), 5) is None and CO.check(None, "call", (2, 3, 16, 16), 5) is None
    assert CO.bind(o, "call", (2, 3, 16, 16), 5, None) is None
    with pytest.raises(EodError):
        CO.check(o, "call", (3, 3, 16, 16), 5)
    with pytest.raises(EodError):                                   # (no CPU path: the refusal of the call itself comes first)
        _diffusion().sampling(2, device="cpu", observation=o)


def test_the_dropin_path_re_exports_the_new_names():
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    assert D.ddpm_step is CO.ddpm_step and D.shard is CO.shard and D.check is CO.check


# ------------------------------------------------------------------------------------------------ the kernels' bodies on the host
def test_kernel_bodies_run_clean_under_sanitizers_and_match_the_contract(tmp_path):
    """tests/ancestral_host_check.cc: csrc/ddpm_p0_body.h compiled for the host with -fsanitize=address,undefined and run as a program of its
    own (nothing is loaded into this interpreter): both access forms, chw in {126, 768}, N in {1, 3}, mixed and out-of-range timesteps,
    exactly sized buffers"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ancestral_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "ancestral_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
