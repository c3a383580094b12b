"""CPU: cross-band PSF observations (PsfObservation(response=...), psf_observe(response=...), tests/spectral_psf_ref.py; DESIGN.md section
9.10): every new refusal; the factorised projection (fp32 emulation, per-plane solve) against a dense float64 solve on kron(R, A_H, A_W); the
Landweber step size against the dense operator's norm; nothing observed; the float64 DDIM loop on the Gaussian toy with a pan link; the
kernels' bodies compiled for the host and run under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, bind, gaussian_psf, psf_gram, psf_observe
from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
from tests import consistency_ref as CR
from tests import psf_cg_ref as GR
from tests import psf_ref as PR
from tests import spectral_psf_ref as SP
from tests import spectral_ref as XR
from tests.helpers import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAN4 = [[0.25, 0.35, 0.25, 0.15]]                                           # cond 1
R32 = [[0.66, 0.29, 0.05], [0.05, 0.29, 0.66]]                              # 3 -> 2, cond 1.34
R43 = [[0.4, 0.4, 0.2, 0.0], [0.1, 0.4, 0.4, 0.1], [0.0, 0.2, 0.4, 0.4]]    # 4 -> 3, cond 5.9
#         R     f  mtf  (H, W)    damping
TABLE = [(PAN4, 4, 0.6, (32, 32), 0.0),
         (R32, 2, 0.3, (24, 28), 0.0),
         (R43, 3, 0.3, (12, 18), 0.0),
         (PAN4, 4, 0.6, (32, 32), 0.05)]


def _v(*shape):
    return torch.zeros(*shape)


# ------------------------------------------------------------------------------------------------ refusals
H3 = [0.25, 0.5, 0.25]


@pytest.mark.parametrize("kw", [
    dict(channels=[0, 2]),                                                   # response with channels
    dict(channels=[0]),
    dict(values=_v(1, 2, 3, 4)), dict(values=_v(1, 3, 3, 4)),                # one band, two / three planes of values
    dict(response=R32, values=_v(1, 1, 3, 4)), dict(response=R32, values=_v(1, 3, 3, 4)),
    dict(response=R32, values=_v(1, 2, 3, 4), mask=_v(1, 2, 3, 4)),          # a per-band mask
    dict(response=R32, values=_v(1, 2, 3, 4), mask=_v(2, 2, 3, 4)),
    dict(response=[[0.5, 0.5, 0.0], [1.0, 1.0, 0.0]], values=_v(1, 2, 3, 4)),                    # rank-deficient
    dict(response=[[0.5, 0.5, 0.0], [0.5, 0.5, 1e-4]], values=_v(1, 2, 3, 4)),                   # below MIN_RCOND
    dict(response=[[0.0, 0.0, 0.0]]),
    dict(response=np.eye(9, 12), values=_v(1, 9, 3, 4)),                     # K = 9
    dict(response=np.full((1, 33), 1 / 33)),                                 # C = 33
    dict(response=np.eye(3)[:, :2], values=_v(1, 3, 3, 4)),                  # K > C
    dict(response=[0.3, 0.3, 0.4]), dict(response="pan"), dict(response=[[float("nan"), 0.5, 0.5]]), dict(response=[[True, False, True]]),
    dict(response=np.zeros((0, 3))),
    dict(solver="cg", mask=torch.full((1, 1, 3, 4), 0.5)),                   # the rules of the solver stay
    dict(damping=0.05), dict(iters=9),
])
def test_psf_observation_with_a_response_refuses(kw):
    args = dict(values=_v(1, 1, 3, 4), psf=H3, factor=4, response=[[0.3, 0.3, 0.4]])
    args.update(kw)
    with pytest.raises(EodError):
        PsfObservation(**args)


def test_what_is_accepted_and_what_is_kept():
    o = PsfObservation(_v(1, 2, 3, 4), H3, 4, None, _v(1, 1, 3, 4), [0.0, 1.0], 64, "cg", [0.0, 0.05], R32)     # the last positional
    assert o.response.dtype == np.float32 and o.response.shape == (2, 3) and o.pinv.dtype == np.float32 and o.pinv.shape == (3, 2)
    assert np.array_equal(o.pinv, np.linalg.pinv(np.float32(R32).astype(np.float64)).astype(np.float32))
    assert np.array_equal(o.pinv, SP.pinv32(R32)) and o.channels is None
    PsfObservation(_v(2, 1, 3, 4), H3, 4, response=torch.tensor(PAN4), mask=_v(2, 1, 3, 4), iters=8)           # a tensor; a soft mask with Landweber
    PsfObservation(_v(1, 8, 3, 4), H3, 1, response=np.eye(8, 32), solver="cg")                                  # the limits themselves
    PsfObservation(_v(1, 1, 3, 4), H3, 4, response=[[1, 2, 1]])                                                 # integers
    plain = PsfObservation(_v(1, 2, 3, 4), H3, 4, [0, 2])
    assert plain.response is None and plain.pinv is None                                                        # response=None: as before
    s = CO.SpectralObservation(_v(1, 2, 12, 16), R32)
    assert np.array_equal(s.pinv, o.pinv) and np.array_equal(s.response, o.response)                            # one rule for both kinds


@pytest.mark.parametrize("shape,n_eval", [
    ((2, 4, 12, 16), 2), ((2, 2, 12, 16), 2),     # C differs from response.shape[1]
    ((2, 33, 12, 16), 2),
    ((2, 3, 12, 12), 2), ((2, 3, 6, 8), 2),       # the coarse grid times f is not the state
    ((3, 3, 12, 16), 2),                          # leading dimension 2 of values
    ((2, 3, 12, 16), 3),                          # two weights
])
def test_bind_and_check_refuse_what_does_not_fit_the_call(shape, n_eval):
    o = PsfObservation(_v(2, 2, 3, 4), H3, 4, mask=_v(1, 1, 3, 4), weight=[1.0, 0.5], response=R32)
    for form in (o, [o]):
        with pytest.raises(EodError):
            bind(form, "call", shape, n_eval, "cpu")
        with pytest.raises(EodError):
            CO.check(form, "call", shape, n_eval)
    if shape[1] <= 32:
        ok = Observation(_v(1, shape[1], *shape[2:]), (1,) * shape[1])
        with pytest.raises(EodError):
            CO.check([ok, o], "call", shape, n_eval)


def test_bind_keeps_the_matrices_the_step_and_the_tables():
    shape = (2, 3, 12, 16)
    h = gaussian_psf(4)
    smax = np.linalg.svd(np.float32(R32).astype(np.float64), compute_uv=False)[0]
    lw = bind(PsfObservation(_v(2, 2, 3, 4), h, 4, iters=3, response=R32), "call", shape, 2, "cpu")
    assert isinstance(lw, CO.BoundChain) and [type(z) for z in lw.links] == [CO.BoundPsf]                       # alone: a chain of one
    lw = lw.links[0]
    assert lw.mixed and lw.K == 2 and lw.channels is None and lw.r == 6 and lw.iters == 3
    assert abs(lw.tau - PR.tau64(h, 4, 12, 16) / smax ** 2) <= 1e-13 * lw.tau
    assert lw.step == float(np.float32(lw.tau / 16)) == SP.step32(h, 4, 12, 16, R32)
    assert list(lw.c_R) == np.float32(R32).ravel().tolist() and list(lw.c_G) == np.float32(R32).T.ravel().tolist()      # Landweber: G = R^T
    cg = bind([PsfObservation(_v(2, 2, 3, 4), h, 4, solver="cg", iters=16, damping=0.05, response=R32)], "call", shape, 2, "cpu").links[0]
    assert cg.mixed and list(cg.c_G) == SP.pinv32(R32).ravel().tolist() and cg.unit_step == 1.0 / 16 and cg.band == 3   # cg: G = pinv(R)
    assert torch.equal(cg.gy, torch.from_numpy(psf_gram(h, 4, 12)[0])) and cg.dampings == [float(np.float32(0.05))] * 2
    plain = bind(PsfObservation(_v(2, 2, 3, 4), h, 4, [0, 2]), "call", shape, 2, "cpu").links[0]
    assert not plain.mixed and plain.channels == (0, 2) and plain.step == PR.step32(h, 4, 12, 16)
    s = CO.SpectralObservation(_v(1, 1, 12, 16), [[0.2, 0.5, 0.3]])
    chain = bind([s, PsfObservation(_v(2, 2, 3, 4), h, 4, response=R32), PsfObservation(_v(2, 2, 3, 4), h, 4, [0, 2])], "call", shape, 2, "cpu")
    assert [type(z) for z in chain.links] == [CO.BoundSpectral, CO.BoundPsf, CO.BoundPsf] and [getattr(z, "mixed", None) for z in chain.links] == [None, True, False]


def test_shard_carries_the_response():
    o = PsfObservation(_v(4, 2, 3, 4), H3, 4, mask=_v(4, 1, 3, 4), iters=16, solver="cg", damping=0.1, response=R32)
    for cut in (o.shard(4, 1, 3), CO.shard([o], 4, 1, 3)[0]):
        assert cut.values.shape[0] == 2 and cut.mask.shape[0] == 2 and cut.solver == "cg" and cut.iters == 16
        assert np.array_equal(cut.response, o.response) and np.array_equal(cut.pinv, o.pinv)
        assert bind(cut, "call", (2, 3, 12, 16), 2, "cpu").links[0].mixed


def test_psf_observe_refuses_on_the_host():
    x = _v(1, 3, 12, 12)
    for kw in (dict(response=R32, channels=[0, 1]), dict(response=PAN4), dict(response=[[0.5, 0.5, float("inf")]]), dict(response=np.eye(9, 3)),
               dict(response=[0.3, 0.3, 0.4]), dict(response=R32, factor=5)):
        args = dict(psf=[1.0], factor=2)
        args.update(kw)
        with pytest.raises(EodError):
            psf_observe(x, **args)
    with pytest.raises(EodError):                                                                    # (a CPU tensor: the kernel is mandatory)
        psf_observe(x, [1.0], 2, response=R32)


def test_the_dropin_path_sees_the_keyword():
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    assert D.PsfObservation is PsfObservation and D.PsfObservation(_v(1, 1, 3, 4), H3, 4, response=[[0.3, 0.3, 0.4]]).response.shape == (1, 3)


# ------------------------------------------------------------------------------------------------ the factorisation
def _inputs(case):
    R, f, mtf, (H, W), mu = TABLE[case]
    rng = np.random.default_rng(300 + case)
    h = PR.gaussian(f, mtf)
    K, C = np.shape(R)
    p = torch.from_numpy(rng.standard_normal((1, C, H, W)).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((1, K, H // f, W // f)).astype(np.float32))
    m = torch.from_numpy((rng.random((1, 1, H // f, W // f)) > 0.3).astype(np.float32))           # hides about 30 % of the coarse pixels
    return R, f, h, p, y, m, mu


def test_the_float64_operator_is_what_the_factors_say():
    """kron(R, A_H, A_W) against the einsum forms, <A x, q> = <x, A^T q>, and A A^T = (R R^T) (x) G_H (x) G_W"""
    R, f, h, p, y, m, _ = _inputs(2)
    H, W = p.shape[2:]
    A = SP.operator64(R, h, f, H, W)
    x64, q64 = p.numpy().astype(np.float64), y.numpy().astype(np.float64)
    assert np.abs(A @ x64.ravel() - SP.apply64(x64, h, f, R).ravel()).max() <= 1e-13
    assert np.abs(A.T @ q64.ravel() - SP.adjoint64(q64, h, f, H, W, R).ravel()).max() <= 1e-13
    R64 = np.float32(R).astype(np.float64)
    assert np.abs(A @ A.T - np.kron(R64 @ R64.T, np.kron(GR.gram64(h, H, f), GR.gram64(h, W, f)))).max() <= 1e-14


@pytest.mark.parametrize("case", range(4))
def test_emulation_lands_on_the_dense_solve(case):
    """white noise p and y, a binary mask, 48 iterations of the per-plane solve in the fp32 emulation: the correction within 1e-5 relative L2
    of the dense float64 solve on kron(R, A_H, A_W) (damped: of ((R R^T) (x) (M G M + mu I))^-1), and the true residual of that system, in
    float64 from the emulation's output, <= 1e-5 of its start.  Measured: corrections 1.6e-7 to 3.8e-7, residuals 8.9e-8 to 5.8e-7"""
    R, f, h, p, y, m, mu = _inputs(case)
    H, W = p.shape[2:]
    gy, gx = (torch.from_numpy(psf_gram(h, f, L)[0]) for L in (H, W))
    out = SP.project_cg(p, y, h, f, gy, gx, R, m, 1.0, mu, iters=48)
    q = GR.cg32(SP.residual(p, y, h, f, R, m, 1.0), gy, gx, m, mu, 1.0, 48).numpy().astype(np.float64)      # the solve's own output, m * z
    p64, y64, m64 = (z.numpy().astype(np.float64) for z in (p, y, m))
    want, c = SP.dense_correction64(p64, y64, h, f, R, m64, float(np.float32(mu)))
    got = out.numpy().astype(np.float64) - p64
    e_cor = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    if mu == 0.0:
        res = m64 * (SP.apply64(out.numpy(), h, f, R) - y64)
    else:                                             # of the damped per-plane system the solve is handed: c - (M G M + mu I) z
        Gy, Gx = GR.gram64(h, H, f), GR.gram64(h, W, f)
        res = c - (m64 * np.einsum("yh,bkhw,xw->bkyx", Gy, m64 * q, Gx) + float(np.float32(mu)) * q)
    e_res = float(np.linalg.norm(res) / np.linalg.norm(c))
    print(f"case {case} (cond R {np.linalg.cond(np.float32(R).astype(np.float64)):.3g}, mu = {mu}): correction vs dense {e_cor:.3e}; "
          f"residual left / its start {e_res:.3e}")
    assert e_cor <= 1e-5 and e_res <= 1e-5


@pytest.mark.parametrize("case", range(3))
def test_landweber_step_size_bounds_the_dense_operator(case):
    """tau ||A||_2^2 <= 1 in float64 on the dense kron(R, A_H, A_W), tau = psf_tau / sigma_max(R)^2 as the link binds it"""
    R, f, h, p, y, m, _ = _inputs(case)
    B, C, H, W = p.shape
    link = bind(PsfObservation(y, h, f, response=R), "call", (B, C, H, W), 1, "cpu").links[0]
    norm2 = float(np.linalg.norm(SP.operator64(R, h, f, H, W), 2)) ** 2
    print(f"case {case}: tau ||A||^2 = {link.tau * norm2:.4f}")
    assert link.tau * norm2 <= 1.0 + 1e-12
    assert link.tau * norm2 >= 1.0 / 1.16 ** 2 - 1e-9                                  # (psf_ref's bound on cmax: the step is not needlessly small)


def test_emulation_follows_float64():
    for case in range(3):
        R, f, h, p, y, m, _ = _inputs(case)
        got = SP.project(p, y, h, f, R, m, 0.75, iters=3)
        want = SP.landweber64(p.numpy(), y.numpy(), h, f, R, m.numpy(), 0.75, iters=3)
        assert np.abs(got.numpy() - want).max() <= 64 * XR.EPS * max(1.0, float(p.abs().max()))
        gy, gx = GR.tables(h, f, *p.shape[2:])
        got = SP.project_cg(p, y, h, f, gy, gx, R, m, 0.75, 0.05, iters=4)
        want = SP.cg64(p.numpy(), y.numpy(), h, f, R, m.numpy(), 0.75, float(np.float32(0.05)), iters=4)
        assert np.abs(got.numpy() - want).max() <= 256 * XR.EPS * max(1.0, float(p.abs().max()))


def test_one_hot_rows_are_the_unmixed_emulation():
    """rows of the identity and G = R^T: the mixed emulation has the bits of psf_ref's with that channel list, unlisted channels included"""
    _, f, h, p, _, m, _ = _inputs(2)
    cs = (1, 3)
    R = np.eye(4, dtype=np.float32)[list(cs)]
    y = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 2, 4, 6)).astype(np.float32))
    q = SP.residual(p, y, h, f, R, m, 0.625)
    assert bits_equal(q, PR.residual(p, y, h, f, cs, m, 0.625)) and bits_equal(SP.apply(p, h, f, R), PR.apply(p, h, f, cs))
    assert bits_equal(SP.update(p, q, h, f, R.T, 0.9), PR.update(p, q, h, f, cs, 0.9))


@pytest.mark.parametrize("case", range(3))
def test_nothing_observed_returns_its_input(case):
    """weight 0 and an all-zero mask, both solvers: the input bit for bit"""
    R, f, h, p, y, m, _ = _inputs(case)
    gy, gx = GR.tables(h, f, *p.shape[2:])
    zero = torch.zeros_like(m)
    assert bits_equal(SP.project(p, y, h, f, R, m, 0.0, iters=2), p) and bits_equal(SP.project(p, y, h, f, R, zero, 1.0, iters=2), p)
    assert bits_equal(SP.project_cg(p, y, h, f, gy, gx, R, m, 0.0, 0.0, iters=5), p)
    assert bits_equal(SP.project_cg(p, y, h, f, gy, gx, R, zero, 1.0, 0.05, iters=5), p)
    assert not torch.equal(SP.project_cg(p, y, h, f, gy, gx, R, m, 1.0, 0.0, iters=5), p)


# ------------------------------------------------------------------------------------------------ the toy loop
def test_float64_ddim_loop_on_the_toy_with_a_pan_link():
    """section 9.4's Gaussian toy as a 4 x 32 x 32 image (20 levels) with a pan band through the PSF at f = 4 after every prediction: with the
    cg link at 16 iterations the loop ends with ||A x - y|| at most one tenth of the Landweber link's at 4 steps (section 9.9's gate).
    Measured: Landweber iters=4 0.0283, cg iters=16 0.0002 (unconstrained 0.3488)"""
    from oracle import schedule as SCH
    acp = SCH.eo_cosine_tables(1000)["alphas_cumprod"].numpy().astype(np.float64)
    levels = make_dpm_timesteps("uniform", 20, acp)
    truth = np.random.default_rng(5).uniform(-1, 1, CR.TOY_SHAPE)
    h = gaussian_psf(4)
    y = SP.apply64(truth, h, 4, PAN4)
    dist = lambda z: float(np.linalg.norm(SP.apply64(z.reshape(CR.TOY_SHAPE), h, 4, PAN4) - y))
    lw, _, _ = XR.ddim_f64(acp, levels, [SP.link64(y, h, 4, PAN4, iters=4)])
    cg, _, _ = XR.ddim_f64(acp, levels, [SP.cg_link64(y, h, 4, PAN4, iters=16)])
    free, _, _ = XR.ddim_f64(acp, levels)
    print(f"||A x - y|| at the end: unconstrained {dist(free):.4f}, Landweber iters=4 {dist(lw):.4f}, cg iters=16 {dist(cg):.4f}")
    assert dist(cg) <= 0.1 * dist(lw) and dist(lw) < dist(free)
    zero, _, _ = XR.ddim_f64(acp, levels, [SP.cg_link64(y, h, 4, PAN4, lam=0.0, iters=16)])
    assert np.array_equal(zero, free)


# ------------------------------------------------------------------------------------------------ the kernels' bodies on the host
def test_kernel_bodies_run_clean_under_sanitizers_and_match_the_contract(tmp_path):
    """tests/spectral_psf_host_check.cc: the mixed phases of csrc/psf_body.h compiled for the host with -fsanitize=address,undefined and run as
    a program of its own (nothing is loaded into this interpreter) over planes from one coarse pixel to ragged tiles, (C, K) up to (32, 8),
    every access form, mask absent / full / broadcast, exactly sized buffers"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "spectral_psf_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "spectral_psf_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
