"""CPU: the exact PSF data consistency (PsfObservation(solver="cg"), psf_gram, tests/psf_cg_ref.py): every new refusal;
the Gram tables against A1 A1^T; float64 conjugate gradients against a dense solve; the fp32 emulation of the solve against the dense solve and
its identities; the float64 DDIM loop on the Gaussian toy with a cg link next to the Landweber link; the kernels' bodies compiled for the host
and run under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import PsfObservation, bind, gaussian_psf, psf_gram
from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
from tests import consistency_ref as CR
from tests import psf_cg_ref as GR
from tests import psf_ref as PR
from tests import spectral_ref as XR
from tests.helpers import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _v(*shape):
    return torch.zeros(*shape)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw", [
    dict(solver="fft"), dict(solver=None), dict(solver=1), dict(solver="CG"),
    dict(iters=9),                                                          # still refused for Landweber
    dict(solver="cg", iters=65), dict(solver="cg", iters=0), dict(solver="cg", iters=2.0),
    dict(solver="cg", damping=-0.01), dict(solver="cg", damping=float("nan")), dict(solver="cg", damping=float("inf")),
    dict(solver="cg", damping=[0.1, -0.1]), dict(solver="cg", damping="a"), dict(solver="cg", damping=True), dict(solver="cg", damping=None),
    dict(damping=0.05), dict(solver="landweber", damping=[0.0, 0.05]),      # damping belongs to cg
    dict(solver="cg", mask=torch.full((1, 1, 3, 4), 0.5)),                   # a soft mask
    dict(solver="cg", mask=torch.tensor([[[[1.0, 0.0, 1.0, 0.999], [1.0] * 4, [0.0] * 4]]])),
])
def test_psf_observation_refuses(kw):
    args = dict(values=_v(1, 2, 3, 4), psf=[0.25, 0.5, 0.25], factor=4, channels=[0, 2], mask=None, weight=1.0, iters=1)
    args.update(kw)
    with pytest.raises(EodError):
        PsfObservation(**args)


def test_the_soft_mask_refusal_names_the_way_out():
    with pytest.raises(EodError, match="weight.*damping"):
        PsfObservation(_v(1, 2, 3, 4), [0.25, 0.5, 0.25], 4, [0, 2], torch.full((1, 1, 3, 4), 0.5), solver="cg")


def test_what_is_accepted():
    o = PsfObservation(_v(1, 2, 3, 4), [0.25, 0.5, 0.25], 4, [0, 2], _v(1, 1, 3, 4), [0.0, 1.0], 64, "cg", [0.0, 0.05])
    assert o.solver == "cg" and o.iters == 64 and o.damping_per_evaluation and o.dampings == [0.0, float(np.float32(0.05))]
    assert CO.MAX_CG_ITERS == 64 and CO.MAX_ITERS == 8
    o = PsfObservation(_v(1, 2, 3, 4), [0.25, 0.5, 0.25], 4, [0, 2], torch.ones(1, 2, 3, 4), solver="cg", damping=0)
    assert o.dampings == [0.0] and not o.damping_per_evaluation
    o = PsfObservation(_v(1, 2, 3, 4), [0.25, 0.5, 0.25], 4, [0, 2], torch.full((1, 1, 3, 4), 0.5), iters=8, damping=0.0)      # soft masks stay with Landweber
    assert o.solver == "landweber" and o.iters == 8


def test_bind_checks_the_damping_sequence_and_keeps_the_tables():
    shape = (2, 3, 12, 16)
    o = PsfObservation(_v(2, 2, 3, 4), gaussian_psf(4), 4, [0, 2], weight=[1.0, 0.5, 0.25], iters=16, solver="cg", damping=[0.0, 0.1, 0.2])
    for n in (2, 4):
        with pytest.raises(EodError):
            bind(o, "call", shape, n, "cpu")
        with pytest.raises(EodError):
            CO.check([o], "call", shape, n)
    link = bind(o, "call", shape, 3, "cpu").links[0]
    assert link.solver == "cg" and link.iters == 16 and link.band == 3 and link.dampings == [0.0, float(np.float32(0.1)), float(np.float32(0.2))]
    assert link.gy.shape == (3, 7) and link.gx.shape == (4, 7) and link.gy.dtype == torch.float32
    assert torch.equal(link.gy, torch.from_numpy(psf_gram(gaussian_psf(4), 4, 12)[0]))
    assert link.unit_step == 1.0 / 16
    one = PsfObservation(_v(2, 2, 3, 4), gaussian_psf(4), 4, [0, 2], solver="cg", damping=0.05)
    assert bind(one, "call", shape, 3, "cpu").links[0].dampings == [float(np.float32(0.05))] * 3
    cut = o.shard(2, 1, 2)                                                  # shard() copies the new fields
    assert cut.solver == "cg" and cut.dampings == o.dampings and cut.iters == 16 and cut.values.shape[0] == 1
    lw = bind(PsfObservation(_v(2, 2, 3, 4), gaussian_psf(4), 4, [0, 2], iters=3), "call", shape, 3, "cpu").links[0]
    assert lw.solver == "landweber" and not hasattr(lw, "gy")


def test_the_dropin_path_re_exports_the_new_names():
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    assert D.psf_gram is psf_gram and D.MAX_CG_ITERS == 64


# ------------------------------------------------------------------------------------------------ the Gram tables
@pytest.mark.parametrize("f", range(1, 9))
@pytest.mark.parametrize("r", [0, 1, 12])
def test_psf_gram_is_a1_a1t(f, r):
    """to 1e-7 relative per entry (the table is fp32: half an ulp is 6e-8) plus fp32's subnormal spacing 2^-149, which is what rounding to
    fp32 costs the products of two far taps of a wide Gaussian (1e-40 and below)"""
    h = PR.gaussian(f, 0.3, radius=r)
    for L in (f, 3 * f, 13 * f):
        bands, b = psf_gram(h, f, L)
        G = GR.gram64(h, L, f)
        assert b == -((-2 * r) // f) and bands.dtype == np.float32 and bands.shape == (L // f, 2 * b + 1)
        want = GR.bands_of(G, b)
        assert np.all(np.abs(bands - want) <= 1e-7 * np.abs(want) + 2.0 ** -149)
        i, j = np.indices(G.shape)
        assert np.all(G[np.abs(i - j) > b] == 0.0)                          # zero beyond b = ceil(2r / f)
        D = GR.dense_of(bands)
        assert np.array_equal(D, D.T)                                       # symmetric bit for bit
        assert np.all(bands[GR.bands_of(np.ones_like(G), b) == 0.0] == 0.0)   # zero where the column lies outside the line


def test_psf_gram_of_identity_taps_and_of_a_scene_line():
    for f in range(1, 9):
        bands, b = psf_gram([1.0], f, 5 * f)
        assert b == 0 and np.array_equal(bands, np.full((5, 1), np.float32(1.0 / f)))
    h = gaussian_psf(2)
    t0 = time.perf_counter()
    bands, b = psf_gram(h, 2, 10980)
    assert time.perf_counter() - t0 < 1.0 and bands.shape == (5490, 2 * b + 1) and b == 3
    inner = GR.bands_of(GR.gram64(h, 40, 2), b)[10]                          # far from both ends the rows are one stencil
    assert np.all(np.abs(bands[2000] - inner) <= 1e-7 * np.abs(inner))
    for bad in (dict(L=0), dict(L=7), dict(L=True), dict(L=8.0), dict(factor=9), dict(taps=[0.2, 0.5, 0.3])):
        kw = dict(taps=h, factor=2, L=8)
        kw.update(bad)
        with pytest.raises(EodError):
            psf_gram(**kw)


# ------------------------------------------------------------------------------------------------ the cases of the issue's table
#        f  mtf  H   W   mask      mu
TABLE = [(4, 0.3, 32, 32, None, 0.0),
         (4, 0.6, 32, 32, None, 0.0),
         (2, 0.3, 24, 28, "binary", 0.0),
         (8, 0.3, 64, 64, "binary", 0.0),
         (4, 0.3, 32, 32, None, 0.05),
         (6, 0.3, 36, 48, "soft", 0.0)]


def _mask(kind, rng, Hc, Wc):
    if kind is None:
        return None
    u = rng.random((1, 1, Hc, Wc))
    return (u > 0.3).astype(np.float64) if kind == "binary" else 0.02 + 0.96 * u


@pytest.mark.parametrize("case", range(6))
def test_float64_cg_reaches_the_dense_solve(case):
    """a 12 x 12-coarse version of each case, 144 iterations = the number of unknowns.  The bound is the textbook one,
    |z_k - z| <= 2 sqrt(kappa) ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k |z| in the 2-norm with kappa of the restricted system as numpy
    measures it, plus 1e-10 for float64 rounding of a system of that conditioning (144 steps of eps * kappa <= 1e-16 * 1e4 * 144)"""
    f, mtf, _, _, kind, mu = TABLE[case]
    rng = np.random.default_rng(100 + case)
    h = PR.gaussian(f, mtf)
    Gy = Gx = GR.gram64(h, 12 * f, f)
    m = _mask(kind, rng, 12, 12)
    c = rng.standard_normal((1, 2, 12, 12)) * (1.0 if m is None else (m != 0))
    want = GR.dense64(c, Gy, Gx, m, mu)
    got = GR.cg64(c, Gy, Gx, m, mu, iters=144)
    mm = np.ones(144) if m is None else m.ravel()
    S = (mm[:, None] * np.kron(Gy, Gx) * mm[None, :])[np.ix_(mm != 0, mm != 0)] + mu * np.eye(int((mm != 0).sum()))
    kappa = float(np.linalg.cond(S))
    q = (np.sqrt(kappa) - 1.0) / (np.sqrt(kappa) + 1.0)
    bound = 2.0 * np.sqrt(kappa) * q ** 144 + 1e-10
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"case {case}: cond {kappa:.3g}, float64 CG vs dense {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    if kind != "soft":
        assert err <= 1e-8


def _table_inputs(case):
    f, mtf, H, W, kind, mu = TABLE[case]
    rng = np.random.default_rng(200 + case)
    h = PR.gaussian(f, mtf)
    p = torch.from_numpy(rng.standard_normal((1, 2, H, W)).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((1, 2, H // f, W // f)).astype(np.float32))
    m = _mask(kind, rng, H // f, W // f)
    return f, h, p, y, None if m is None else torch.from_numpy(m.astype(np.float32)), mu


@pytest.mark.parametrize("case", range(5))
def test_emulation_lands_on_the_dense_solve(case):
    """white noise p and y (the worst case), 48 iterations: the correction p_out - p within 1e-5 relative L2 of the dense float64 solve's.
    Measured: 2.2e-7 to 5.1e-7"""
    f, h, p, y, m, mu = _table_inputs(case)
    H, W = p.shape[2:]
    gy, gx = (torch.from_numpy(psf_gram(h, f, L)[0]) for L in (H, W))
    out = GR.project32(p, y, h, f, gy, gx, None, m, 1.0, mu, iters=48)
    p64, m64 = p.numpy().astype(np.float64), None if m is None else m.numpy().astype(np.float64)
    c = (1.0 if m64 is None else m64) * (PR.apply64(p64, h, f) - y.numpy())
    z = GR.dense64(c, GR.gram64(h, H, f), GR.gram64(h, W, f), m64, mu)
    want = -PR.adjoint64((1.0 if m64 is None else m64) * z, h, f, H, W)
    got = out.numpy().astype(np.float64) - p64
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    res = (1.0 if m64 is None else m64) * (PR.apply64(out.numpy(), h, f) - y.numpy())
    print(f"case {case}: correction vs dense {err:.3e}; true residual / start {np.linalg.norm(res) / np.linalg.norm(c):.3e} (mu = {mu})")
    assert err <= 1e-5


def test_emulation_with_nothing_observed_returns_its_input():
    f, h, p, y, m, mu = _table_inputs(2)
    gy, gx = GR.tables(h, f, *p.shape[2:])
    assert bits_equal(GR.project32(p, y, h, f, gy, gx, None, m, 0.0, 0.0, iters=5), p)
    assert bits_equal(GR.project32(p, y, h, f, gy, gx, None, torch.zeros_like(m), 1.0, 0.05, iters=5), p)
    out = GR.project32(p, y[:, 1:], h, f, gy, gx, (1,), m, 1.0, 0.0, iters=5)                 # a channel that is not listed is copied
    assert bits_equal(out[:, 0], p[:, 0]) and not torch.equal(out[:, 1], p[:, 1])


def test_emulation_with_identity_taps_is_the_block_mean_projection():
    """G = I / f^2 exactly for f a power of two: one iteration solves it"""
    rng = np.random.default_rng(9)
    for f in (1, 2, 4, 8):
        p = torch.from_numpy(rng.standard_normal((2, 3, 2 * f, 3 * f)).astype(np.float32))
        y = torch.from_numpy(rng.uniform(-1, 1, (2, 3, 2, 3)).astype(np.float32))
        gy, gx = GR.tables([1.0], f, 2 * f, 3 * f)
        got = GR.project32(p, y, np.float32([1.0]), f, gy, gx, iters=1)
        rep = lambda z: z.repeat_interleave(f, 2).repeat_interleave(f, 3).contiguous()
        want = CR.project(p, rep(y), (f,) * 3, None, 1.0)
        assert float((got - want).abs().max()) <= 4 * XR.EPS * max(1.0, float(p.abs().max()))


# ------------------------------------------------------------------------------------------------ the toy loop
def test_float64_ddim_loop_on_the_toy_lands_where_landweber_does_not():
    """section 9.4's Gaussian toy as a 4 x 32 x 32 image with a PSF link at f = 4 after every prediction, as tests/test_psf_host.py runs it:
    with the cg link at 16 iterations the loop ends with ||A x - y|| below one tenth of the Landweber link's at 4 steps.
    Measured: Landweber iters=4 0.0908, cg iters=16 0.0013"""
    from oracle import schedule as SCH
    acp = SCH.eo_cosine_tables(1000)["alphas_cumprod"].numpy().astype(np.float64)
    levels = make_dpm_timesteps("uniform", 20, acp)
    truth = np.random.default_rng(5).uniform(-1, 1, CR.TOY_SHAPE)
    h = gaussian_psf(4)
    y = PR.apply64(truth, h, 4)
    dist = lambda z: float(np.linalg.norm(PR.apply64(z.reshape(CR.TOY_SHAPE), h, 4) - y))
    lw, _, _ = XR.ddim_f64(acp, levels, [PR.psf_link64(y, h, 4, iters=4)])
    cg, _, _ = XR.ddim_f64(acp, levels, [GR.cg_link64(y, h, 4, iters=16)])
    print(f"||A x - y|| at the end: Landweber iters=4 {dist(lw):.4f}, cg iters=16 {dist(cg):.4f}")
    assert dist(cg) < 0.1 * dist(lw)
    free, _, _ = XR.ddim_f64(acp, levels)
    zero, _, _ = XR.ddim_f64(acp, levels, [GR.cg_link64(y, h, 4, lam=0.0, iters=16)])
    assert np.array_equal(zero, free)


# ------------------------------------------------------------------------------------------------ the kernels' bodies on the host
def test_kernel_bodies_run_clean_under_sanitizers_and_match_the_contract(tmp_path):
    """tests/psf_cg_host_check.cc: csrc/psf_cg_body.h compiled for the host with -fsanitize=address,undefined and run as a program of its own
    (nothing is loaded into this interpreter) over planes of 1 x 1, planes inside the halo, b in {0, 3, 24}, ragged tiles, both access forms"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "psf_cg_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "psf_cg_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
