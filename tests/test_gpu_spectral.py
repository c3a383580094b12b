"""GPU: cross-band observations and chains of observations -- eod_ddim_step_spec, eod_dpmpp_step_spec, eod_spec_project, eod_spec_apply,
eod_obs_project, eod_pred_x0, eod_ddim_step_p0, eod_dpmpp_step_p0 (csrc/sampler.hip) and SpectralObservation / lists on `observation=`
(diffusion/consistency.py).  DESIGN.md section 9.6.

The kernels are held bit for bit to the torch fp32 emulation of tests/spectral_ref.py (the order include/eodiff.h states) for ANY values and a
soft mask; the fused kernels to the unfused route; nothing observed to the plain step kernels; R = I to the observation itself; a member of
a batch to the launch on its slice; the residual to the emulation's; whole calls with injected draws to CPU loops of the oracle UNet and
the emulated steps under the trajectory gates of tests/test_gpu_sampling.py; scenes to sample() on the tiles and to the emulation on the
recorded inputs of the scene-level step; every refusal to a forward hook that sees no call."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.consistency import Observation, SpectralObservation, block_mean, spectral_response
from eo_diffusion_amd.tiling import TilePlan
from tests import consistency_ref as CR
from tests import spectral_ref as XR
from tests import test_gpu_consistency as TC
from tests.gpu_util import DEV
from tests.helpers import bits_equal, rel_l2
from tests.synth import synth_input
from tests.test_gpu_dpm_solver import LEVELS, _eps_tiny, _nan, _offset_by_4_bytes, _scalars, dpmpp
from tests.test_gpu_sampling import TRAJ_TOL, _model
from tests.test_gpu_scene import _diffusion, cut, stitch
from tests.test_gpu_scene_skip import Calls

pytestmark = pytest.mark.gpu

EPS = XR.EPS
# (C, K, f, (H, W)): each the smallest reach of a branch of spec_kernel / its launcher
CASES = [(1, 1, 1, (16, 16)),       # the smallest plane
         (4, 1, 1, (6, 7)),         # hw % 4 != 0: the scalar tail of the quads
         (4, 1, 1, (16, 16)),       # aligned quads
         (13, 3, 1, (12, 18)),
         (32, 8, 1, (8, 8)),        # both limits
         (2, 1, 4, (16, 16)),
         (13, 8, 2, (12, 28)),      # the 8-byte form
         (3, 3, 3, (12, 18)),       # square R, odd f
         (7, 4, 5, (35, 70)),
         (13, 2, 6, (24, 30)),
         (5, 2, 8, (24, 168))]
MODES = {"full": (True, True), "bcast": (False, False), "nomask": (True, None)}      # values per sample?, mask per sample? (None: no mask)


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _mat(M):
    M = np.ascontiguousarray(M, np.float32)
    return (ctypes.c_float * M.size)(*M.ravel().tolist())


def _matrices(C, K, seed=None):
    R = XR.response(K, C, 100 + 7 * C + K if seed is None else seed)
    assert XR.rcond(R) >= XR.MIN_RCOND                                   # (float64: the matrix passes the conditioning refusal)
    return R, XR.pinv32(R)


def _tensors(C, K, H, W, B, mode, unaligned=False, seed=11):
    """device tensors of a kernel case: arbitrary per-pixel values, a soft mask"""
    vb, mb = MODES[mode]
    shape = (B, C, H, W)
    t = dict(x=synth_input("qx", shape, seed), e=synth_input("qe", shape, seed + 1), d=synth_input("qd", shape, seed + 2),
             noise=synth_input("qn", shape, seed + 3), values=synth_input("qv", (B if vb else 1, K, H, W), seed + 4, uniform=True) * 2 - 1)
    if mb is not None:
        t["mask"] = synth_input("qm", (B if mb else 1, 1, H, W), seed + 5, uniform=True)
    t = {k: v.to(DEV) for k, v in t.items()}
    t["out"], t["p0"] = _nan(*shape), _nan(*shape)
    if unaligned:
        t = {k: _offset_by_4_bytes(v) for k, v in t.items()}
    return t


def _cpu(t, *names):
    return [None if t.get(k) is None else t[k].cpu() for k in names]


def _tail(t, R, G, f, lam):
    B, C, H, W = t["x"].shape
    v, m = t["values"], t.get("mask")
    return (v.data_ptr(), _lib.ptr(m), float(lam), _mat(R), _mat(G), int(R.shape[0]), int(f), B, C, H, W, int(v.shape[0] != B),
            int(m is not None and m.shape[0] != B))


def ddim_spec(t, R, G, f, lam, a_t, a_prev, sigma, s1m, temperature=1.0):
    """eod_ddim_step_spec itself on the tensors of t; returns (rc, x_prev, pred_x0)"""
    rc = _lib.lib().eod_ddim_step_spec(t["x"].data_ptr(), t["e"].data_ptr(), _lib.ptr(t.get("noise")), float(a_t), float(a_prev), float(sigma),
                                       float(s1m), float(temperature), *_tail(t, R, G, f, lam), t["out"].data_ptr(), t["p0"].data_ptr(), _stream())
    return rc, t["out"], t["p0"]


def dpm_spec(t, R, G, f, lam, a_s, s1m, c, clip, second):
    rc = _lib.lib().eod_dpmpp_step_spec(t["x"].data_ptr(), t["e"].data_ptr(), _lib.ptr(t["d"] if second else None), float(a_s), float(s1m),
                                        *(float(v) for v in c), int(clip), *_tail(t, R, G, f, lam), t["out"].data_ptr(), t["p0"].data_ptr(),
                                        _stream())
    return rc, t["out"], t["p0"]


def spec_project(t, R, G, f, lam, p=None, out=None):
    """eod_spec_project of p (default: t["x"]) into out (default: t["out"])"""
    p = t["x"] if p is None else p
    out = t["out"] if out is None else out
    rc = _lib.lib().eod_spec_project(p.data_ptr(), *_tail(t, R, G, f, lam), out.data_ptr(), _stream())
    return rc, out


def obs_project(t, factors, lam, p, out):
    rc = _lib.lib().eod_obs_project(p.data_ptr(), *TC._tail(t, factors, lam), out.data_ptr(), _stream())
    return rc, out


def pred_x0(x, e, a, s1m, clip, out):
    return _lib.lib().eod_pred_x0(x.data_ptr(), e.data_ptr(), float(a), float(s1m), int(clip), out.data_ptr(), x.numel(), _stream()), out


def ddim_p0(e, p0c, noise, a_prev, sigma, temperature, out):
    return _lib.lib().eod_ddim_step_p0(e.data_ptr(), p0c.data_ptr(), _lib.ptr(noise), float(a_prev), float(sigma), float(temperature),
                                       out.data_ptr(), e.numel(), _stream()), out


def dpm_p0(x, p0c, d, c, out):
    return _lib.lib().eod_dpmpp_step_p0(x.data_ptr(), p0c.data_ptr(), _lib.ptr(d), *(float(v) for v in c), out.data_ptr(), x.numel(), _stream()), out


def _refill(t):
    t["out"].fill_(float("nan")), t["p0"].fill_(float("nan"))


# ------------------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
def _check_ddim(t, R, G, f, levels=LEVELS):
    x, e, noise, values, mask = _cpu(t, "x", "e", "noise", "values", "mask")
    for (a_t, a_prev), sigma, lam in zip(levels, (0.0, 0.3, 0.005), (1.0, 0.625, 0.3)):          # (sigma^2 < 1 - a_prev at every level)
        for with_noise in (True, False):
            a, s1m, _ = _scalars(a_t, a_prev, False)
            rc, got_x, got_p = ddim_spec(dict(t, noise=t["noise"] if with_noise else None), R, G, f, lam, a, np.float32(a_prev), sigma, s1m, 0.9)
            assert rc == 0, _lib.lib().eod_last_error()
            want_x, want_p = XR.ddim_step(x, e, noise if with_noise else None, a, a_prev, sigma, s1m, 0.9, [XR.spec_link(values, R, f, mask, lam, G)])
            assert bool(torch.isfinite(got_x).all()) and bool(torch.isfinite(got_p).all())
            assert bits_equal(got_p.cpu(), want_p) and bits_equal(got_x.cpu(), want_x), (a_t, with_noise)
            _refill(t)


def _check_dpm(t, R, G, f, levels=LEVELS):
    x, e, d, values, mask = _cpu(t, "x", "e", "d", "values", "mask")
    for (a_s, a_t), lam in zip(levels, (1.0, 0.625, 0.3)):
        for second in (False, True):
            for clip in (False, True):
                a, s1m, c = _scalars(a_s, a_t, second)
                rc, got_x, got_p = dpm_spec(t, R, G, f, lam, a, s1m, c, clip, second)
                assert rc == 0, _lib.lib().eod_last_error()
                want_x, want_p = XR.dpm_step(x, e, d if second else None, a, s1m, *c, clip, [XR.spec_link(values, R, f, mask, lam, G)])
                assert bool(torch.isfinite(got_x).all()) and bool(torch.isfinite(got_p).all())
                assert bits_equal(got_p.cpu(), want_p) and bits_equal(got_x.cpu(), want_x), (a_s, second, clip)
                _refill(t)


def _check_project(t, R, G, f):
    """eod_spec_project and eod_spec_apply on a given prediction (three scales of it)"""
    values, mask = _cpu(t, "values", "mask")
    for scale, lam in zip((1.0, 600.0, 1e-3), (1.0, 0.625, 0.3)):
        p = (t["x"] * scale).contiguous() if t["x"].data_ptr() % 16 == 0 else _offset_by_4_bytes(t["x"] * scale)
        rc, got = spec_project(t, R, G, f, lam, p)
        assert rc == 0, _lib.lib().eod_last_error()
        assert bits_equal(got.cpu(), XR.project(p.cpu(), values, R, G, f, mask, lam)) and bool(torch.isfinite(got).all())
        band = _nan(p.shape[0], R.shape[0], *p.shape[2:])
        band = band if p.data_ptr() % 16 == 0 else _offset_by_4_bytes(band)
        rc = _lib.lib().eod_spec_apply(p.data_ptr(), _mat(R), R.shape[0], f, band.data_ptr(), *p.shape, _stream())
        assert rc == 0 and bits_equal(band.cpu(), XR.apply(p.cpu(), R, f))
        _refill(t)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,K,f,plane", CASES)
def test_ddim_step_spec_is_bit_exact(C, K, f, plane, B, mode, unaligned):
    _check_ddim(_tensors(C, K, *plane, B, mode, unaligned), *_matrices(C, K), f)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,K,f,plane", CASES)
def test_dpmpp_step_spec_is_bit_exact(C, K, f, plane, B, mode, unaligned):
    _check_dpm(_tensors(C, K, *plane, B, mode, unaligned), *_matrices(C, K), f)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,K,f,plane", CASES)
def test_spec_project_and_apply_are_bit_exact(C, K, f, plane, B, mode, unaligned):
    _check_project(_tensors(C, K, *plane, B, mode, unaligned), *_matrices(C, K), f)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("mode", ["full", "bcast", "mixed", "nomask"])
@pytest.mark.parametrize("factors,plane", TC.PLANES)
def test_obs_project_is_the_block_mean_emulation(factors, plane, mode, unaligned):
    """eod_obs_project on a given p: tests/consistency_ref.py project (block_mean, then the four operations), bit for bit"""
    t = TC._tensors(factors, *plane, 2, mode, unaligned)
    values, mask = _cpu(t, "values", "mask")
    for scale, lam in zip((1.0, 600.0), (1.0, 0.3)):
        p = (t["x"] * scale).contiguous() if not unaligned else _offset_by_4_bytes(t["x"] * scale)
        rc, got = obs_project(t, factors, lam, p, t["out"])
        assert rc == 0, _lib.lib().eod_last_error()
        assert bits_equal(got.cpu(), CR.project(p.cpu(), values, factors, mask, lam))
        t["out"].fill_(float("nan"))


@pytest.mark.parametrize("one", ["x", "e", "d", "noise", "values", "mask", "out", "p0"])
def test_one_unaligned_pointer_takes_the_scalar_form_with_the_same_bits(one):
    C, K, f, plane = 13, 8, 2, (12, 28)
    R, G = _matrices(C, K)
    t = _tensors(C, K, *plane, 2, "full")
    t[one] = _offset_by_4_bytes(t[one])
    _check_dpm(t, R, G, f, LEVELS[:1])
    _check_ddim(t, R, G, f, LEVELS[:1])
    t4 = _tensors(4, 1, 16, 16, 2, "full")                   # and the quads of f = 1
    t4[one] = _offset_by_4_bytes(t4[one])
    _check_dpm(t4, *_matrices(4, 1), 1, LEVELS[:1])


def test_a_plane_beyond_the_grid_cap_is_walked_by_the_stride_loop():
    """f = 1, B = 1: more quads than EOD_SPEC_GRID_BLOCKS * 256 threads, so the first threads take a second quad"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eodiff.h")).read()
    cap = int(re.search(r"#define EOD_SPEC_GRID_BLOCKS (\d+)", hdr).group(1))
    assert cap == _lib.SPEC_GRID_BLOCKS
    W = 2048
    H = -(-cap * 256 * 4 // W) + 2
    assert (H * W) // 4 > cap * 256 and (H * W) // 4 < cap * 256 * 2
    C, K = 2, 1
    R, G = _matrices(C, K)
    t = _tensors(C, K, H, W, 1, "bcast")
    x, e, d, values, mask = _cpu(t, "x", "e", "d", "values", "mask")
    a, s1m, c = _scalars(0.37, 0.61, True)
    rc, got_x, got_p = dpm_spec(t, R, G, 1, 0.625, a, s1m, c, True, True)
    want_x, want_p = XR.dpm_step(x, e, d, a, s1m, *c, True, [XR.spec_link(values, R, 1, mask, 0.625, G)])
    assert rc == 0 and bits_equal(got_p.cpu(), want_p) and bits_equal(got_x.cpu(), want_x)


# ------------------------------------------------------------------------------------------------------------ 2. invariants
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("C,K,f,plane", CASES)
def test_fused_equals_unfused_for_the_cross_band_observation(C, K, f, plane, unaligned):
    """eod_pred_x0 -> eod_spec_project -> eod_ddim_step_p0 / eod_dpmpp_step_p0 against the one-launch kernels"""
    R, G = _matrices(C, K)
    t = _tensors(C, K, *plane, 2, "full", unaligned)
    mk = (lambda: _offset_by_4_bytes(_nan(*t["x"].shape))) if unaligned else (lambda: _nan(*t["x"].shape))
    for (a_s, a_t), lam, sigma in zip(LEVELS, (1.0, 0.625, 0.3), (0.0, 0.3, 0.005)):
        for second in (False, True):
            for clip in (False, True):
                a, s1m, c = _scalars(a_s, a_t, second)
                rc, want_x, want_p = dpm_spec(t, R, G, f, lam, a, s1m, c, clip, second)
                rc1, p0 = pred_x0(t["x"], t["e"], a, s1m, clip, mk())
                rc2, p0c = spec_project(t, R, G, f, lam, p0, mk())
                rc3, xn = dpm_p0(t["x"], p0c, t["d"] if second else None, c, mk())
                assert (rc, rc1, rc2, rc3) == (0, 0, 0, 0), _lib.lib().eod_last_error()
                assert bits_equal(p0c, want_p) and bits_equal(xn, want_x) and bool(torch.isfinite(xn).all())
                _refill(t)
        for noise in (None, t["noise"]):
            a, s1m, _ = _scalars(a_s, a_t, False)
            rc, want_x, want_p = ddim_spec(dict(t, noise=noise), R, G, f, lam, a, np.float32(a_t), sigma, s1m, 0.9)
            rc1, p0 = pred_x0(t["x"], t["e"], a, s1m, False, mk())
            rc2, p0c = spec_project(t, R, G, f, lam, p0, mk())
            rc3, xp = ddim_p0(t["e"], p0c, noise, np.float32(a_t), sigma, 0.9, mk())
            assert (rc, rc1, rc2, rc3) == (0, 0, 0, 0), _lib.lib().eod_last_error()
            assert bits_equal(p0c, want_p) and bits_equal(xp, want_x) and bool(torch.isfinite(xp).all())
            _refill(t)


@pytest.mark.parametrize("factors,plane", [((1, 2, 4), (16, 16)), (CR.S2_FACTORS, (12, 18)), ((3, 6, 8), (24, 24)), ((1, 1, 1), (6, 7))])
def test_fused_equals_unfused_for_the_block_mean_observation(factors, plane):
    t = TC._tensors(factors, *plane, 2, "mixed")
    mk = lambda: _nan(*t["x"].shape)
    for (a_s, a_t), lam, sigma in zip(LEVELS, (1.0, 0.625, 0.3), (0.0, 0.3, 0.005)):
        for second in (False, True):
            for clip in (False, True):
                a, s1m, c = _scalars(a_s, a_t, second)
                rc, want_x, want_p = TC.dpm_obs(t, factors, lam, a, s1m, c, clip, second)
                rc1, p0 = pred_x0(t["x"], t["e"], a, s1m, clip, mk())
                rc2, p0c = obs_project(t, factors, lam, p0, mk())
                rc3, xn = dpm_p0(t["x"], p0c, t["d"] if second else None, c, mk())
                assert (rc, rc1, rc2, rc3) == (0, 0, 0, 0), _lib.lib().eod_last_error()
                assert bits_equal(p0c, want_p) and bits_equal(xn, want_x) and bool(torch.isfinite(xn).all())
                _refill(t)
        for noise in (None, t["noise"]):
            a, s1m, _ = _scalars(a_s, a_t, False)
            rc, want_x, want_p = TC.ddim_obs(dict(t, noise=noise), factors, lam, a, np.float32(a_t), sigma, s1m, 0.9)
            rc1, p0 = pred_x0(t["x"], t["e"], a, s1m, False, mk())
            rc2, p0c = obs_project(t, factors, lam, p0, mk())
            rc3, xp = ddim_p0(t["e"], p0c, noise, np.float32(a_t), sigma, 0.9, mk())
            assert (rc, rc1, rc2, rc3) == (0, 0, 0, 0), _lib.lib().eod_last_error()
            assert bits_equal(p0c, want_p) and bits_equal(xp, want_x)
            _refill(t)


@pytest.mark.parametrize("numel", [77, 4099, 3 * 16 * 16])
def test_the_ends_of_a_chain_have_the_plain_kernels_bits(numel):
    """eod_pred_x0 is eod_dpmpp_step's pred_x0 (clamped or not), and the step from it is that kernel's x_next; the same against eod_ddim_step"""
    x, e, d, z = (synth_input(n, (numel,), 3 + i).to(DEV) for i, n in enumerate(("ex", "ee", "ed", "ez")))
    for (a_s, a_t), sigma in zip(LEVELS, (0.0, 0.3, 0.005)):
        for second in (False, True):
            for clip in (False, True):
                a, s1m, c = _scalars(a_s, a_t, second)
                rc, want_x, want_p = dpmpp(x, e, d if second else None, a, s1m, c, clip)
                rc1, p0 = pred_x0(x, e, a, s1m, clip, _nan(numel))
                rc2, xn = dpm_p0(x, p0, d if second else None, c, _nan(numel))
                assert (rc, rc1, rc2) == (0, 0, 0) and bits_equal(p0, want_p) and bits_equal(xn, want_x)
        for noise in (None, z):
            a, s1m, _ = _scalars(a_s, a_t, False)
            want_x, want_p = _nan(numel), _nan(numel)
            _lib.check(_lib.lib().eod_ddim_step(x.data_ptr(), e.data_ptr(), _lib.ptr(noise), a, float(np.float32(a_t)), sigma, s1m, 0.9,
                                                want_x.data_ptr(), want_p.data_ptr(), numel, _stream()), "eod_ddim_step")
            rc1, p0 = pred_x0(x, e, a, s1m, False, _nan(numel))
            rc2, xp = ddim_p0(e, p0, noise, np.float32(a_t), sigma, 0.9, _nan(numel))
            assert (rc1, rc2) == (0, 0) and bits_equal(p0, want_p) and bits_equal(xp, want_x)


@pytest.mark.parametrize("how", ["weight 0", "mask 0"])
@pytest.mark.parametrize("C,K,f,plane", [(4, 1, 1, (6, 7)), (13, 8, 2, (12, 28)), (3, 3, 3, (12, 18)), (5, 2, 8, (24, 168))])
def test_nothing_observed_gives_the_plain_kernels_bits(C, K, f, plane, how):
    """finite inputs of unit scale (an infinite dot times a zero weight would be a NaN: the formula is what it is)"""
    R, G = _matrices(C, K)
    t = _tensors(C, K, *plane, 2, "full")
    lam = 0.0 if how == "weight 0" else 1.0
    if how == "mask 0":
        t["mask"].zero_()
    n = t["x"].numel()
    for (a_s, a_t), sigma_on in zip(LEVELS, (0.3, 0.3, 0.005)):
        for second in (False, True):
            for clip in (False, True):
                a, s1m, c = _scalars(a_s, a_t, second)
                rc, got_x, got_p = dpm_spec(t, R, G, f, lam, a, s1m, c, clip, second)
                rc2, want_x, want_p = dpmpp(t["x"], t["e"], t["d"] if second else None, a, s1m, c, clip)
                assert rc == 0 and rc2 == 0 and bool(torch.isfinite(want_x).all())
                assert bits_equal(got_x, want_x) and bits_equal(got_p, want_p), (a_s, second, clip)
        for noise, sigma in ((None, 0.0), (t["noise"], sigma_on)):
            a, s1m, _ = _scalars(a_s, a_t, False)
            rc, got_x, got_p = ddim_spec(dict(t, noise=noise), R, G, f, lam, a, np.float32(a_t), sigma, s1m, 0.9)
            want_x, want_p = _nan(*t["x"].shape), _nan(*t["x"].shape)
            _lib.check(_lib.lib().eod_ddim_step(t["x"].data_ptr(), t["e"].data_ptr(), _lib.ptr(noise), a, float(np.float32(a_t)), sigma, s1m, 0.9,
                                                want_x.data_ptr(), want_p.data_ptr(), n, _stream()), "eod_ddim_step")
            assert rc == 0 and bool(torch.isfinite(want_x).all())
            assert bits_equal(got_x, want_x) and bits_equal(got_p, want_p), (a_s, sigma)


@pytest.mark.parametrize("C", [1, 3, 8])
def test_identity_response_at_full_resolution_replaces_the_prediction(C):
    """R = I (K = C, so G = I), f = 1, mask 1, weight 1: d = p0, t = r = p0 - values, pred_x0 = p0 - r IS values wherever the fp32 difference
    p0 - values is exact (the premise of tests/test_gpu_consistency.py's test for factors all 1, evaluated per pixel in float64); the zero
    terms of the dots add +-0 to a finite number and change nothing"""
    I = np.eye(C, dtype=np.float32)
    assert np.array_equal(XR.pinv32(I), I) and XR.rcond(I) == 1.0
    t = _tensors(C, C, 24, 40, 2, "full")
    t["mask"].fill_(1.0)
    t["values"].copy_(torch.round(t["values"] * 4096) / 4096)
    a, s1m, c = _scalars(0.37, 0.61, False)
    rc, p0 = pred_x0(t["x"], t["e"], a, s1m, False, _nan(*t["x"].shape))
    p64, v64 = p0.cpu().double(), t["values"].cpu().double()
    exact = ((p0.cpu() - t["values"].cpu()).double() == p64 - v64)
    assert rc == 0 and float(exact.float().mean()) > 0.25
    for run in (lambda: ddim_spec(dict(t, noise=None), I, I, 1, 1.0, a, 0.61, 0.0, s1m)[2], lambda: dpm_spec(t, I, I, 1, 1.0, a, s1m, c, False, False)[2],
                lambda: spec_project(t, I, I, 1, 1.0, p0)[1]):
        _refill(t)
        got = run()
        assert bits_equal(got.cpu()[exact], t["values"].cpu()[exact])
        assert float((got.cpu() - t["values"].cpu()).abs().max()) <= 2 * EPS * float(p0.abs().max())


def _block_case(C, K, f, plane, B=2, seed=31):
    """block-constant values made from an image, a 0 / 1 mask constant on the blocks"""
    R, G = _matrices(C, K)
    t = _tensors(C, K, *plane, B, "full", seed=seed)
    H, W = plane
    truth = synth_input("qt", (B, C, H, W), seed + 7, uniform=True) * 2 - 1
    cells = (synth_input("qc", (B, 1, H // f, W // f), seed + 8, uniform=True) > 0.4).float()
    t["values"] = XR.apply(truth, R, f).to(DEV)
    t["mask"] = cells.repeat_interleave(f, 2).repeat_interleave(f, 3).contiguous().to(DEV)
    assert 0.0 < float(t["mask"].mean()) < 1.0
    return R, G, t


@pytest.mark.parametrize("C,K,f,plane", [(4, 1, 1, (16, 16)), (13, 8, 2, (12, 28)), (3, 3, 3, (12, 18)), (7, 4, 5, (35, 70)), (5, 2, 8, (24, 168))])
def test_residual_against_the_emulations(C, K, f, plane):
    """max |R (x) D_f pred_x0 - values| over the observed blocks, the operator being eod_spec_apply, against the same figure of the emulation on
    the same inputs with a margin of 4 x, and the emulation's against 3 eps * max(1, |p0|max) (tests/test_spectral_host.py measures at most
    1.5 of that unit on the CPU for these matrices).  Measured on an MI355X: the GPU figure equals the emulation's in every case, at most
    2.50 eps at |p0|max 8.25 (ddim, C = 13, K = 8, f = 2) and 1.03 eps (dpm, clamped)."""
    R, G, t = _block_case(C, K, f, plane)
    x, e, d, values, mask = _cpu(t, "x", "e", "d", "values", "mask")
    a, s1m, c = _scalars(0.37, 0.61, True)
    on = (mask == 1).expand(-1, K, -1, -1)
    for name, run, want, plain in (
            ("ddim", lambda: ddim_spec(dict(t, noise=None), R, G, f, 1.0, a, np.float32(0.61), 0.0, s1m),
             XR.ddim_step(x, e, None, a, 0.61, 0.0, s1m, 1.0, [XR.spec_link(values, R, f, mask, 1.0, G)])[1], XR.pred_x0(x, e, a, s1m)),
            ("dpm", lambda: dpm_spec(t, R, G, f, 1.0, a, s1m, c, True, True),
             XR.dpm_step(x, e, d, a, s1m, *c, True, [XR.spec_link(values, R, f, mask, 1.0, G)])[1], XR.pred_x0(x, e, a, s1m, True))):
        _refill(t)
        rc, _, got = run()
        assert rc == 0 and bits_equal(got.cpu(), want)
        res_gpu = float((spectral_response(got.clone(), R, f).cpu() - values).abs()[on].max())
        res_emu = float((XR.apply(want, R, f) - values).abs()[on].max())
        scale = max(1.0, float(plain.abs().max()))
        print(f"{name} C={C} K={K} f={f}: residual {res_gpu / EPS:.2f} eps on the GPU, {res_emu / EPS:.2f} eps in the emulation, |p0|max {scale:.2f}")
        assert res_emu <= 3 * EPS * scale
        assert res_gpu <= 4 * res_emu
        free = (mask == 0).expand(-1, C, -1, -1)
        assert bits_equal(got.cpu()[free], plain[free])               # a free block keeps the plain prediction


@pytest.mark.parametrize("mode", ["full", "bcast"])
@pytest.mark.parametrize("C,K,f,plane", [(4, 1, 1, (6, 7)), (13, 8, 2, (12, 28)), (3, 3, 3, (12, 18)), (5, 2, 8, (24, 168))])
def test_member_b_of_a_batch_equals_the_launch_on_its_slice(C, K, f, plane, mode):
    R, G = _matrices(C, K)
    t = _tensors(C, K, *plane, 3, mode)
    a, s1m, c = _scalars(0.37, 0.61, True)
    shape = t["x"].shape
    rc, all_x, all_p = dpm_spec(t, R, G, f, 0.75, a, s1m, c, True, True)
    rc2, dd_x, dd_p = ddim_spec(dict(t, out=_nan(*shape), p0=_nan(*shape)), R, G, f, 0.75, a, 0.61, 0.2, s1m)
    rc3, pj = spec_project(t, R, G, f, 0.75, None, _nan(*shape))
    assert (rc, rc2, rc3) == (0, 0, 0)
    for b in range(3):
        one = {k: (v[b:b + 1].contiguous() if v.shape[0] == 3 else v) for k, v in t.items()}
        one["out"], one["p0"] = _nan(1, *shape[1:]), _nan(1, *shape[1:])
        rc, x1, p1 = dpm_spec(one, R, G, f, 0.75, a, s1m, c, True, True)
        assert rc == 0 and bits_equal(x1, all_x[b:b + 1]) and bits_equal(p1, all_p[b:b + 1])
        rc, x1, p1 = ddim_spec(one, R, G, f, 0.75, a, 0.61, 0.2, s1m)
        assert rc == 0 and bits_equal(x1, dd_x[b:b + 1]) and bits_equal(p1, dd_p[b:b + 1])
        rc, j1 = spec_project(one, R, G, f, 0.75, None, _nan(1, *shape[1:]))
        assert rc == 0 and bits_equal(j1, pj[b:b + 1])


def test_bad_arguments_return_the_error_and_leave_the_outputs_alone():
    C, K, f = 3, 2, 2
    R, G = _matrices(C, K)
    t = _tensors(C, K, 16, 16, 2, "full")
    a, s1m, c = _scalars(0.37, 0.61, True)
    n = t["x"].numel()
    buf = _nan(2 * n)
    shape = t["x"].shape
    calls = []
    L = _lib.lib()

    def run_dpm(tt, R=R, G=G, f=f, lam=1.0, a_s=a):
        calls.append(dpm_spec(tt, R, G, f, lam, a_s, s1m, c, False, True)[0])

    def run_ddim(tt, R=R, G=G, f=f, lam=1.0, a_s=a):
        calls.append(ddim_spec(tt, R, G, f, lam, a_s, 0.61, 0.0, s1m)[0])

    def run_project(tt, R=R, G=G, f=f, lam=1.0, a_s=a):
        calls.append(spec_project(tt, R, G, f, lam)[0])

    for run in (run_dpm, run_ddim, run_project):
        for bad_f in (0, 9, -1, 3, 5, 7):                                                 # outside 1 .. 8; 3, 5, 7 do not divide 16
            run(t, f=bad_f)
        for lam in (-0.25, 1.5, float("nan"), float("inf")):
            run(t, lam=lam)
        if run is not run_project:
            for a_s in (0.0, -0.1, 1.5, float("nan")):
                run(t, a_s=a_s)
        for k in ("x", "e", "d", "noise", "values", "mask"):                              # an output on top of an input
            if (k == "d" and run is not run_dpm) or (k == "noise" and run is not run_ddim) or (k == "e" and run is run_project):
                continue
            if k in ("values", "mask"):                                                   # (fewer planes than the state: a partial overlap, inside buf)
                over = {k: buf[n - 4:n - 4 + t[k].numel()].view(t[k].shape)}
                run(dict(t, out=buf[:n].view(shape), **over))
                if run is not run_project:
                    run(dict(t, p0=buf[:n].view(shape), **over))
                continue
            run(dict(t, out=t[k]))
            if run is not run_project:
                run(dict(t, p0=t[k]))
        if run is not run_project:
            run(dict(t, out=buf[:n].view(shape), p0=buf[n // 2:n // 2 + n].view(shape)))    # the two outputs overlap
    # limits of the matrix: K = 0, K > C, K > 8, C > 32 (the shapes say so; nothing may be read before the refusal)
    wide = _tensors(3, 2, 4, 4, 1, "nomask")
    for K_bad, C_bad in ((0, 3), (4, 3), (9, 16), (1, 33)):
        Rb = np.ones((max(K_bad, 1), C_bad), np.float32)
        tt = dict(wide, x=t["x"].view(-1)[:C_bad * 16].view(1, C_bad, 4, 4), e=t["e"].view(-1)[:C_bad * 16].view(1, C_bad, 4, 4))
        tail = (tt["values"].data_ptr(), 0, 1.0, _mat(Rb), _mat(Rb.T), K_bad, 1, 1, C_bad, 4, 4, 0, 0)
        calls.append(L.eod_spec_project(tt["x"].data_ptr(), *tail, t["out"].data_ptr(), _stream()))
        calls.append(L.eod_dpmpp_step_spec(tt["x"].data_ptr(), tt["e"].data_ptr(), 0, a, s1m, *(float(v) for v in c), 0, *tail, t["out"].data_ptr(),
                                           t["p0"].data_ptr(), _stream()))
        calls.append(L.eod_spec_apply(tt["x"].data_ptr(), _mat(Rb), K_bad, 1, t["out"].data_ptr(), 1, C_bad, 4, 4, _stream()))
    x = t["x"]
    tail = _tail(t, R, G, f, 1.0)
    calls.append(L.eod_spec_project(0, *tail, t["out"].data_ptr(), _stream()))                                       # null pointers
    calls.append(L.eod_spec_project(x.data_ptr(), *tail, 0, _stream()))
    calls.append(L.eod_spec_project(x.data_ptr(), 0, *tail[1:], t["out"].data_ptr(), _stream()))
    calls.append(L.eod_spec_project(x.data_ptr(), *tail[:3], None, tail[4], *tail[5:], t["out"].data_ptr(), _stream()))
    calls.append(L.eod_spec_project(x.data_ptr(), *tail[:4], None, *tail[5:], t["out"].data_ptr(), _stream()))
    calls.append(L.eod_spec_apply(x.data_ptr(), _mat(R), K, f, x.data_ptr(), *shape, _stream()))                      # out on top of x
    calls.append(L.eod_spec_apply(x.data_ptr(), None, K, f, t["out"].data_ptr(), *shape, _stream()))
    calls.append(L.eod_spec_apply(x.data_ptr(), _mat(R), K, 3, t["out"].data_ptr(), *shape, _stream()))
    # the ends of a chain and section 9.5's projection of a given p
    calls.append(pred_x0(x, t["e"], 0.0, s1m, 0, t["out"])[0])
    calls.append(pred_x0(x, t["e"], float("nan"), s1m, 0, t["out"])[0])
    calls.append(pred_x0(x, t["e"], a, s1m, 0, x)[0])
    calls.append(pred_x0(x, t["e"], a, s1m, 0, t["e"])[0])
    calls.append(L.eod_pred_x0(x.data_ptr(), 0, a, s1m, 0, t["out"].data_ptr(), n, _stream()))
    calls.append(L.eod_pred_x0(x.data_ptr(), t["e"].data_ptr(), a, s1m, 0, t["out"].data_ptr(), 0, _stream()))
    for k in ("e", "d", "noise"):
        calls.append(ddim_p0(t["e"], t["d"], t["noise"], 0.61, 0.2, 1.0, t[k])[0])
        calls.append(dpm_p0(t["e"], t["noise"], t["d"], c, t[k])[0])
    calls.append(L.eod_ddim_step_p0(0, t["d"].data_ptr(), 0, 0.61, 0.0, 1.0, t["out"].data_ptr(), n, _stream()))
    calls.append(L.eod_dpmpp_step_p0(x.data_ptr(), 0, 0, *(float(v) for v in c), t["out"].data_ptr(), n, _stream()))
    to = TC._tensors((1, 2, 4), 16, 16, 2, "full")
    for fs, lam, p, out in (((1, 2, 9), 1.0, to["x"], to["out"]), ((1, 2, 3), 1.0, to["x"], to["out"]), ((1, 2, 4), 1.5, to["x"], to["out"]),
                            ((1, 2, 4), float("nan"), to["x"], to["out"]), ((1, 2, 4), 1.0, to["x"], to["x"]), ((1, 2, 4), 1.0, to["x"], to["values"]),
                            ((1, 2, 4), 1.0, to["x"], to["mask"])):
        calls.append(obs_project(to, fs, lam, p, out)[0])
    torch.cuda.synchronize()
    assert calls and all(rc == -1 for rc in calls), calls
    for z in (t["out"], t["p0"], buf, to["out"]):
        assert bool(torch.isnan(z).all())
    for z, name in ((t["x"], "qx"), (t["e"], "qe"), (t["d"], "qd"), (t["noise"], "qn")):                             # (no input was written)
        assert bool(torch.isfinite(z).all())
    with pytest.raises(EodError):
        _lib.check(spec_project(t, R, G, 9, 1.0)[0], "eod_spec_project")


# ------------------------------------------------------------------------------------------------------------ 3. whole calls
T_CALL, S_CALL = TC.T_CALL, TC.S_CALL
VARIANTS = TC.VARIANTS
PAN3 = np.array([[0.3, 0.5, 0.2]], np.float32)
FORMS = ("spec", "chain")


def _links(form, shape, n_eval, seed, consistent=False):
    """the observations of a call on a state of `shape` = (B, 3, H, W) as plain data: form "spec": K = 2 bands at f = 2 under a block mask;
    "chain": [a pan band at f = 1, the three bands at f = 4 under a block mask].  One weight per evaluation and link (consistent: 1,
    no masks, both links made from ONE truth image)."""
    B, C, H, W = shape
    truth = synth_input("lt", shape, seed, uniform=True) * 2 - 1
    w_down = [float(np.float32(w)) for w in np.linspace(1.0, 0.5, n_eval)]
    w_up = [float(np.float32(w)) for w in np.linspace(0.25, 1.0, n_eval)]
    if consistent:
        w_down = w_up = [1.0] * n_eval
    cells = lambda c, L, tag: (synth_input(tag, (B, c, H // L, W // L), seed, uniform=True) > 0.3).float().repeat_interleave(L, 2).repeat_interleave(L, 3).contiguous()
    if form == "spec":
        R = XR.response(2, 3, seed)
        assert XR.rcond(R) >= XR.MIN_RCOND
        return [dict(kind="spec", values=XR.apply(truth, R, 2), R=R, f=2, mask=cells(1, 2, "lc"), weights=w_down)]
    assert XR.rcond(PAN3) >= XR.MIN_RCOND
    return [dict(kind="spec", values=XR.apply(truth, PAN3, 1), R=PAN3, f=1, mask=None, weights=w_up),
            dict(kind="obs", values=CR.block_mean(truth, (4, 4, 4)), factors=(4, 4, 4), mask=None if consistent else cells(3, 4, "ld"), weights=w_down)]


def _observation(links, sl=None, per_evaluation=True):
    """the product's objects for the links (sl: a function that cuts values / mask, for tiles and members)"""
    sl = sl or (lambda z: z)
    out = []
    for l in links:
        m = None if l["mask"] is None else sl(l["mask"])
        w = l["weights"] if per_evaluation else l["weights"][0]
        out.append(SpectralObservation(sl(l["values"]), l["R"], l["f"], m, w) if l["kind"] == "spec" else Observation(sl(l["values"]), l["factors"], m, w))
    return out[0] if len(out) == 1 else out


def _cpu_links(links, k):
    return [XR.spec_link(l["values"], l["R"], l["f"], l["mask"], l["weights"][k]) if l["kind"] == "spec"
            else XR.obs_link(l["values"], l["factors"], l["mask"], l["weights"][k]) for l in links]


def _call_case(form, n_lv, masked=False, resample=None, seed=91):
    c = TC._call_case(n_lv, masked, resample, seed)
    c["links"] = _links(form, (2, 3, 16, 16), len(c["obs"]["weights"]), seed)
    return c


@functools.lru_cache(maxsize=None)
def _ddim_reference(form, variant):
    from oracle import schedule as SCH
    steps = TC._ddim_steps()
    c = _call_case(form, len(steps), **VARIANTS[variant])
    dd = SCH.ddim_tables(TC._tables()["alphas_cumprod"], steps, 0.5)
    _, _, eps = _eps_tiny()
    return XR.ddim_sampled(TC._tables(), dd, steps, eps, c["x_T"], c["step_noises"], lambda k: _cpu_links(c["links"], k), c.get("x0"), c.get("mask"),
                           c.get("mix_noises"), VARIANTS[variant].get("resample"), c["jump_noises"])


@functools.lru_cache(maxsize=None)
def _dpm_reference(form, variant, clip, observed=True):
    levels = TC._dpm_levels()
    c = _call_case(form, len(levels), **VARIANTS[variant])
    _, _, eps = _eps_tiny()
    links = c["links"] if observed else []
    return XR.dpm_sampled(TC._tables(), levels, eps, c["x_T"], lambda k: _cpu_links(links, k), 2, clip, c.get("x0"), c.get("mask"), c.get("mix_noises"),
                          VARIANTS[variant].get("resample"), c["jump_noises"])


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS)
def test_ddim_call_vs_cpu_loop(form, variant, prec):
    """8 evaluations (more with resample = (2, 2)) of T = 1000 on u_a0_tiny, batch 2, eta 0.5, one weight per evaluation and link; plain, with
    the RePaint mix of a known region, with resampling.  The CPU loop: the oracle UNet and the emulated steps."""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    steps = TC._ddim_steps()
    kw = VARIANTS[variant]
    c = _call_case(form, len(steps), **kw)
    ref, ref_p0 = _ddim_reference(form, variant)
    smp = DDIMSampler(_model(prec, T=T_CALL))
    extra = dict(x0=c["x0"].to(DEV), mask=c["mask"].to(DEV), mix_noises=c["mix_noises"]) if kw.get("masked") else {}
    out, inter = smp.sample(S_CALL, 2, (3, 16, 16), eta=0.5, verbose=False, progress=False, log_every_t=1, x_T=c["x_T"], step_noises=c["step_noises"],
                            resample=kw.get("resample"), jump_noises=c["jump_noises"], observation=_observation(c["links"]), **extra)
    assert len(inter["pred_x0"]) == 1 + len(c["links"][0]["weights"])
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DDIM + {form}, {variant} [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS)
def test_dpm_call_vs_cpu_loop(form, variant, clip, prec):
    """the same for DPMSolverSampler.sample, order 2: the history is the chain's final prediction; after a jump it is dropped"""
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    levels = TC._dpm_levels()
    kw = VARIANTS[variant]
    c = _call_case(form, len(levels), **kw)
    ref, ref_p0 = _dpm_reference(form, variant, clip)
    smp = DPMSolverSampler(_model(prec, T=T_CALL))
    extra = dict(x0=c["x0"].to(DEV), mask=c["mask"].to(DEV), mix_noises=c["mix_noises"]) if kw.get("masked") else {}
    out, inter = smp.sample(S_CALL, 2, (3, 16, 16), clip_denoised=clip, x_T=c["x_T"], resample=kw.get("resample"), jump_noises=c["jump_noises"],
                            progress=False, log_every_t=1, observation=_observation(c["links"]), **extra)
    assert np.array_equal(smp.dpm_timesteps, levels) and len(inter["pred_x0"]) == 1 + len(c["links"][0]["weights"])
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DPM-Solver++ + {form}, {variant}, clip {clip} [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} "
          f"(gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]
    assert rel_l2(_dpm_reference(form, variant, clip, False)[0], ref) > 10 * TRAJ_TOL["fp32"]       # (the observation matters)


def _record(smp, which):
    """wraps the sampler's update so that its arguments are kept: returns the list"""
    seen = []
    name = "_ddim_update" if which == "ddim" else "_dpm_update"
    inner = getattr(smp, name)
    setattr(smp, name, lambda *a: (seen.append(a), inner(*a))[1])
    return seen


def _emulate_last(smp, which, seen, links, k):
    """the emulated step on the recorded inputs of the call's last evaluation (number k): (x, pred_x0)"""
    if which == "ddim":
        x, e_t, noise, index, temperature, obs = seen[-1]
        return XR.ddim_step(x.cpu(), e_t.cpu(), None if noise is None else noise.cpu(), smp.ddim_alphas[index], smp.ddim_alphas_prev[index],
                            smp.ddim_sigmas[index], smp.ddim_sqrt_one_minus_alphas[index], temperature, _cpu_links(links, k))
    x, e_t, hist, index, clip, obs = seen[-1]
    assert index == 0                                              # (lower-order final: first order)
    return XR.dpm_step(x.cpu(), e_t.cpu(), None, smp.ddim_alphas[index], smp.dpm_sqrt_one_minus_alphas[index], *smp.dpm_first[index], clip,
                       _cpu_links(links, k))


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_on_consistent_data_the_last_prediction_meets_both_observations(which):
    """the chain [pan at f = 1, bands at f = 4] made from ONE truth image, weights 1, no masks: the last evaluation's pred_x0 equals the
    emulated unfused step on its recorded inputs bit for bit, and its two residuals, measured with eod_spec_apply / eod_block_mean, are
    within 4 x the emulation's (which tests/test_spectral_host.py holds to 1e-12 in float64: the projections commute there).  Measured on
    an MI355X: (pan, bands) = 4.75, 4.62 eps for ddim and 4.00, 2.38 eps for dpm at |p0|max 18, the same in the emulation."""
    smp = TC._samplers(_model("fp32x3", T=T_CALL))[which]
    n = len(TC._ddim_steps()) if which == "ddim" else len(TC._dpm_levels())
    c = TC._call_case(n)
    links = _links("chain", (2, 3, 16, 16), n, 93, consistent=True)
    seen = _record(smp, which)
    kw = dict(eta=0.0, verbose=False, step_noises=c["step_noises"]) if which == "ddim" else dict(clip_denoised=False)
    out, inter = smp.sample(S_CALL, 2, (3, 16, 16), x_T=c["x_T"], progress=False, observation=_observation(links, per_evaluation=False), **kw)
    assert len(seen) == n
    got = inter["pred_x0"][-1]
    want_x, want = _emulate_last(smp, which, seen, links, n - 1)
    assert bits_equal(got.cpu(), want) and bits_equal(out.cpu(), want_x)
    pan, bands = links[0]["values"], links[1]["values"]
    res_gpu = (float((spectral_response(got, PAN3, 1).cpu() - pan).abs().max()), float((block_mean(got, (4, 4, 4)).cpu() - bands).abs().max()))
    res_emu = (float((XR.apply(want, PAN3, 1) - pan).abs().max()), float((CR.block_mean(want, (4, 4, 4)) - bands).abs().max()))
    print(f"{which}, consistent chain: residuals (pan, bands) {res_gpu[0] / EPS:.2f}, {res_gpu[1] / EPS:.2f} eps on the GPU; "
          f"{res_emu[0] / EPS:.2f}, {res_emu[1] / EPS:.2f} eps in the emulation; |p0|max {float(want.abs().max()):.2f}")
    assert res_gpu[0] <= 4 * res_emu[0] and res_gpu[1] <= 4 * res_emu[1]
    # both hold at once.  The last link's own residual is under the 3 eps of tests/test_spectral_host.py; the first link's is its own 3 eps,
    # plus what the second link's rounding moves it by: the fp32 block sum of 16 terms (15 adds of half an ulp) enters every t_c, and one
    # more rounding each for mean - values, lm * t and p0 - t; the rows of R sum to one: 3 + 7.5 + 1.5 = 12 eps of the largest magnitude
    x, e_t, index = seen[-1][0].cpu(), seen[-1][1].cpu(), seen[-1][3]
    s1m = smp.ddim_sqrt_one_minus_alphas[index] if which == "ddim" else smp.dpm_sqrt_one_minus_alphas[index]
    scale = max(1.0, float(want.abs().max()), float(XR.pred_x0(x, e_t, smp.ddim_alphas[index], s1m).abs().max()))
    assert max(res_emu) <= 12 * EPS * scale


def _today_ddim_update(self, x, e_t, noise, index, temperature, obs=None):
    """DDIMSampler._ddim_update as it was before chains existed: eod_ddim_step, or eod_ddim_step_obs through the test's own binding"""
    from eo_diffusion_amd.engine import f32c
    if obs is None:
        return TC._parent_ddim_update(self, x, e_t, noise, index, temperature)
    o, i = obs
    t = dict(x=f32c(x), e=f32c(e_t), noise=noise, values=o.values, mask=o.mask, out=torch.empty_like(x), p0=torch.empty_like(x))
    rc, x_prev, p0 = TC.ddim_obs(t, o.factors, o.weights[i], self.ddim_alphas[index], self.ddim_alphas_prev[index], self.ddim_sigmas[index],
                                 self.ddim_sqrt_one_minus_alphas[index], temperature)
    assert rc == 0
    return x_prev, p0


def _today_dpm_update(self, x, e_t, hist, index, clip, obs=None):
    from eo_diffusion_amd.engine import f32c
    if obs is None:
        return TC._parent_dpm_update(self, x, e_t, hist, index, clip)
    o, i = obs
    second = self.dpm_second[index] if hist is not None and hist[0] == index + 1 else None
    c = self.dpm_first[index] if second is None else second
    t = dict(x=f32c(x), e=f32c(e_t), d=None if second is None else hist[1], values=o.values, mask=o.mask, out=torch.empty_like(x), p0=torch.empty_like(x))
    rc, x_next, p0 = TC.dpm_obs(t, o.factors, o.weights[i], self.ddim_alphas[index], self.dpm_sqrt_one_minus_alphas[index], c, clip, second is not None)
    assert rc == 0
    return x_next, p0


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_none_a_bare_observation_and_a_list_of_one_take_the_direct_paths(which):
    """observation=None and a bare Observation against the same call with the update replaced by the direct eod_ddim_step /
    eod_ddim_step_obs (eod_dpmpp_step / eod_dpmpp_step_obs) launches of the version before; a list of one (of either kind) against the
    bare object; and a chain whose weights are all 0 against the call without an observation"""
    import types
    m = _model("fp32x3", T=T_CALL)
    n = len(TC._ddim_steps()) if which == "ddim" else len(TC._dpm_levels())
    c = TC._call_case(n)
    bare = TC._observation(c["obs"])
    spec = _observation(_links("spec", (2, 3, 16, 16), n, 94))
    chain = _links("chain", (2, 3, 16, 16), n, 94)

    def run(direct, **kw):
        smp = TC._samplers(m)[which]
        if direct:
            name, fn = ("_ddim_update", _today_ddim_update) if which == "ddim" else ("_dpm_update", _today_dpm_update)
            setattr(smp, name, types.MethodType(fn, smp))
        if which == "ddim":
            return smp.sample(S_CALL, 2, (3, 16, 16), eta=0.5, verbose=False, progress=False, x_T=c["x_T"], step_noises=c["step_noises"], **kw)[0]
        return smp.sample(S_CALL, 2, (3, 16, 16), clip_denoised=True, x_T=c["x_T"], progress=False, **kw)[0]

    free = run(True)
    assert bool(torch.isfinite(free).all()) and torch.equal(run(False), free) and torch.equal(run(False, observation=None), free)
    want = run(True, observation=bare)
    got = run(False, observation=bare)
    assert torch.equal(got, want) and not torch.equal(got, free)
    assert torch.equal(run(False, observation=[bare]), got) and torch.equal(run(False, observation=(bare,)), got)
    one = run(False, observation=spec)
    assert torch.equal(run(False, observation=[spec]), one) and not torch.equal(one, free)
    zero = _observation([dict(l, weights=[0.0] * n) for l in chain])
    assert torch.equal(run(False, observation=zero), free)
    assert not torch.equal(run(False, observation=_observation(chain)), free)


# ------------------------------------------------------------------------------------------------------------ 4. scenes
def _scene_links(form, H, W, n, seed, B=1, fs=(2, (2, 4, 8))):
    """_links for a scene: form "spec": K = 2 at f = fs[0]; "chain": [pan at f = 1, the bands at factors fs[1]]"""
    shape = (B, 3, H, W)
    truth = synth_input("st", shape, seed, uniform=True) * 2 - 1
    w = [float(np.float32(v)) for v in np.linspace(1.0, 0.25, n)]
    if form == "spec":
        R, f = XR.response(2, 3, seed), fs[0]
        cells = (synth_input("sc", (B, 1, H // f, W // f), seed, uniform=True) > 0.3).float()
        return [dict(kind="spec", values=XR.apply(truth, R, f), R=R, f=f, mask=cells.repeat_interleave(f, 2).repeat_interleave(f, 3).contiguous(), weights=w)]
    values, mask = TC._scene_obs(H, W, fs[1], seed, B)
    return [dict(kind="spec", values=XR.apply(truth, PAN3, 1), R=PAN3, f=1, mask=None, weights=w[::-1]),
            dict(kind="obs", values=values, factors=fs[1], mask=mask, weights=w)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_scene_with_overlap_0_equals_sample_on_the_tiles(which, form):
    s, S, H, W = 16, 6, 32, 48
    smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))[which]
    plan = TilePlan(H, W, s, 0)
    n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 7
    links = _scene_links(form, H, W, n, 85)                           # every factor divides the tile: no block crosses a tile border
    kw = TC._scene_kw(which, n, H, W, 85)
    scene, inter = smp.sample_scene(S, (H, W), progress=False, observation=_observation(links), **kw)
    tile_kw = {k: (cut(v, plan) if k == "x_T" else torch.stack([cut(z, plan) for z in v]) if k == "step_noises" else v) for k, v in kw.items()}
    tiles, inter_t = smp.sample(S, plan.n_tiles, (3, s, s), progress=False, observation=_observation(links, lambda z: cut(z, plan)), **tile_kw)
    assert smp.ddim_timesteps.shape[0] == n and bool(torch.isfinite(scene).all())
    assert torch.equal(scene, stitch(tiles, plan)) and torch.equal(inter["pred_x0"][-1], stitch(inter_t["pred_x0"][-1], plan))
    free, _ = smp.sample_scene(S, (H, W), progress=False, **kw)
    assert not torch.equal(free, scene)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_a_block_across_a_tile_border_equals_the_emulation_on_the_recorded_inputs(which, form):
    """overlap 8, tile 16, scene 24 x 36: tile edges at x = 8, 16, 20, 24, 32; blocks of edge 6 are cut by them (asserted from the plan).  The
    scene-level step is one pass (a chain: four) over the scene: its recorded inputs go through the emulation, which it equals bit for bit"""
    s, S, H, W = 16, 5, 24, 36
    plan = TilePlan(H, W, s, 8)
    edges = sorted({int(o) for o in plan.origins_x} | {int(o) + s for o in plan.origins_x})
    assert any(e % 6 for e in edges if 0 < e < W) and len(plan.origins_x) > 2
    smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))[which]
    n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
    links = _scene_links(form, H, W, n, 86, fs=(6, (4, 6, 1)))
    seen = _record(smp, which)
    scene, inter = smp.sample_scene(S, (H, W), overlap=8, progress=False, observation=_observation(links), **TC._scene_kw(which, n, H, W, 86))
    assert len(seen) == n and seen[-1][0].shape == (1, 3, H, W) and seen[-1][-1] is not None
    want_x, want = _emulate_last(smp, which, seen, links, n - 1)
    assert bits_equal(inter["pred_x0"][-1].cpu(), want) and bits_equal(scene.cpu(), want_x)


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_member_b_of_a_stack_equals_the_single_scene_call(which):
    s, S, H, W, B = 16, 5, 24, 36, 2
    smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))[which]
    n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
    links = _scene_links("chain", H, W, n, 87, B, fs=(6, (4, 6, 1)))
    kw = TC._scene_kw(which, n, H, W, 87, B)
    stack, inter = smp.sample_scene(S, (H, W), overlap=8, progress=False, n_scenes=B, observation=_observation(links), **kw)
    shared, _ = smp.sample_scene(S, (H, W), overlap=8, progress=False, n_scenes=B, observation=_observation(links, lambda z: z[:1]), **kw)
    assert stack.shape == (B, 3, H, W) and bool(torch.isfinite(stack).all())
    for b in range(B):
        one_kw = {k: (v[b:b + 1] if k == "x_T" else v[:, b:b + 1] if k == "step_noises" else v) for k, v in kw.items()}
        one, inter1 = smp.sample_scene(S, (H, W), overlap=8, progress=False, observation=_observation(links, lambda z: z[b:b + 1]), **one_kw)
        assert torch.equal(stack[b:b + 1], one) and torch.equal(inter["pred_x0"][-1][b:b + 1], inter1["pred_x0"][-1])
    assert torch.equal(shared[:1], stack[:1]) and not torch.equal(shared[1:], stack[1:])


def test_refusals_come_before_any_launch():
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    s, T, S, H, W = 16, 20, 5, 32, 48
    m = EODiffusion(Never(), timesteps=T, image_size=s, in_channels=3, device=DEV).to(DEV)
    z = torch.zeros
    pan = lambda *shape, **kw: SpectralObservation(z(*shape), PAN3, **kw)
    ok, ok_obs = pan(1, 1, H, W), Observation(z(1, 3, H, W), (1, 2, 4))
    with Calls(m.model) as calls:
        for which, smp in TC._samplers(m).items():
            n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
            extra = dict(verbose=False) if which == "ddim" else {}
            for kw in (dict(observation=ok, skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)),       # skip_known + observation
                       dict(observation=[ok, ok_obs], skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)),
                       dict(observation=[ok_obs], skip_known=True),
                       dict(observation=pan(1, 1, 32, 32)),                                                  # not scene-sized
                       dict(observation=[ok_obs, pan(1, 1, 32, 32)]),
                       dict(observation=SpectralObservation(z(1, 1, H, W), [[0.25, 0.25, 0.25, 0.25]])),     # mixes 4 channels, the state has 3
                       dict(observation=pan(2, 1, H, W)),                                                    # leading dimension 2, one scene
                       dict(observation=pan(3, 1, H, W), n_scenes=2),
                       dict(observation=pan(1, 1, H, W, mask=z(2, 1, H, W))),
                       dict(observation=pan(1, 1, H, W, weight=[1.0] * (n + 1))),                            # weights against the walk
                       dict(observation=[ok_obs, pan(1, 1, H, W, weight=[1.0] * n)], resample=(2, 2)),
                       dict(observation=[]), dict(observation=[ok] * 5), dict(observation=[ok, None]), dict(observation=[[ok]]),
                       dict(observation="values")):
                with pytest.raises(EodError):
                    smp.sample_scene(S, (H, W), progress=False, **extra, **kw)
            for kw in (dict(observation=ok), dict(observation=[ok_obs, ok]), dict(observation=pan(3, 1, s, s)),
                       dict(observation=[pan(2, 1, s, s, weight=[0.5] * (n - 1))]),
                       dict(observation=[pan(2, 1, s, s), Observation(z(2, 3, s, s), (1, 2, 4), weight=[0.5] * n)], resample=(2, 2))):
                with pytest.raises(EodError):
                    smp.sample(S, 2, (3, s, s), progress=False, **extra, **kw)
    assert calls.batches == []
