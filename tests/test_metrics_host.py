"""CPU: the image-quality metrics (eo_diffusion_amd/metrics.py, csrc/metrics.hip) as far as they need no GPU: the
float64 emulation of eod_ssim (tests/metrics_ref.py) against the published definition in oracle/harness_ref.py, the fp32 raw-moment
evaluation that misses it (the reason the kernel is float64 inside), the host formulas of quality() against closed forms, hole_of, every
refusal, the signatures, and the tile body of eod_ssim compiled for the host and walked under the address and undefined-behaviour
sanitizers as a stand-alone program."""
import ast
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd import metrics as M
from eo_diffusion_amd._lib import EodError
from oracle import harness_ref as R
from tests import metrics_ref as MR
from tests.synth import synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_bright():
    """a flat band of value 0.9 with 1e-3 noise, 2 x 3 x 48 x 40: cloud, snow, water"""
    shape = (2, 3, 48, 40)
    return (0.9 + 1e-3 * synth_input("mh_fp", shape, 3, uniform=True)), (0.9 + 1e-3 * synth_input("mh_ft", shape, 4, uniform=True))


def _smooth(shape, seed):
    B, C, H, W = shape
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = 0.5 + 0.4 * torch.sin(0.13 * y + 0.1 * seed) * torch.cos(0.09 * x)
    return f.expand(B, C, H, W).contiguous()


def _ssim_inputs():
    shape = (2, 3, 40, 48)
    gt = synth_input("mh_gt", shape, 1, uniform=True)
    yield "noise01", (gt + 0.05 * synth_input("mh_nz", shape, 2)).clip(0, 1), gt, 1.0
    yield "smooth", _smooth(shape, 0) + 0.01 * synth_input("mh_sn", shape, 5), _smooth(shape, 1), 1.0
    sg = synth_input("mh_sg", shape, 6, uniform=True) * 2 - 1
    yield "pm1", (sg + 0.1 * synth_input("mh_sz", shape, 7)).clip(-1, 1), sg, 2.0
    yield ("flat_bright",) + _flat_bright() + (1.0,)
    big = synth_input("mh_bg", shape, 8, uniform=True) * 1e4
    yield "range1e4", (big + 300.0 * synth_input("mh_bz", shape, 9)).clip(0, 1e4), big, 1e4


@pytest.mark.parametrize("name,pred,gt,rng", list(_ssim_inputs()), ids=[c[0] for c in _ssim_inputs()])
def test_ssim_emulation_against_the_oracle(name, pred, gt, rng):
    """the kernel's documented arithmetic (valid region, taps in sequence, float64) is the published definition to 1e-9, the gate
    tests/test_gpu_harness.py holds the host evaluation to; measured: at most 1.1e-14 over these inputs"""
    got, want = MR.ssim_mean(pred, gt, rng), R.ssim(pred, gt, rng)
    print(f"{name}: |emulation - oracle| = {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-9
    assert MR.ssim_mean(gt, gt, rng) == 1.0 and bool((MR.ssim_map(gt, gt, MR.gauss(), (0.01 * rng) ** 2, (0.03 * rng) ** 2) == 1.0).all())


def test_fp32_raw_moments_miss_the_definition_on_a_flat_bright_band():
    """why eod_ssim is float64 inside: E[x^2] - mu^2 cancels in fp32.  The same sequence of operations in fp32 misses 1e-6 on the flat
    bright band (measured: 5.3e-4 at the worst pixel, 1.1e-4 mean |error| per pixel; the errors are of both signs and the image mean is off by
    6e-7 on this draw); the float64 sequence holds 1e-9 (measured 1.1e-14)."""
    pred, gt = _flat_bright()
    g = [float(v) for v in MR.gauss().astype(np.float32)]
    p, t = pred.float(), gt.float()
    Ep, Et, Epp, Ett, Ept = (MR.blur(q, g) for q in (p, t, p * p, t * t, p * t))
    assert Ep.dtype == torch.float32
    c1, c2 = np.float32(0.01 ** 2), np.float32(0.03 ** 2)
    m32 = ((2 * (Ep * Et) + c1) * (2 * (Ept - Ep * Et) + c2)) / (((Ep * Ep + Et * Et) + c1) * (((Epp - Ep * Ep) + (Ett - Et * Et)) + c2))
    want = R.ssim(pred, gt)
    err = (m32.double() - MR.ssim_map(pred, gt, MR.gauss(), 0.01 ** 2, 0.03 ** 2)).abs()     # per pixel, against the float64 map
    miss = abs(float(m32.double().reshape(2, -1).mean(-1).mean()) - want)
    print(f"fp32 raw moments: worst pixel {float(err.max()):.3e}, mean |error| {float(err.mean()):.3e}, error of the mean {miss:.3e} "
          f"(the signs cancel); float64: {abs(MR.ssim_mean(pred, gt) - want):.3e}")
    assert float(err.max()) > 1e-6 and float(err.mean()) > 1e-6
    assert abs(MR.ssim_mean(pred, gt) - want) <= 1e-9


def _quality(pred, ref, where=None, aff=(1.0, 0.0), data_range=1.0, ratio=None):
    """metrics.quality's host arithmetic on the emulated tables (no SSIM)"""
    band, _ = MR.band_stats(pred, ref, where, *aff)
    sample, _ = MR.sample_stats(pred, ref, where, *aff)
    return M._derive(band.numpy(), sample.numpy(), None, data_range, ratio)


def test_psnr_all_against_the_oracle():
    gt = synth_input("mh_pg", (3, 5, 24, 20), 1, uniform=True)
    pred = (gt + 0.05 * synth_input("mh_pn", (3, 5, 24, 20), 2)).clip(0, 1)
    q = _quality(pred, gt)
    for b in range(3):
        want = R.psnr(pred[b:b + 1], gt[b:b + 1])
        assert abs(q.psnr_all[b] - want) <= 1e-12 * abs(want)
    q = _quality(pred * 2 - 1, gt * 2 - 1, data_range=2.0)
    assert abs(q.psnr_all[1] - R.psnr(pred[1:2] * 2 - 1, gt[1:2] * 2 - 1, 2.0)) <= 1e-12 * q.psnr_all[1]
    same = _quality(gt, gt)
    assert np.isinf(same.psnr).all() and np.isinf(same.psnr_all).all() and (same.rmse == 0).all() and (same.sam_deg == 0).all()


def test_closed_forms_scaled_truth():
    """pred = k ref: the angle is exactly 0 where the scaling is exact in fp32 (k = 2; for k = 1.1 it is 0 to rounding), cc = 1,
    uiqi = 2k / (1 + k^2) ... and ERGAS = 100 / ratio * |k - 1| * sqrt(mean_c(E[t_c^2] / mu_c^2))"""
    ref = 0.1 + synth_input("mh_cr", (2, 4, 16, 12), 1, uniform=True)
    assert (_quality(2.0 * ref, ref).sam_deg == 0.0).all()                      # bit-proportional spectra: exactly 0
    k = 1.1
    pred = (k * ref.double())                                                   # float64 product, handed over as float64: exact inputs
    band, _ = MR.band_stats(pred, ref)
    sample, _ = MR.sample_stats(pred, ref)
    q = M._derive(band.numpy(), sample.numpy(), None, 1.0, 2.0)
    t = ref.double().numpy()
    mu, e2 = t.mean((2, 3)), (t * t).mean((2, 3))
    var = e2 - mu * mu
    # The closed form is 0.  In floating point pp * tt and dot * dot are equal only where k * t is exact: each of pp, tt, dot carries C
    # roundings of 2^-53 and the two products one more each, so w <= (4 C + 2) 2^-53 pp tt and theta <= sqrt((4 C + 2) 2^-53) rad = 4.5e-8.
    print(f"sam of 1.1 * ref: {np.abs(q.sam_deg).max():.3e} degrees")
    assert np.abs(q.sam_deg).max() <= np.degrees(np.sqrt((4 * 4 + 2) * 2.0 ** -53))
    assert np.abs(q.cc - 1.0).max() <= 1e-12
    # uiqi = 4 (k var) (k mu^2) / ((1 + k^2) var (1 + k^2) mu^2)
    assert np.abs(q.uiqi - 4 * k * k / (1 + k * k) ** 2).max() <= 1e-11
    assert np.abs(q.ergas - 100.0 / 2.0 * (k - 1) * np.sqrt((e2 / (mu * mu)).mean(1))).max() <= 1e-11 * q.ergas.max()
    assert np.abs(q.rmse - (k - 1) * np.sqrt(e2)).max() <= 1e-13 and _quality(pred, ref).ergas is None


def test_closed_forms_offset_orthogonal_zero_and_empty():
    ref = synth_input("mh_or", (2, 3, 16, 12), 1, uniform=True)
    d = 0.25                                                                    # (exact in fp32 against [0, 1) data up to rounding of the sum)
    pred = ref.double() + d
    band, _ = MR.band_stats(pred, ref)
    sample, _ = MR.sample_stats(pred, ref)
    q = M._derive(band.numpy(), sample.numpy(), None, 1.0, None)
    assert np.abs(q.bias - d).max() <= 1e-15 and np.abs(q.rmse - d).max() <= 1e-15 and np.abs(q.max_abs - d).max() <= 1e-15
    assert np.abs(q.cc - 1.0).max() <= 1e-12 and np.abs(q.psnr - 10 * np.log10(1 / d ** 2)).max() <= 1e-12
    # orthogonal spectra: 90 degrees; a zero spectrum on either side: no angle
    p = torch.zeros(1, 2, 2, 2)
    t = torch.zeros(1, 2, 2, 2)
    p[0, 0], t[0, 1] = 3.0, 0.5
    p[0, :, 0, 0] = 0.0                                                         # pixel (0, 0): pred is a zero spectrum
    t[0, :, 1, 1] = 0.0                                                         # pixel (1, 1): the truth is
    q = _quality(p, t)
    assert q.sam_deg[0] == 90.0 and q.sam_undefined[0] == 2 and q.n[0] == 4
    # an empty region: NaN, not an error; a batch-1 where against B = 2
    q = _quality(torch.rand(2, 3, 4, 4), torch.rand(1, 3, 4, 4), where=torch.zeros(1, 1, 4, 4))
    assert (q.n == 0).all() and (q.sam_undefined == 0).all()
    for f in ("rmse", "bias", "max_abs", "psnr", "psnr_all", "cc", "uiqi", "sam_deg"):
        assert np.isnan(getattr(q, f)).all(), f
    ref_q = MR.quality_ref(torch.rand(2, 3, 4, 4), torch.rand(1, 3, 4, 4), where=torch.zeros(1, 1, 4, 4), kernel_size=3)
    assert np.isnan(ref_q["rmse"]).all() and (ref_q["n"] == 0).all()


def test_host_formulas_against_the_independent_reference():
    """_derive (raw moments) against quality_ref (centred, from the definitions) with where and the affine.  Raw-moment variances lose
    about E[x^2] / var = 4 digits-of-2 against the centred ones and both carry n * 2^-53 = 2e-13 of summation error: 1e-9 relative is
    three orders above that and eight below the quantities."""
    pred = synth_input("mh_hp", (2, 4, 20, 24), 1)
    ref = pred + 0.1 * synth_input("mh_hr", (1, 4, 20, 24), 2)
    where = (synth_input("mh_hw", (2, 1, 20, 24), 3, uniform=True) > 0.3).float()
    aff = (0.5, 0.5)
    q = _quality(pred, ref[:1], where, aff, 1.0, 2.0)
    want = MR.quality_ref(pred, ref[:1], where, 1.0, aff, 2.0, kernel_size=3)
    for f in ("n", "rmse", "bias", "max_abs", "psnr", "psnr_all", "cc", "uiqi", "sam_deg", "sam_undefined", "ergas"):
        got, w = getattr(q, f), want[f]
        assert got.shape == w.shape and np.abs(got - w).max() <= 1e-9 * np.abs(w).max(), f


def test_hole_of_follows_the_skip_known_rule():
    m = torch.tensor([[1.0, 0.0, 0.5], [float("nan"), 1.0 - 2 ** -24, 1.0]]).reshape(1, 1, 2, 3)
    h = M.hole_of(m)
    assert h.dtype == torch.float32 and tuple(h.shape) == (1, 1, 2, 3) and h.flatten().tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 0.0]
    assert tuple(M.hole_of(torch.ones(3, 4, 5)).shape) == (3, 1, 4, 5) and tuple(M.hole_of(torch.ones(4, 5)).shape) == (1, 1, 4, 5)
    for bad in (torch.ones(1, 2, 4, 4), torch.ones(4), "mask"):
        with pytest.raises(EodError):
            M.hole_of(bad)


def test_every_refusal():
    x, y = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)
    calls = (lambda *a, **k: M.quality(*a, **k), lambda *a, **k: M.ssim(*a, **k), lambda *a, **k: M.psnr(*a, **k),
             lambda *a, **k: M.band_stats(*a, **k))
    for f in calls:
        with pytest.raises(EodError, match="no CPU"):                       # CPU tensors: the kernels are mandatory
            f(x, y)
        for bad in ((x, torch.zeros(2, 3, 16, 15)), (x, torch.zeros(3, 3, 16, 16)), (x, torch.zeros(2, 4, 16, 16)), (x[0], y[0]), (x, "y"),
                    (torch.zeros(1, 33, 12, 12), torch.zeros(1, 33, 12, 12)), (torch.zeros(0, 3, 16, 16), torch.zeros(0, 3, 16, 16))):
            with pytest.raises(EodError) as e:
                f(*bad)
            assert "no CPU" not in str(e.value)                               # (refused for the shape, before the device is looked at)
        for w in (torch.zeros(2, 3, 16, 16), torch.zeros(3, 1, 16, 16), torch.zeros(2, 1, 16, 15), torch.zeros(16, 16), 1.0):
            with pytest.raises(EodError) as e:
                f(x, y, where=w)
            assert "no CPU" not in str(e.value)
        for aff in ((1.0,), 2.0, (1.0, float("nan")), (float("inf"), 0.0), ("a", 0.0), (True, 0.0)):
            with pytest.raises(EodError) as e:
                f(x, y, affine=aff)
            assert "no CPU" not in str(e.value)
    for f in calls[:2]:
        for ks in (0, 2, 10, 27, -3, 3.0, True, None):                          # even, oversized, not an integer
            with pytest.raises(EodError, match="kernel_size"):
                f(x, y, kernel_size=ks)
        for kw in (dict(sigma=0.0), dict(sigma=float("nan")), dict(k1=float("inf")), dict(k2="a"), dict(data_range=0.0), dict(data_range=-1.0)):
            with pytest.raises(EodError) as e:
                f(x, y, **kw)
            assert "no CPU" not in str(e.value)
        with pytest.raises(EodError, match="smaller than"):                     # an image smaller than the window
            f(torch.zeros(1, 3, 10, 16), torch.zeros(1, 3, 10, 16))
        with pytest.raises(EodError, match="smaller than"):
            f(torch.zeros(1, 3, 16, 4), torch.zeros(1, 3, 16, 4), kernel_size=5)
    with pytest.raises(EodError, match="no CPU"):                           # (quality without SSIM needs no window)
        M.quality(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2), ssim=False)
    for ratio in (0, 0.0, -2, float("nan"), "2", True):
        with pytest.raises(EodError, match="ratio"):
            M.quality(x, y, ratio=ratio)
    with pytest.raises(EodError, match="data_range"):
        M.psnr(x, y, 0.0)


def test_signatures_and_no_oracle_import():
    def names(f):
        return [(p.name, p.kind, p.default) for p in inspect.signature(f).parameters.values()]
    P, K, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    assert names(M.band_stats) == [("pred", P, E), ("ref", P, E), ("where", P, None), ("affine", P, (1.0, 0.0))]
    assert names(M.quality) == [("pred", P, E), ("ref", P, E), ("where", K, None), ("data_range", K, 1.0), ("affine", K, (1.0, 0.0)), ("ratio", K, None),
                                ("ssim", K, True), ("kernel_size", K, 11), ("sigma", K, 1.5), ("k1", K, 0.01), ("k2", K, 0.03)]
    assert names(M.ssim) == [("pred", P, E), ("ref", P, E), ("data_range", P, 1.0), ("kernel_size", P, 11), ("sigma", P, 1.5), ("k1", P, 0.01),
                             ("k2", P, 0.03), ("where", K, None), ("affine", K, (1.0, 0.0)), ("return_map", K, False)]
    assert names(M.psnr) == [("pred", P, E), ("ref", P, E), ("data_range", P, 1.0), ("where", K, None), ("affine", K, (1.0, 0.0))]
    assert names(M.hole_of) == [("mask", P, E)]
    from eo_diffusion_amd import harness as H
    assert [n for n, _, _ in names(M.ssim)][:7] == [n if n not in ("preds", "target") else {"preds": "pred", "target": "ref"}[n] for n, _, _ in names(H.ssim)]
    assert np.array_equal(M.gauss_window(11, 1.5), H._gauss_kernel(11, 1.5)) and np.array_equal(M.gauss_window(5, 0.7), MR.gauss(5, 0.7))
    with open(M.__file__) as f:
        tree = ast.parse(f.read())
    mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    mods += [(n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert mods and not any(m.split(".")[0] == "oracle" for m in mods)


def test_tile_body_runs_clean_under_sanitizers_and_matches_a_plain_loop(tmp_path):
    """tests/ssim_host_check.cc: the tile phases of csrc/ssim_body.h compiled for the host with -fsanitize=address,undefined and run as a
    program of its own (nothing is loaded into this interpreter): valid-region extents 1, 31, 32, 33 and 65 on both axes independently at
    r = 5, r = 0, 1 and 12 at the same edges, exactly sized buffers, the map bit for bit against a plain double loop in the same file"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    # no skip: this is the out-of-bounds check of the tile body, and a machine that built the library has a C++ compiler
    assert cxx is not None, "no host C++ compiler (ROCm's clang++, clang++ or g++) to build tests/ssim_host_check.cc with"
    exe = str(tmp_path / "ssim_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "ssim_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok 34"), run.stdout[-2000:] + run.stderr[-2000:]
