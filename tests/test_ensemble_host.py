"""CPU: the emulations of the ensemble statistics (tests/ensemble_ref.py) against independent forms -- numpy's float64 quantile, the
brute-force CRPS double loop, the flat rank histogram of a calibrated Gaussian ensemble -- the shared (k, frac) rule against the rule
DynamicThreshold.rank has always had, and every refusal of tiling.scene_quantiles / metrics.ensemble that needs no GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd import metrics as M
from eo_diffusion_amd import tiling as T
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.threshold import DynamicThreshold
from eo_diffusion_amd.engine import quantile_rank
from tests import ensemble_ref as ER

QS = (0.0, 1.0, 0.5, 0.05, 0.95, 1.0 / 3.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rank_rule(q, n):
    """the rule as DynamicThreshold.rank stated it before the helper existed, restated here"""
    pos = q * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    frac = float(np.float32(pos - k)) if pos > k else 0.0
    if frac >= 1.0:
        k, frac = k + 1, 0.0
    return k, frac


def test_keys_are_a_total_order_and_invert():
    vals = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf, np.nan], dtype=np.float32)
    k = ER.keys(vals)
    assert (np.diff(k.astype(np.int64)) > 0).all() and k[-1] == ER.TOP
    assert ER.keys(np.array([-np.nan], dtype=np.float32))[0] == ER.TOP                      # a NaN of either sign
    back = ER.unkeys(k)
    assert np.array_equal(back.view(np.uint32)[:-1], vals.view(np.uint32)[:-1]) and np.isnan(back[-1])
    x = np.random.default_rng(0).standard_normal((7, 100)).astype(np.float32)
    assert np.array_equal(ER.unkeys(ER.sorted_keys(x)), np.sort(x, axis=0))


@pytest.mark.parametrize("B", (1, 2, 3, 5, 8, 17, 64))
def test_fp32_quantile_emulation_against_numpy_float64(B):
    x = (np.random.default_rng(B).standard_normal((B, 513)) * 3).astype(np.float32)
    bound = 4 * 2.0 ** -24 * float(np.abs(x).max())
    for q in QS:
        got = ER.scene_quantiles(x, [quantile_rank(q, B)])[0].astype(np.float64)
        want = np.quantile(x.astype(np.float64), q, axis=0, method="linear")
        assert np.abs(got - want).max() <= bound, (B, q, np.abs(got - want).max(), bound)


@pytest.mark.parametrize("B", (1, 2, 9, 33))
def test_sorted_crps_against_the_double_loop(B):
    rng = np.random.default_rng(100 + B)
    x = rng.standard_normal((B, 64)).astype(np.float32)
    y = rng.standard_normal(64).astype(np.float32)
    x[:, 3] = x[0, 3]                                                                       # equal members
    y[5] = x[B // 2, 5]                                                                     # a tie with the truth
    p = ER.pixel_terms(x, y)
    for i in range(64):
        want = ER.crps_brute(x[:, i], y[i])
        scale = max(abs(want), float(np.abs(x[:, i] - y[i]).mean()))
        assert abs(p["crps"][i] - want) <= 1e-12 * scale, (i, p["crps"][i], want)
    assert (p["crps"] <= p["terms"][:, 0]).all()                                            # CRPS <= the members' mean absolute error
    if B == 1:
        assert np.array_equal(p["crps"], np.abs(x[0].astype(np.float64) - y.astype(np.float64))) and (p["terms"][:, 3] == 0).all()


def test_rank_histogram_of_a_calibrated_gaussian_ensemble_is_flat():
    """members and truth iid from one Gaussian: the truth's rank is uniform on 0 .. B; every bin within 5 standard deviations of n / (B + 1)
    (an off-by-one of the rank empties an end bin)"""
    B, n = 9, 20000
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((B, n)).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    p = ER.pixel_terms(x, y)
    hist = np.bincount(p["rank"], minlength=B + 1)
    pr = 1.0 / (B + 1)
    assert hist.sum() == n and len(hist) == B + 1
    assert (np.abs(hist - n * pr) <= 5 * math.sqrt(n * pr * (1 - pr))).all(), hist
    assert np.array_equal(ER.pixel_terms(x, np.full(n, -100, np.float32))["rank"], np.zeros(n, np.int64))
    assert np.array_equal(ER.pixel_terms(x, np.full(n, 100, np.float32))["rank"], np.full(n, B))


def test_the_shared_rank_helper_is_the_rule_of_dynamic_threshold():
    qs = [0.0, 1.0, 0.5, 0.05, 0.95, 1.0 / 3.0, 0.995, 0.999999, 1e-9, 1 - 2.0 ** -30, 0.25, 0.75]
    ns = [1, 2, 3, 5, 8, 9, 16, 33, 64, 65, 1000, 3 * 64 * 64, 2 ** 24 + 1, 2 ** 31 - 1]
    for q in qs:
        for n in ns:
            k, frac = quantile_rank(q, n)
            assert (k, frac) == rank_rule(q, n) == DynamicThreshold(q).rank(n), (q, n)
            assert 0 <= k < n and 0.0 <= frac < 1.0 and (frac == 0.0 or k + 1 < n) and frac == float(np.float32(frac))
    assert quantile_rank(1 - 2.0 ** -30, 2) == (1, 0.0)                                     # pos - k rounds to 1 in fp32: the carry
    assert T.quantile_ranks("t", (0.05, 0.5, 0.95), 9) == [quantile_rank(q, 9) for q in (0.05, 0.5, 0.95)]
    assert T.quantile_ranks("t", 0.5, 4) == [(1, 0.5)]


def test_scene_quantiles_refusals_need_no_gpu():
    ok = torch.zeros(4, 2, 3, 5)
    for stack, kw in ((torch.zeros(4, 3, 5), {}), (torch.zeros(0, 2, 3, 5), {}), (torch.zeros(4, 2, 0, 5), {}), ("stack", {}),
                      (torch.zeros(65, 1, 2, 2), {}),
                      (ok, dict(q=())), (ok, dict(q=(0.5,) * 9)), (ok, dict(q=(-0.1,))), (ok, dict(q=(1.5,))), (ok, dict(q=(math.nan,))),
                      (ok, dict(q=(True,))), (ok, dict(q=True)), (ok, dict(q=("0.5",))), (ok, dict(q=None)),
                      (ok, dict(out=torch.zeros(2, 2, 3, 5))), (ok, dict(out=torch.zeros(3, 2, 3, 5, dtype=torch.float64))),
                      (ok, dict(out=torch.zeros(3, 2, 5, 3).transpose(2, 3))), (ok, dict(out=torch.zeros(3, 2, 3, 5, device="meta"))),
                      (ok, dict(out="out"))):
        with pytest.raises(EodError):
            T.scene_quantiles(stack, **kw)
    with pytest.raises(EodError, match="MI355X"):                                           # good arguments: only the GPU is missing
        T.scene_quantiles(ok, (0.5,), out=torch.zeros(1, 2, 3, 5))


def test_ensemble_refusals_need_no_gpu():
    d, r = torch.zeros(4, 2, 3, 5), torch.zeros(1, 2, 3, 5)
    for a, kw in (((torch.zeros(4, 3, 5), r), {}), ((torch.zeros(0, 2, 3, 5), r), {}), ((torch.zeros(65, 2, 3, 5), r), {}),
                  ((torch.zeros(4, 33, 3, 5), torch.zeros(1, 33, 3, 5)), {}),
                  ((d, torch.zeros(4, 2, 3, 5)), {}), ((d, torch.zeros(1, 3, 3, 5)), {}), ((d, torch.zeros(2, 3, 5)), {}),
                  ((d, r), dict(where=torch.zeros(4, 1, 3, 5))), ((d, r), dict(where=torch.zeros(1, 2, 3, 5))), ((d, r), dict(where=torch.zeros(3, 5))),
                  ((d, r), dict(levels=(0.1, 0.2, 0.3, 0.4, 0.5))), ((d, r), dict(levels=(1.5,))), ((d, r), dict(levels=(math.nan,))),
                  ((d, r), dict(levels=(True,))), ((d, r), dict(levels=0.5))):
        with pytest.raises(EodError):
            M.ensemble(*a, **kw)
    with pytest.raises(EodError, match="MI355X"):
        M.ensemble(d, r, where=torch.ones(1, 1, 3, 5), levels=())


def test_derive_and_describe_on_host_tables():
    """the host arithmetic of ensemble() from the emulation's tables: an empty region gives NaN, not an error"""
    B, C, H, W = 5, 2, 6, 7
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    y = rng.standard_normal((C, H, W)).astype(np.float32)
    lv, lo, hi = M._levels("t", (0.5, 0.9), B)
    sums, _, counts, _ = ER.ensemble_stats(x, y, None, list(zip(lo, hi)))
    e = M._derive_ensemble(sums, counts, B, lv)
    assert e.rank_hist.shape == (C, B + 1) and e.coverage.shape == (C, 2) and (e.n == H * W).all() and (e.rank_hist.sum(1) == H * W).all()
    assert (e.crps <= e.mae_members).all() and (e.crps_fair <= e.crps).all() and (e.coverage[:, 0] <= e.coverage[:, 1]).all()
    mean = x.astype(np.float64).mean(0)
    assert np.allclose(e.rmse_mean, np.sqrt(((mean - y) ** 2).mean((1, 2))), rtol=1e-12)
    assert np.allclose(e.spread, np.sqrt(x.astype(np.float64).var(0, ddof=1).mean((1, 2))), rtol=1e-12)
    assert "5 members" in M.describe_ensemble(e, "t")
    sums, _, counts, cmap = ER.ensemble_stats(x, y, np.zeros((H, W), np.float32), list(zip(lo, hi)))
    z = M._derive_ensemble(sums, counts, B, lv)
    assert (z.n == 0).all() and np.isnan(z.crps).all() and np.isnan(z.coverage).all() and np.isnan(z.spread_skill).all() and np.isnan(cmap).all()
    assert np.isnan(M._derive_ensemble(*ER.ensemble_stats(x[:1], y)[0:3:2], 1, ()).crps_fair).all()


def test_the_sorter_header_on_the_host_under_sanitizers(tmp_path):
    """tests/ensemble_host_check.cc: csrc/ensemble_body.h compiled for the host with -fsanitize=address,undefined and run as a program of its
    own (nothing is loaded into this interpreter): the key order, the network of every padded size against std::sort, the pick at every
    index, the quantile against its three fp32 operations"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler (ROCm's clang++, clang++ or g++) to build tests/ensemble_host_check.cc with"
    exe = str(tmp_path / "ensemble_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "ensemble_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
