"""CPU: prediction targets other than the noise (DESIGN.md sections 8.2 and 9.16) -- tests/param_ref.py against float64, the identities
between the eps, x0 and v views of one triple and between their min-SNR weights, the float64 loops on the Gaussian toy under each denoiser,
the host-side contract of EODiffusion(parameterization=...), and the kernel bodies (csrc/param_body.h) compiled for the host and run under
the address and undefined-behaviour sanitizers as a stand-alone program whose outputs are compared with the emulation."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from oracle import schedule as SCH
from tests import ancestral_ref as AR
from tests import dpm_ref as DR
from tests import param_ref as PR
from tests.helpers import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (2.43e-9, 2.4e-6, 1e-4, 0.37, 0.99995875)
BUFFERS = ["betas", "alphas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"]


def _ulp(ref64):
    """the spacing of fp32 at |ref64| (never below that of the smallest normal)"""
    return np.spacing(np.maximum(np.abs(ref64), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def _diffusion(parameterization="eps", T=20, **kw):
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")
    return EODiffusion(Never(), timesteps=T, image_size=16, in_channels=3, parameterization=parameterization, **kw)


# ------------------------------------------------------------------------------------------------ the emulation against float64
def test_emulation_is_within_two_ulp_of_float64():
    """every output against the float64 evaluation of the SAME rounded inputs (x, o, sqrtf(a), sqrt_1m_a as fp32 values): three roundings
    for the v prediction, three for its noise estimate, three for x0's.  The product sa * x is exact to half an ulp of itself, the sum to
    half an ulp of the result, so the bound of 2 ulp of the result holds wherever the two products do not cancel: inputs with sa * x and
    s1 * o of one sign for the sum, of opposite sign for the difference.  The via-eps route is printed next to it."""
    rng = np.random.default_rng(3)
    n = 65536
    worst = {}
    for a in LEVELS + (0.0,):
        sa32, s1_32 = np.sqrt(np.float32(a)), np.sqrt(np.float32(1.0) - np.float32(a))
        sa, s1 = float(sa32), float(s1_32)
        mag_x, mag_o = np.abs(rng.standard_normal(n)).astype(np.float32) + np.float32(0.01), np.abs(rng.standard_normal(n)).astype(np.float32) + np.float32(0.01)
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
        for kind, name in ((PR.V, "v"), (PR.X0, "x0")):
            # p of v subtracts, e of v adds, e of x0 subtracts: one sign pattern per output keeps its two terms from cancelling
            for out_name, x, o in (("p", sign * mag_x, -sign * mag_o), ("e", sign * mag_x, (sign if kind == PR.V else -sign) * mag_o)):
                if kind == PR.X0 and a == 0.0:
                    continue                                         # (x0 at a = 0 is the copy; its e divides by 1: covered by the other levels)
                p, e = PR.pred(torch.from_numpy(x), torch.from_numpy(o), kind, a, s1_32)
                got = (p if out_name == "p" else e).numpy().astype(np.float64)
                want = PR.pred64(x, o, kind, sa, s1) if out_name == "p" else PR.eps64(x, o, kind, sa, s1)
                err = float((np.abs(got - want) / _ulp(want)).max())
                worst[(name, out_name)] = max(worst.get((name, out_name), 0.0), err)
                assert err <= 2.0, (name, out_name, a, err)
        # signs at random (the terms may cancel): each product is off by half an ulp of itself, the sum by half an ulp of the result, so
        # the error is at most 1.5 ulp of the largest of the three
        x, o = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        p, e = PR.pred(torch.from_numpy(x), torch.from_numpy(o), PR.V, a, s1_32)
        for got, want, big in ((p, PR.pred64(x, o, PR.V, sa, s1), np.maximum(np.abs(sa * x.astype(np.float64)), np.abs(s1 * o.astype(np.float64)))),
                               (e, PR.eps64(x, o, PR.V, sa, s1), np.maximum(np.abs(sa * o.astype(np.float64)), np.abs(s1 * x.astype(np.float64))))):
            assert (np.abs(got.numpy().astype(np.float64) - want) <= 1.5 * _ulp(np.maximum(big, np.abs(want)))).all(), a
    print("largest |fp32 emulation - float64| in ulp of the result: " + ", ".join(f"{k[0]}.{k[1]} {v:.2f}" for k, v in sorted(worst.items())))


def test_direct_form_against_the_via_eps_route():
    """the table of the design: max |error of the prediction| of a v output on 65 536 standard-normal elements, float64 on the same rounded
    inputs as the reference.  The direct form stays at rounding level at every noise level; the route through a noise estimate does not."""
    rng = np.random.default_rng(0)
    x, v = rng.standard_normal(65536).astype(np.float32), rng.standard_normal(65536).astype(np.float32)
    for a in LEVELS:
        sa32, s1_32 = np.sqrt(np.float32(a)), np.sqrt(np.float32(1.0) - np.float32(a))
        want = PR.pred64(x, v, PR.V, float(sa32), float(s1_32))
        direct = float(np.abs(PR.pred(torch.from_numpy(x), torch.from_numpy(v), PR.V, a, s1_32)[0].numpy() - want).max())
        via = float(np.abs(PR.via_eps(x, v, a, s1_32).astype(np.float64) - want).max())
        print(f"a = {a:.3g}: max |error of the prediction|: via eps {via:.2e}, direct {direct:.2e}")
        assert direct <= 4 * 2.0 ** -24 * float(np.abs(want).max() + 1.0)      # (three roundings of quantities of at most |want| + 1 in size)
        if a <= 1e-4:
            assert via > 10 * direct                                 # (the via-eps error grows like 2^-24 / sqrt(a): 100 x rounding level at a = 1e-4)


# ------------------------------------------------------------------------------------------------ identities in float64
def test_the_three_views_of_one_triple_agree_in_float64():
    rng = np.random.default_rng(1)
    x0, eps = rng.uniform(-1, 1, 4096), rng.standard_normal(4096)
    for a in (1e-4, 0.01, 0.37, 0.9, 0.999):
        x, outs = PR.views64(x0, eps, a)
        sa, s1 = np.sqrt(a), np.sqrt(1.0 - a)
        for kind, o in outs.items():
            assert np.abs(PR.pred64(x, o, kind, sa, s1) - x0).max() <= 1e-12 * max(1.0, 1.0 / sa), (kind, a)
            assert np.abs(PR.eps64(x, o, kind, sa, s1) - eps).max() <= 1e-12 * max(1.0, 1.0 / s1), (kind, a)
        p = {k: PR.pred64(x, o, k, sa, s1) for k, o in outs.items()}
        e = {k: PR.eps64(x, o, k, sa, s1) for k, o in outs.items()}
        assert np.abs(p[PR.V] - p[PR.X0]).max() <= 1e-12 and np.abs(e[PR.V] - e[0]).max() <= 1e-12


def test_min_snr_weights_of_the_three_targets():
    """w_x0 = w_eps * SNR and w_v = w_eps * a to 1e-12 on the T = 1000 buffer with gamma = 5 (float64 of the table's own arithmetic), each
    table equal to min(SNR, gamma) over its loss's SNR scale, and the edges a = 0 and a = 1 finite"""
    from eo_diffusion_amd.diffusion.model import loss_weight_table
    m = _diffusion(T=1000)
    acp = m.alphas_cumprod
    a = acp.double().numpy()
    snr = a / (1.0 - a)
    w = {k: loss_weight_table(acp.double(), "min_snr", 5.0, parameterization=k).double().numpy() for k in ("eps", "x0", "v")}
    # (the product rounds the table to fp32 once: compare at fp32 resolution, and in float64 through the unrounded arithmetic below)
    def exact(kind):
        if kind == "eps":
            return np.minimum(1.0, 5.0 * (1.0 - a) / a)
        return np.minimum(a / (1.0 - a), 5.0) if kind == "x0" else np.minimum(a, 5.0 * (1.0 - a))
    ref = PR.min_snr64(a, 5.0)
    for kind in ("eps", "x0", "v"):
        assert np.abs(exact(kind) - ref[PR.KINDS[kind]]).max() <= 1e-12 * max(1.0, float(ref[PR.KINDS[kind]].max())), kind
        assert np.array_equal(w[kind], exact(kind).astype(np.float32).astype(np.float64)), kind
    assert np.abs(exact("x0") - exact("eps") * snr).max() <= 1e-12 * 5.0
    assert np.abs(exact("v") - exact("eps") * a).max() <= 1e-12
    for kind in ("eps", "x0", "v"):
        assert torch.equal(m.loss_weights("min_snr", 5.0, parameterization=kind), loss_weight_table(acp, "min_snr", 5.0, parameterization=kind))
        edge = loss_weight_table(torch.tensor([0.0, 1.0, 0.5]), "min_snr", 5.0, parameterization=kind)
        assert bool(torch.isfinite(edge).all())
        assert edge.tolist() == {"eps": [1.0, 0.0, 1.0], "x0": [0.0, 5.0, 1.0], "v": [0.0, 0.0, 0.5]}[kind]
        for other in ("p2", "uniform"):                              # (independent of the target)
            assert torch.equal(loss_weight_table(acp, other, 1.0, parameterization=kind), loss_weight_table(acp, other, 1.0))
    assert torch.equal(_diffusion("v", T=1000).loss_weights("min_snr", 5.0), m.loss_weights("min_snr", 5.0, parameterization="v"))
    assert torch.equal(m.loss_weights("min_snr", 5.0), loss_weight_table(acp, "min_snr", 5.0))      # the default: today's table


# ------------------------------------------------------------------------------------------------ the toy
def test_float64_loops_on_the_toy_do_not_depend_on_the_target():
    acp = SCH.eo_cosine_tables(1000)["alphas_cumprod"].numpy().astype(np.float64)
    worst = {}
    for S in (25, 100):
        base, levels = DR.dpm_f64(acp, S, 2, "logsnr")
        for kind in (PR.X0, PR.V):
            got, lv = PR.dpm_f64(acp, S, 2, "logsnr", kind)
            assert np.array_equal(lv, levels)
            worst[("dpm", S, kind)] = float(np.abs(got - base).max())
    levels = np.arange(1, 1000, 4)
    base = DR.ddim_f64(acp, levels)
    for kind in (PR.X0, PR.V):
        worst[("ddim", 250, kind)] = float(np.abs(PR.ddim_f64(acp, levels, kind) - base).max())
    T = 50
    tb64 = AR.tables64(SCH.eo_cosine_tables(T))
    noises = np.random.default_rng(9).standard_normal((T, DR.TOY_N))
    base, _ = AR.ddpm_f64(tb64, noises)
    for kind in (PR.X0, PR.V):
        worst[("ddpm", T, kind)] = float(np.abs(PR.ddpm_f64(tb64, noises, kind) - base).max())
    print("max |x0 / v loop - eps loop| in float64: " + ", ".join(f"{k}: {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-10, worst
    # ... and the loops under kind 0 ARE the eps loops (the same operations)
    assert np.array_equal(PR.dpm_f64(acp, 25, 2, "logsnr", 0)[0], DR.dpm_f64(acp, 25, 2, "logsnr")[0])


# ------------------------------------------------------------------------------------------------ the host-side contract
def test_default_is_eps_and_the_state_dict_is_unchanged():
    from eo_diffusion_amd.diffusion.model import EODiffusion
    import inspect
    assert _diffusion().parameterization == "eps"
    assert list(inspect.signature(EODiffusion.__init__).parameters)[-1] == "parameterization"   # the last keyword: positional calls unchanged
    for p in ("eps", "x0", "v"):
        m = _diffusion(p)
        assert m.parameterization == p and isinstance(m.parameterization, str)
        assert list(m.state_dict().keys()) == BUFFERS
        assert [k for k, _ in m.named_buffers()] == BUFFERS
        other = _diffusion("eps")
        other.load_state_dict(m.state_dict())                        # a checkpoint carries the schedule, not the target
        assert other.parameterization == "eps"


def test_deepcopy_and_averaged_model_keep_the_attribute():
    from eo_diffusion_amd.optim import ExponentialMovingAverage
    for p in ("x0", "v"):
        m = _diffusion(p)
        assert copy.deepcopy(m).parameterization == p
        assert torch.optim.swa_utils.AveragedModel(m, use_buffers=True).module.parameterization == p
        assert ExponentialMovingAverage(m, 0.99).module.parameterization == p


def test_refusals_before_any_launch():
    from eo_diffusion_amd.diffusion import consistency as CO
    from eo_diffusion_amd.diffusion import threshold as TH
    from eo_diffusion_amd.diffusion.model import EODiffusion, loss_weight_table
    for bad in ("epsilon", "V", "", None, 2, b"v"):
        with pytest.raises(EodError):
            EODiffusion(torch.nn.Identity(), 16, 3, parameterization=bad)
        with pytest.raises(EodError):
            loss_weight_table(torch.tensor([0.5]), "min_snr", 5.0, parameterization=bad if bad is not None else "none")
        with pytest.raises(EodError):
            CO.BoundChain([], parameterization=bad)
        with pytest.raises(EodError):
            TH.bind(None, None, "call", (1, 3, 16, 16), 4, None, bad)
    x = torch.zeros(2, 3, 16, 16)
    for p in ("eps", "x0", "v"):
        m = _diffusion(p)
        for bad in (1, 0, "yes", None, torch.tensor(True)):          # a return_target that is no bool: refused on a CPU tensor, before anything else
            with pytest.raises(EodError):
                m(x, x, t=torch.zeros(2, dtype=torch.int64), return_target=bad)
    # the binding of a call: None for an eps model without observation, ALWAYS a chain for the others (device None: the refusals alone)
    assert TH.bind(None, None, "call", (1, 3, 16, 16), 4, None, "v") is None
    assert TH.bind(None, None, "call", (1, 3, 16, 16), 4, "cpu", "eps") is None
    chain = TH.bind(None, None, "call", (1, 3, 16, 16), 4, "cpu", "v")
    assert isinstance(chain, CO.BoundChain) and chain.links == [] and chain.kind == 2 and chain.threshold is None
    one = TH.bind(None, CO.Observation(torch.zeros(1, 3, 16, 16), (1, 2, 4)), "call", (1, 3, 16, 16), 4, "cpu", "x0")
    assert isinstance(one, CO.BoundChain) and len(one.links) == 1 and one.kind == 1
    assert isinstance(TH.bind(None, CO.Observation(torch.zeros(1, 3, 16, 16), (1, 2, 4)), "call", (1, 3, 16, 16), 4, "cpu"), CO.BoundObservation)


def test_targets_that_need_no_launch():
    x, z = torch.randn(2, 3, 16, 16), torch.randn(2, 3, 16, 16)
    t = torch.tensor([3, 7])
    assert _diffusion("eps").target(x, z, t) is z and _diffusion("x0").target(x, z, t) is x


def test_library_exports_every_symbol_of_the_param_header():
    """include/eodiff_param.h (which include/eodiff.h includes) against _lib.PARAM_SYMBOLS and the compiled library, as
    tests/test_host_contract.py holds include/eodiff.h against _lib.SYMBOLS"""
    import re
    from eo_diffusion_amd import _lib
    inc = os.path.join(ROOT, "include")
    declared = set(re.findall(r"\b(eod_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "eodiff_param.h")).read(), flags=re.S)))
    assert declared == set(_lib.PARAM_SYMBOLS) == {"eod_param_pred", "eod_ddpm_param_pred", "eod_q_sample_v"}
    assert '#include "eodiff_param.h"' in open(os.path.join(inc, "eodiff.h")).read()
    assert not set(_lib.PARAM_SYMBOLS) & set(_lib.SYMBOLS)
    L = _lib.lib()
    for name, (res, args) in _lib.PARAM_SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert L.eod_version() == _lib.ABI_VERSION == 120


def test_the_dropin_paths_still_re_export():
    from eo_diffusion_amd.diffusion import consistency as CO
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    from eo_diffusion_amd.dropin.diffusion.model import EODiffusion as DropinEODiffusion
    assert DropinEODiffusion is EODiffusion and D.BoundChain is CO.BoundChain and D.ddpm_step is CO.ddpm_step
    assert D.ddpm_pred_x0 is CO.ddpm_pred_x0 and D.PARAMETERIZATIONS == ("eps", "x0", "v")


# ------------------------------------------------------------------------------------------------ the kernels' bodies on the host
def _records(stdout, words):
    """the cases of tests/param_host_check.cc's file: dicts of numpy / torch views"""
    for line in stdout.splitlines():
        if not line.startswith("case "):
            continue
        f = line.split()
        form, kind, clip, two, N, chw, T = (int(v) for v in f[1:8])
        a, s1, off = float(f[8]), float(f[9]), int(f[10])
        n = N * chw
        take = lambda k: torch.from_numpy(words[off + k * n: off + (k + 1) * n].copy()).reshape(N, chw)
        rec = dict(form=form, kind=kind, clip=clip, two=two, N=N, chw=chw, T=T, a=a, s1=s1, x=take(0), o=take(1), out0=take(2), out1=take(3))
        if form != 0:
            p = off + 4 * n
            rec["t"] = torch.from_numpy(words[p: p + 2 * N].copy().view(np.int64))
            rec["tb"] = {"alphas_cumprod": torch.zeros(T), "sqrt_alphas_cumprod": torch.from_numpy(words[p + 2 * N: p + 2 * N + T].copy()),
                         "sqrt_one_minus_alphas_cumprod": torch.from_numpy(words[p + 2 * N + T: p + 2 * N + 2 * T].copy())}
        yield rec


def test_kernel_bodies_run_clean_under_sanitizers_and_match_the_emulation(tmp_path):
    """tests/param_host_check.cc: csrc/param_body.h compiled for the host with -fsanitize=address,undefined and run as a program of its own
    (nothing is loaded into this interpreter): both access forms, chw in {77, 768}, both kinds, every level, out-of-range timesteps, exactly
    sized buffers; then every case it wrote, bit for bit against tests/param_ref.py"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, data = str(tmp_path / "param_host_check"), str(tmp_path / "cases.bin")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "param_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.splitlines()[-1].startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
    words = np.fromfile(data, dtype=np.float32)
    seen = 0
    for r in _records(run.stdout, words):
        if r["form"] == 0:
            p, e = PR.pred(r["x"], r["o"], r["kind"], r["a"], r["s1"], bool(r["clip"]), with_e=bool(r["two"]))
            assert bits_equal(p, r["out0"]) and (not r["two"] or bits_equal(e, r["out1"])), r
        elif r["form"] == 1:
            assert bits_equal(PR.ddpm_pred(r["tb"], r["x"], r["o"], r["t"], r["kind"], bool(r["clip"])), r["out0"]), r
        else:
            x_t, v = PR.q_sample_v(r["tb"], r["x"], r["o"], r["t"])
            assert bits_equal(x_t, r["out0"]) and bits_equal(v, r["out1"]), r
        seen += 1
    assert seen == int(run.stdout.splitlines()[-1].split()[1]) == 86
