"""GPU: prediction targets other than the noise -- eod_param_pred, eod_ddpm_param_pred, eod_q_sample_v (csrc/sampler.hip, csrc/param_body.h) and
EODiffusion(parameterization="x0" | "v") through training and the six samplers.  DESIGN.md sections 8.2 and 9.16.

The three kernels are held bit for bit to the torch fp32 emulation of tests/param_ref.py (both access forms, every level, scaled inputs, NaN
elements, refusals with the outputs untouched) and the prediction at the top of the chain to float64; whole calls with injected draws to CPU
loops of the oracle UNet, its output read as v or as x0, under the trajectory gates of tests/test_gpu_sampling.py; the toy's error to the
float64 loops; scenes to bit equalities; one training step to autograd through the oracle; the default model to the launches of before."""
import collections
import functools

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation
from eo_diffusion_amd.diffusion.threshold import DynamicThreshold
from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
from eo_diffusion_amd.tiling import TilePlan
from oracle import sampler_ref as SR
from oracle import schedule as SCH
from tests import consistency_ref as CR
from tests import dpm_ref as DR
from tests import param_ref as PR
from tests.gpu_util import DEV
from tests.helpers import bits_equal, rel_l2, unet_cfgs
from tests.synth import rect_mask, synth_input, synth_state_dict
from tests.test_gpu_sampling import TRAJ_TOL

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
A_TOP = 2.43e-9                                          # acp[999] of the T = 1000 cosine schedule
LEVELS = (A_TOP, 0.37, 0.99995875)
NEW = ("eod_param_pred", "eod_ddpm_param_pred", "eod_q_sample_v")
KIND = PR.KINDS


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _offset_by_4_bytes(t):
    """a copy of `t` that starts 4 bytes behind a 16-byte boundary of its own allocation"""
    base = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    assert base.data_ptr() % 16 == 0
    v = base[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def same(a, b):
    """bit equality with NaN equal to NaN"""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and bits_equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _s1(a):
    return float(np.sqrt(np.float32(1.0) - np.float32(a)))


def param_pred(x, o, kind, a, s1, clip, p0, e_t, numel=None):
    """eod_param_pred itself; returns rc"""
    like = next(v for v in (x, o, p0) if v is not None)
    return _lib.lib().eod_param_pred(_lib.ptr(x), _lib.ptr(o), kind, float(a), float(s1), int(clip), _lib.ptr(p0), _lib.ptr(e_t),
                                     like.numel() if numel is None else numel, _stream())


@functools.lru_cache(maxsize=None)
def _tables(T):
    tb = SCH.eo_cosine_tables(T)
    return tb, {k: v.to(DEV).contiguous() for k, v in tb.items()}


def ddpm_param_pred(T, x, o, t, kind, clip, p0, N=None, chw=None, sa=None, s1=None, T_arg=None):
    d = _tables(T)[1]
    like = next(v for v in (x, o, p0) if v is not None)
    return _lib.lib().eod_ddpm_param_pred(_lib.ptr(x), _lib.ptr(o), _lib.ptr(t), d["sqrt_alphas_cumprod"].data_ptr() if sa is None else sa,
                                          d["sqrt_one_minus_alphas_cumprod"].data_ptr() if s1 is None else s1, kind, int(clip), _lib.ptr(p0),
                                          like.shape[0] if N is None else N, (like.numel() // like.shape[0]) if chw is None else chw,
                                          T if T_arg is None else T_arg, _stream())


def q_sample_v(T, x0, z, t, x_t, v, N=None, chw=None):
    d = _tables(T)[1]
    like = next(u for u in (x0, z, x_t, v) if u is not None)
    return _lib.lib().eod_q_sample_v(_lib.ptr(x0), _lib.ptr(z), _lib.ptr(t), d["sqrt_alphas_cumprod"].data_ptr(),
                                     d["sqrt_one_minus_alphas_cumprod"].data_ptr(), _lib.ptr(x_t), _lib.ptr(v), like.shape[0] if N is None else N,
                                     (like.numel() // like.shape[0]) if chw is None else chw, T, _stream())


# ------------------------------------------------------------------------------------------------------------ 1. eod_param_pred, bit for bit
@pytest.mark.parametrize("scale", [1e-30, 1.0, 1e30])
@pytest.mark.parametrize("numel", [77, 3 * 16 * 16, 4099, 3 * 64 * 64])
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_param_pred_is_bit_exact(kind, unaligned, numel, scale):
    """every level (a = 0 for v, too), clip on and off, with the noise estimate and with e_t NULL (nothing is written then); every pointer
    aligned, or every pointer 4 bytes off; inputs scaled by 1e-30, 1, 1e30 stay finite"""
    k = KIND[kind]
    x, o = (synth_input("px", (numel,), 3) * scale).to(DEV), (synth_input("po", (numel,), 4) * scale).to(DEV)
    p0, e_t = _nan(numel), _nan(numel)
    if unaligned:
        x, o, p0, e_t = (_offset_by_4_bytes(v) for v in (x, o, p0, e_t))
    for a in LEVELS + ((0.0,) if kind == "v" else ()):
        for clip in (False, True):
            for with_e in (True, False):
                p0.fill_(float("nan")), e_t.fill_(float("nan"))
                assert param_pred(x, o, k, a, _s1(a), clip, p0, e_t if with_e else None) == 0
                want_p, want_e = PR.pred(x.cpu(), o.cpu(), k, a, _s1(a), clip, with_e)
                assert bits_equal(p0.cpu(), want_p), (a, clip, with_e)
                assert bool(torch.isfinite(p0).all())
                if with_e:
                    assert bits_equal(e_t.cpu(), want_e) and bool(torch.isfinite(e_t).all()), (a, clip)
                else:
                    assert bool(torch.isnan(e_t).all()), "e_t was written by a call that was given none"
                if clip:
                    assert float(p0.abs().max()) <= 1.0


@pytest.mark.parametrize("one", ["x", "o", "p0", "e_t"])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_one_unaligned_pointer_takes_the_scalar_form_with_the_same_bits(kind, one):
    n = 3 * 16 * 16
    t = dict(x=synth_input("px", (n,), 3).to(DEV), o=synth_input("po", (n,), 4).to(DEV), p0=_nan(n), e_t=_nan(n))
    t[one] = _offset_by_4_bytes(t[one])
    assert param_pred(t["x"], t["o"], KIND[kind], 0.37, _s1(0.37), True, t["p0"], t["e_t"]) == 0
    want_p, want_e = PR.pred(t["x"].cpu(), t["o"].cpu(), KIND[kind], 0.37, _s1(0.37), True)
    assert bits_equal(t["p0"].cpu(), want_p) and bits_equal(t["e_t"].cpu(), want_e)


@pytest.mark.parametrize("kind", ["x0", "v"])
def test_a_nan_stays_in_its_own_element(kind):
    """a NaN in x or in o: NaN in the outputs that read it, at that element and nowhere else -- through the clamp, too"""
    n = 256
    k = KIND[kind]
    for where, idx in (("x", 5), ("o", 130)):
        x, o = synth_input("px", (n,), 3), synth_input("po", (n,), 4)
        (x if where == "x" else o)[idx] = float("nan")
        p0, e_t = _nan(n), _nan(n)
        assert param_pred(x.to(DEV), o.to(DEV), k, 0.37, _s1(0.37), True, p0, e_t) == 0
        want_p, want_e = PR.pred(x, o, k, 0.37, _s1(0.37), True)
        assert same(p0, want_p) and same(e_t, want_e)
        keep = torch.arange(n) != idx
        assert bool(torch.isfinite(p0.cpu()[keep]).all()) and bool(torch.isfinite(e_t.cpu()[keep]).all())
        assert bool(torch.isnan(e_t[idx]))                            # (the noise estimate reads both)
        assert bool(torch.isnan(p0[idx])) == (kind == "v" or where == "o")   # (the x0 prediction is the output itself)


def test_refusals_return_the_error_and_leave_the_outputs_alone():
    n = 768
    x, o = synth_input("px", (n,), 3).to(DEV), synth_input("po", (n,), 4).to(DEV)
    p0, e_t = _nan(n), _nan(n)
    s1 = _s1(0.37)
    both = torch.cat([x, o])
    bad = {
        "kind 0": lambda: param_pred(x, o, 0, 0.37, s1, 0, p0, e_t),
        "kind 3": lambda: param_pred(x, o, 3, 0.37, s1, 0, p0, e_t),
        "x null": lambda: param_pred(None, o, 2, 0.37, s1, 0, p0, e_t),
        "o null": lambda: param_pred(x, None, 2, 0.37, s1, 0, p0, e_t),
        "p0 null": lambda: param_pred(x, o, 2, 0.37, s1, 0, None, e_t, n),
        "numel 0": lambda: param_pred(x, o, 2, 0.37, s1, 0, p0, e_t, 0),
        "a < 0": lambda: param_pred(x, o, 2, -1e-6, s1, 0, p0, e_t),
        "a > 1": lambda: param_pred(x, o, 2, 1.0001, s1, 0, p0, e_t),
        "a nan": lambda: param_pred(x, o, 2, float("nan"), s1, 0, p0, e_t),
        "x0 with e_t at sqrt_1m_a = 0": lambda: param_pred(x, o, 1, 1.0, 0.0, 0, p0, e_t),
        "p0 is x": lambda: param_pred(x, o, 2, 0.37, s1, 0, x, e_t),
        "e_t is o": lambda: param_pred(x, o, 2, 0.37, s1, 0, p0, o),
        "p0 is e_t": lambda: param_pred(x, o, 2, 0.37, s1, 0, p0, p0),
        "p0 overlaps x partly": lambda: param_pred(both[:n], o, 2, 0.37, s1, 0, both[n // 2:n // 2 + n], e_t),
    }
    T = 1000
    t = torch.tensor([5, 500, 999], device=DEV)
    xs, os_ = synth_input("px3", (3, 256), 3).to(DEV), synth_input("po3", (3, 256), 4).to(DEV)
    q0, q1 = _nan(3, 256), _nan(3, 256)
    d = _tables(T)[1]
    bad.update({
        "ddpm kind 0": lambda: ddpm_param_pred(T, xs, os_, t, 0, 0, q0),
        "ddpm t null": lambda: ddpm_param_pred(T, xs, os_, None, 2, 0, q0),
        "ddpm x null": lambda: ddpm_param_pred(T, None, os_, t, 2, 0, q0),
        "ddpm p0 null": lambda: ddpm_param_pred(T, xs, os_, t, 2, 0, None),
        "ddpm T 0": lambda: ddpm_param_pred(T, xs, os_, t, 2, 0, q0, T_arg=0),
        "ddpm chw 0": lambda: ddpm_param_pred(T, xs, os_, t, 2, 0, q0, chw=0),
        "ddpm p0 is o": lambda: ddpm_param_pred(T, xs, os_, t, 2, 0, os_),
        "ddpm p0 is a table": lambda: ddpm_param_pred(T, xs, os_, t, 2, 0, d["sqrt_alphas_cumprod"], N=1, chw=768),
        "q_sample_v v null": lambda: q_sample_v(T, xs, os_, t, q0, None),
        "q_sample_v x_t is v": lambda: q_sample_v(T, xs, os_, t, q0, q0),
        "q_sample_v x_t is x0": lambda: q_sample_v(T, xs, os_, t, xs, q1),
        "q_sample_v t null": lambda: q_sample_v(T, xs, os_, None, q0, q1),
    })
    kept = [v.clone() for v in (x, o, xs, os_, d["sqrt_alphas_cumprod"])]
    for what, call in bad.items():
        assert call() == -1, what
        assert _lib.lib().eod_last_error()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(v).all()) for v in (p0, e_t, q0, q1)), what
    assert all(torch.equal(a, b) for a, b in zip(kept, (x, o, xs, os_, d["sqrt_alphas_cumprod"])))
    # (x0 WITHOUT a noise estimate at a = 1 is the copy: accepted)
    assert param_pred(x, o, 1, 1.0, 0.0, 0, p0, None) == 0 and torch.equal(p0, o)


# ------------------------------------------------------------------------------------------------------------ 2. the per-sample form
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("chw", [77, 768])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_ddpm_param_pred_is_bit_exact_and_checks_its_timesteps(kind, chw, unaligned):
    """N = 3 at t = [0, T - 1, 500]; then t = [0, T, 5] and [5, -1, 3]: sample 1 all NaN, samples 0 and 2 bit-equal to the reference"""
    T, k = 1000, KIND[kind]
    tb = _tables(T)[0]
    x, o = synth_input("dx", (3, chw), 5).to(DEV), synth_input("do", (3, chw), 6).to(DEV)
    p0 = _nan(3, chw)
    if unaligned:
        x, o, p0 = (_offset_by_4_bytes(v) for v in (x, o, p0))
    for tc in ([0, T - 1, 500], [0, T, 5], [5, -1, 3]):
        t = torch.tensor(tc, dtype=torch.int64)
        for clip in (False, True):
            p0.fill_(float("nan"))
            assert ddpm_param_pred(T, x, o, t.to(DEV), k, clip, p0) == 0
            want = PR.ddpm_pred(tb, x.cpu(), o.cpu(), t, k, clip)
            assert same(p0, want), (tc, clip)
            ok = [n for n, v in enumerate(tc) if 0 <= v < T]
            assert bool(torch.isfinite(p0[ok]).all()) and all(bool(torch.isnan(p0[n]).all()) for n in range(3) if n not in ok)
            if len(ok) == 3 and not clip:      # ... and each sample is the scalar-level form at the level its tables hold (a = sa^2 is not
                for n in range(3):             # representable in general, so this is said of the v prediction's operands, not of eod_param_pred)
                    sa, s1 = float(tb["sqrt_alphas_cumprod"][tc[n]]), float(tb["sqrt_one_minus_alphas_cumprod"][tc[n]])
                    ref = PR._forms(x.cpu()[n], o.cpu()[n], k, sa, s1, False)[0]
                    assert bits_equal(p0.cpu()[n], ref)


# ------------------------------------------------------------------------------------------------------------ 3. eod_q_sample_v
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("chw", [77, 768, 3 * 64 * 64])
def test_q_sample_v_is_q_sample_and_the_v_target(chw, unaligned):
    T = 1000
    tb, d = _tables(T)
    x0, z = synth_input("qx", (3, chw), 7, uniform=True).to(DEV) * 2 - 1, synth_input("qz", (3, chw), 8).to(DEV)
    x_t, v, plain = _nan(3, chw), _nan(3, chw), _nan(3, chw)
    if unaligned:
        x0, z, x_t, v = (_offset_by_4_bytes(u) for u in (x0, z, x_t, v))
    for tc in ([0, T - 1, 500], [7, T, 5], [5, -1, 3]):
        t = torch.tensor(tc, dtype=torch.int64)
        x_t.fill_(float("nan")), v.fill_(float("nan")), plain.fill_(float("nan"))
        assert q_sample_v(T, x0, z, t.to(DEV), x_t, v) == 0
        x0c, zc = x0.contiguous(), z.contiguous()
        assert _lib.lib().eod_q_sample(x0c.data_ptr(), zc.data_ptr(), t.to(DEV).data_ptr(), d["sqrt_alphas_cumprod"].data_ptr(),
                                       d["sqrt_one_minus_alphas_cumprod"].data_ptr(), plain.data_ptr(), 3, chw, T, _stream()) == 0
        assert same(x_t, plain), tc                                   # eod_q_sample's bits, the poisoned sample included
        want_xt, want_v = PR.q_sample_v(tb, x0.cpu(), z.cpu(), t)
        assert same(x_t, want_xt) and same(v, want_v), tc
        bad = [n for n, u in enumerate(tc) if not 0 <= u < T]
        assert all(bool(torch.isnan(x_t[n]).all()) and bool(torch.isnan(v[n]).all()) for n in bad)
        assert bool(torch.isfinite(v[[n for n in range(3) if n not in bad]]).all())


def test_the_target_and_the_prediction_are_inverse_at_every_level():
    """v = eod_q_sample_v(x0, eps) fed back with its x_t gives x0 again, to the rounding of two three-operation forms on quantities of at
    most |x0| + |eps| in size (6 half-ulps of that), at t = 0, 500 and T - 1 -- the top of the chain included"""
    T, chw = 1000, 4096
    x0, z = synth_input("qx", (3, chw), 7, uniform=True).to(DEV) * 2 - 1, synth_input("qz", (3, chw), 8).to(DEV)
    t = torch.tensor([0, 500, T - 1], device=DEV)
    x_t, v, back = _nan(3, chw), _nan(3, chw), _nan(3, chw)
    assert q_sample_v(T, x0, z, t, x_t, v) == 0 and ddpm_param_pred(T, x_t, v, t, 2, False, back) == 0
    err = float((back - x0).abs().max())
    bound = 6 * 0.5 * EPS * float((x0.abs() + z.abs()).max())
    print(f"max |predict(q_sample_v(x0, eps)) - x0| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------ 4. the top of the chain
def test_prediction_at_the_top_of_the_chain_is_within_two_ulp_of_float64():
    """the claim the design rests on, on the kernel itself at a = 2.43e-9: 65 536 standard-normal (x, v); float64 on the same rounded
    inputs.  The via-eps route (numpy fp32 emulation) is printed next to it."""
    n = 65536
    rng = np.random.default_rng(0)
    x, v = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    sa, s1 = np.sqrt(np.float32(A_TOP)), np.float32(_s1(A_TOP))
    p0 = _nan(n)
    assert param_pred(torch.from_numpy(x).to(DEV), torch.from_numpy(v).to(DEV), 2, A_TOP, s1, False, p0, None) == 0
    want = PR.pred64(x, v, PR.V, float(sa), float(s1))
    got = p0.cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(want), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    direct, via = np.abs(got - want), np.abs(PR.via_eps(x, v, A_TOP, s1).astype(np.float64) - want)
    print(f"a = {A_TOP:g}: max |error of the prediction|: kernel {direct.max():.2e} ({(direct / ulp).max():.2f} ulp), via eps {via.max():.2e}")
    assert (direct <= 2 * ulp).all()
    assert via.max() > 1000 * direct.max()


# ------------------------------------------------------------------------------------------------------------ 5. whole calls against CPU loops
T_CALL = 50


def _unet(prec, name="u_a0_tiny"):
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    cfg = unet_cfgs()[name]
    u = UNetModel(**cfg).set_precision(prec)
    u.load_state_dict(synth_state_dict(unet_param_shapes(**cfg), 7))
    return u


def _model(prec, parameterization, T=T_CALL, cond_type=None):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    return EODiffusion(_unet(prec), timesteps=T, image_size=16, in_channels=3, cond_type=cond_type, device=DEV,
                       parameterization=parameterization).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _oracle():
    from eo_diffusion_amd.backbones.unet_openai import unet_param_shapes
    from oracle import unet_ref as UR
    cfg = unet_cfgs()["u_a0_tiny"]
    sd = synth_state_dict(unet_param_shapes(**cfg), 7)
    return lambda x, t: UR.unet_forward(sd, cfg, x, t)


def _tb(m):
    """the model's own buffers on the host: what its kernels read"""
    return {k: getattr(m, k).detach().cpu() for k in ("betas", "alphas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}


@functools.lru_cache(maxsize=None)
def _inputs(n_eval):
    x_T = synth_input("cx", (2, 3, 16, 16), 91)
    noises = synth_input("cn", (n_eval, 2, 3, 16, 16), 91)
    gt = synth_input("cg", (2, 3, 16, 16), 91, uniform=True) * 2 - 1
    return x_T, noises, gt, rect_mask(2, 16, 16, 91)


@functools.lru_cache(maxsize=None)
def _ddpm_reference(kind, clip, masked):
    x_T, noises, gt, mask = _inputs(T_CALL)
    tb = SCH.eo_cosine_tables(T_CALL)
    return PR.ddpm_sampled(tb, _oracle(), KIND[kind], x_T, noises, clip, gt=gt if masked else None, mask=mask if masked else None)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_sampling_vs_cpu_loop(kind, clip, masked, prec):
    m = _model(prec, kind, cond_type="sum" if masked else None)
    tb = _tb(m)
    ref_tb = SCH.eo_cosine_tables(T_CALL)
    assert all(torch.equal(tb[k], ref_tb[k]) for k in ("betas", "alphas", "alphas_cumprod"))
    x_T, noises, gt, mask = _inputs(T_CALL)
    cond = torch.cat([gt, mask], 1).to(DEV) if masked else None
    out = m.sampling(2, clipped_reverse_diffusion=clip, device=DEV, cond=cond, x_T=x_T, noises=noises, progress=False).cpu()
    want = _ddpm_reference(kind, clip, masked)
    err = rel_l2(out, want)
    print(f"sampling T = {T_CALL} as {kind} [{prec}, clip {clip}, masked {masked}]: rel-L2 vs the CPU loop {err:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert bool(torch.isfinite(out).all()) and err < TRAJ_TOL[prec]
    if prec == "fp32x3" and not masked:
        # the first evaluation, on the model's own output: predict_x0 and the reverse step are the emulation's bits
        t = torch.full((2,), T_CALL - 1, dtype=torch.int64)
        with torch.no_grad():                                         # (as the samplers call it)
            o = m.model(x_T.to(DEV), t.to(DEV))
        p = m.predict_x0(x_T.to(DEV), t.to(DEV), o, clip=clip)
        want_p = PR.ddpm_pred(tb, x_T, o.cpu(), t, KIND[kind], clip)
        assert bits_equal(p.cpu(), want_p)
        step = (m._reverse_diffusion_with_clip if clip else m._reverse_diffusion)(x_T.to(DEV), t.to(DEV), noises[0].to(DEV))
        from tests import ancestral_ref as AR
        assert bits_equal(step.cpu(), AR.finish(tb, x_T, want_p, noises[0], t))


@functools.lru_cache(maxsize=None)
def _ddim_reference(kind, eta):
    x_T, noises, _, _ = _inputs(T_CALL)
    tb = SCH.eo_cosine_tables(T_CALL)
    steps = SCH.ddim_timesteps("uniform", 10, T_CALL)
    dd = SCH.ddim_tables(tb["alphas_cumprod"], steps, eta)
    return PR.ddim_sampled(tb, dd, steps, _oracle(), KIND[kind], x_T, noises[:len(steps)]), steps, dd


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_ddim_sample_vs_cpu_loop(kind, eta, prec):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    m = _model(prec, kind)
    x_T, noises, _, _ = _inputs(T_CALL)
    (want, want_p0, _), steps, dd = _ddim_reference(kind, eta)
    s = DDIMSampler(m)
    out, inter = s.sample(10, 2, (3, 16, 16), eta=eta, x_T=x_T, verbose=False, log_every_t=1, step_noises=noises[:len(steps)], progress=False)
    assert np.array_equal(np.asarray(s.ddim_timesteps, np.int64), steps)
    e_out, e_p0 = rel_l2(out.cpu(), want), rel_l2(inter["pred_x0"][-1].cpu(), want_p0)
    print(f"DDIM S = 10 as {kind} [{prec}, eta {eta}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]
    if prec == "fp32x3":                                             # the first evaluation on the model's own output: the emulation's bits
        index = len(steps) - 1
        ts = torch.full((2,), int(steps[index]), dtype=torch.long)
        with torch.no_grad():                                         # (as the samplers call it)
            o = m.model(x_T.to(DEV), ts.to(DEV)).cpu()
        p, e = PR.pred(x_T, o, KIND[kind], float(dd["a"][index]), float(dd["sqrt_1m_a"][index]))
        assert bits_equal(inter["pred_x0"][1].cpu(), p)
        assert bits_equal(inter["x_inter"][1].cpu(), PR.ddim_finish(e, p, noises[0], float(dd["a_prev"][index]), float(dd["sigma"][index])))


@functools.lru_cache(maxsize=None)
def _dpm_reference(kind, clip):
    x_T = _inputs(T_CALL)[0]
    tb = SCH.eo_cosine_tables(T_CALL)
    levels = make_dpm_timesteps("logsnr", 8, tb["alphas_cumprod"].numpy())
    return PR.dpm_sampled(tb, levels, _oracle(), KIND[kind], x_T, 2, clip), levels


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_dpm_sample_vs_cpu_loop(kind, clip, prec):
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    m = _model(prec, kind)
    x_T = _inputs(T_CALL)[0]
    (want, want_p0, _), levels = _dpm_reference(kind, clip)
    s = DPMSolverSampler(m)
    out, inter = s.sample(8, 2, (3, 16, 16), order=2, clip_denoised=clip, x_T=x_T, log_every_t=1, progress=False)
    assert np.array_equal(np.asarray(s.dpm_timesteps, np.int64), np.asarray(levels, np.int64))
    e_out, e_p0 = rel_l2(out.cpu(), want), rel_l2(inter["pred_x0"][-1].cpu(), want_p0)
    print(f"DPM-Solver++ S = 8 as {kind} [{prec}, clip {clip}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]
    if prec == "fp32x3":
        a, s1m, _, _ = DR.tables(SCH.eo_cosine_tables(T_CALL)["alphas_cumprod"].numpy(), levels)
        ts = torch.full((2,), int(levels[-1]), dtype=torch.long)
        with torch.no_grad():                                         # (as the samplers call it)
            o = m.model(x_T.to(DEV), ts.to(DEV)).cpu()
        assert bits_equal(inter["pred_x0"][1].cpu(), PR.pred(x_T, o, KIND[kind], a[-1], s1m[-1], clip, with_e=False)[0])


# ------------------------------------------------------------------------------------------------------------ 6. guidance, observations, thresholds
GUIDED_CFG = dict(image_size=16, in_channels=7, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[2],
                  channel_mult=[1, 2], num_heads=2)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_guided_ddim_call_as_v_vs_cpu_loop(prec):
    """classifier-free guidance (scale 3, concatenated conditioning): the RAW outputs are combined, then read as v"""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from oracle import unet_ref as UR
    sd = synth_state_dict(unet_param_shapes(**GUIDED_CFG), 7)
    u = UNetModel(**GUIDED_CFG).set_precision(prec)
    u.load_state_dict(sd)
    m = EODiffusion(u, timesteps=T_CALL, image_size=16, in_channels=3, device=DEV, parameterization="v").to(DEV).eval()
    x_T, noises, _, _ = _inputs(T_CALL)
    c = synth_input("gc", (2, 4, 16, 16), 51, uniform=True)
    uc = torch.zeros_like(c)

    def out_fn(x, t):
        e_u, e_c = UR.unet_forward(sd, GUIDED_CFG, x, t, cond=uc), UR.unet_forward(sd, GUIDED_CFG, x, t, cond=c)
        d = e_c - e_u
        return e_u + 3.0 * d

    tb = SCH.eo_cosine_tables(T_CALL)
    steps = SCH.ddim_timesteps("uniform", 10, T_CALL)
    dd = SCH.ddim_tables(tb["alphas_cumprod"], steps, 0.5)
    want, want_p0, _ = PR.ddim_sampled(tb, dd, steps, out_fn, PR.V, x_T, noises[:len(steps)])
    out, inter = DDIMSampler(m).sample(10, 2, (3, 16, 16), conditioning=c.to(DEV), eta=0.5, x_T=x_T, verbose=False, log_every_t=1,
                                       unconditional_guidance_scale=3.0, unconditional_conditioning=uc.to(DEV), step_noises=noises[:len(steps)],
                                       progress=False)
    e_out, e_p0 = rel_l2(out.cpu(), want), rel_l2(inter["pred_x0"][-1].cpu(), want_p0)
    print(f"guided DDIM as v [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


FACTORS3 = (1, 2, 4)


def _observation(seed, weight=1.0):
    values = CR.block_mean(synth_input("wv", (2, 3, 16, 16), seed, uniform=True) * 2 - 1, FACTORS3)
    return Observation(values, FACTORS3, weight=weight), values


def _residual(p0, values):
    """max |block_mean(pred_x0) - values| with the bound of tests/test_gpu_consistency.py test_residual_against_the_emulations: the emulation
    stays below 3 eps * max(1, |p0|max), the GPU within 4 x of the emulation"""
    res = float((CO.block_mean(p0.clone(), FACTORS3).cpu() - values).abs().max())
    return res, 4 * 3 * EPS * max(1.0, float(p0.abs().max()))


@pytest.mark.parametrize("which", ["ddim", "dpm", "ddpm"])
def test_observations_and_thresholds_as_v(which):
    """an Observation, a two-link list and a DynamicThreshold (in front of an Observation) under v: the final prediction, re-observed, meets
    the LAST link's observation at the gates of the eps tests; the single Observation is bit-equal to the same call given as a list of one"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    m = _model("fp32x3", "v", T=20)
    x_T, noises, _, _ = _inputs(T_CALL)
    noises = noises[:20]
    first, v1 = _observation(61)
    last, v2 = _observation(62)

    def call(**kw):
        if which == "ddim":
            out, inter = DDIMSampler(m).sample(8, 2, (3, 16, 16), eta=0.5, x_T=x_T, verbose=False, step_noises=noises[:10], progress=False, **kw)
            return out, inter["pred_x0"][-1]
        if which == "dpm":
            out, inter = DPMSolverSampler(m).sample(8, 2, (3, 16, 16), x_T=x_T, progress=False, **kw)
            return out, inter["pred_x0"][-1]
        out = m.sampling(2, device=DEV, x_T=x_T, noises=noises, progress=False, **kw)
        return out, out                                                # (at t = 0 the posterior step returns the prediction: out = (beta_0 / (1 - acp_0)) p0)

    free, _ = call()
    scale = float(m.betas[0] / (1.0 - m.alphas_cumprod[0])) if which == "ddpm" else 1.0
    for name, kw, values in (("one", dict(observation=first), v1), ("two links", dict(observation=[first, last]), v2),
                             ("threshold + one", dict(threshold=DynamicThreshold(0.9), observation=last), v2)):
        out, p0 = call(**kw)
        res, bound = _residual(p0 / scale if scale != 1.0 else p0, values)
        if scale != 1.0:
            bound += 2 * EPS * float(p0.abs().max())                  # (the step's product and this test's division by it)
        print(f"{which} as v, {name}: max |block mean of pred_x0 - values| = {res / EPS:.2f} eps (bound {bound / EPS:.2f} eps)")
        assert bool(torch.isfinite(out).all()) and res <= bound
        assert rel_l2(out.cpu(), free.cpu()) > 1e-3                    # (the observation matters)
    one, p_one = call(observation=first)
    listed, p_listed = call(observation=[first])
    assert torch.equal(one, listed) and torch.equal(p_one, p_listed)
    thr = DynamicThreshold(0.9)
    out, p0 = call(threshold=thr)
    if which != "ddpm":
        assert float(p0.abs().max()) <= 1.0 and bool((thr.last_bound.last_scale >= 1.0).all())


# ------------------------------------------------------------------------------------------------------------ 7. the toy on the GPU
class ToyOutput(torch.nn.Module):
    """stands in for EODiffusion.model: the closed-form denoiser of tests/dpm_ref.py's Gaussian pixels in fp32 on the device, returning eps,
    x0 or v.  E[x0 | x] = mu + sa s^2 (x - sa mu) / (a s^2 + 1 - a) is written out (forming it from eps would cancel at high noise)."""

    def __init__(self, acp, kind):
        super().__init__()
        mu, s, _ = DR.toy()
        self.mu, self.s2 = (torch.from_numpy(v).float().to(DEV).view(1, 1, 64, 64) for v in (mu, s * s))
        self.acp, self.kind = acp.to(DEV), kind

    def forward(self, x, t, cond=None, y=None):
        a = self.acp[t].view(-1, 1, 1, 1)
        sa, s1 = torch.sqrt(a), torch.sqrt(1.0 - a)
        r = (x - sa * self.mu) / (a * self.s2 + 1.0 - a)
        e, p0 = s1 * r, self.mu + sa * self.s2 * r
        return e if self.kind == 0 else (p0 if self.kind == PR.X0 else sa * e - s1 * p0)


@pytest.mark.parametrize("kind", ["x0", "v"])
def test_the_toy_on_the_gpu(kind):
    """DPM-Solver++ at S in {25, 100}: the GPU's toy error within 5e-5 of the float64 loop's (100 steps x 4 roundings x 6e-8, doubled, as
    tests/test_gpu_dpm_solver.py derives it); DDIM eta 0 at S = 250: 1.2e-4, the same derivation with 250 steps"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion
    T = 1000
    m = EODiffusion(torch.nn.Identity(), timesteps=T, image_size=64, in_channels=1, device=DEV, parameterization=kind).to(DEV)
    acp = m.alphas_cumprod.cpu().numpy()
    m.model = ToyOutput(m.alphas_cumprod, KIND[kind])
    x_T = torch.from_numpy(DR.toy()[2]).float().view(1, 1, 64, 64)
    smp = DPMSolverSampler(m)
    for S in (25, 100):
        out, _ = smp.sample(S, 1, (1, 64, 64), order=2, x_T=x_T, progress=False)
        host, levels = PR.dpm_f64(acp, S, 2, "logsnr", KIND[kind])
        e, host_e = DR.toy_error(out.cpu().numpy(), acp, levels[-1]), DR.toy_error(host, acp, levels[-1])
        print(f"toy as {kind}, DPM-Solver++ S = {S}: {e:.6e} on the GPU, {host_e:.6e} in float64, difference {abs(e - host_e):.1e}")
        assert abs(e - host_e) < 5e-5
    d = DDIMSampler(m)
    out, _ = d.sample(250, 1, (1, 64, 64), eta=0.0, x_T=x_T, verbose=False, progress=False)
    levels = np.asarray(d.ddim_timesteps, np.int64)
    host = PR.ddim_f64(acp, levels, KIND[kind])
    e, host_e = DR.toy_error(out.cpu().numpy(), acp, int(levels[-1])), DR.toy_error(host, acp, int(levels[-1]))
    print(f"toy as {kind}, DDIM eta 0 S = 250: {e:.6e} on the GPU, {host_e:.6e} in float64, difference {abs(e - host_e):.1e}")
    assert abs(e - host_e) < 1.2e-4


# ------------------------------------------------------------------------------------------------------------ 8. scenes as v
_SCENE_UNETS = {}


def _scene_model(prec="fp32x3", T=6, cond_type=None, parameterization="v"):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    if prec not in _SCENE_UNETS:
        _SCENE_UNETS[prec] = _unet(prec).to(DEV).eval()
    return EODiffusion(_SCENE_UNETS[prec], timesteps=T, image_size=16, in_channels=3, cond_type=cond_type, device=DEV,
                       parameterization=parameterization).to(DEV).eval()


def _cut(scene, plan):
    s = plan.tile
    return torch.cat([scene[:, :, y0:y0 + s, x0:x0 + s] for y0, x0 in plan.origins()]).contiguous()


def _stitch(tiles, plan):
    s = plan.tile
    out = torch.empty((1, tiles.shape[1], plan.H, plan.W), dtype=tiles.dtype, device=tiles.device)
    for i, (y0, x0) in enumerate(plan.origins()):
        out[0, :, y0:y0 + s, x0:x0 + s] = tiles[i]
    return out


H, W = 40, 56


def _known_scene(seed, B=1):
    gt = synth_input("kg", (B, 3, H, W), seed, uniform=True) * 2 - 1
    mask = np.ones((H, W), np.float32)
    mask[14:20, 10:30] = 0.0
    return gt, mask, torch.cat([gt, torch.from_numpy(mask)[None, None].expand(B, 1, H, W)], 1)


def test_scene_with_overlap_0_equals_the_samplers_on_the_tiles_as_v():
    """a scene that 16 x 16 tiles partition (32 x 48; at 40 x 56 the last row and column of tiles overlap their neighbours, and overlap 0
    is no partition): sampling_scene against sampling, DPMSolverSampler.sample_scene against sample, DDIMSampler likewise"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    T = 6
    m = _scene_model(T=T)
    plan = TilePlan(32, 48, 16, 0)
    x_T, noises = synth_input("sx", (1, 3, 32, 48), 21), synth_input("sn", (T, 1, 3, 32, 48), 21)
    per_tile = torch.stack([_cut(noises[k], plan) for k in range(T)])
    for clip in (True, False):
        scene = m.sampling_scene((32, 48), clip, DEV, x_T=x_T, noises=noises, progress=False)
        tiles = m.sampling(6, clip, DEV, x_T=_cut(x_T, plan), noises=per_tile, progress=False)
        assert bool(torch.isfinite(scene).all()) and torch.equal(scene, _stitch(tiles, plan))
    smp = DPMSolverSampler(m)
    scene, inter = smp.sample_scene(4, (32, 48), x_T=x_T, progress=False)
    tiles, inter_t = smp.sample(4, 6, (3, 16, 16), x_T=_cut(x_T, plan), progress=False)
    assert torch.equal(scene, _stitch(tiles, plan)) and torch.equal(inter["pred_x0"][-1], _stitch(inter_t["pred_x0"][-1], plan))
    ddim = DDIMSampler(m)
    scene, _ = ddim.sample_scene(3, (32, 48), eta=1.0, x_T=x_T, step_noises=noises[:3], progress=False)
    tiles, _ = ddim.sample(3, 6, (3, 16, 16), eta=1.0, x_T=_cut(x_T, plan), verbose=False, progress=False, step_noises=per_tile[:3])
    assert torch.equal(scene, _stitch(tiles, plan))


def test_scene_identities_as_v():
    """40 x 56, image size 16, overlap 4: tile_batch never shows; skip_known equals the full call at estimated pixels and is x0 elsewhere;
    member 1 of a stack of three equals the single call; the sharded call on one rank equals the direct call.  All torch.equal."""
    from eo_diffusion_amd import dist as D
    from tests.test_gpu_scene_skip import assert_skip_equals_full, classes
    T = 6
    m = _scene_model(T=T, cond_type="sum")
    plan = TilePlan(H, W, 16, 4)
    gt, mask, cond = _known_scene(33)
    _, _, est = classes(plan, mask)
    kw = dict(cond=cond, overlap=4, rng="philox", seed=9, progress=False)
    full = m.sampling_scene((H, W), True, DEV, tile_batch=16, **kw)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(m.sampling_scene((H, W), True, DEV, tile_batch=3, **kw), full)
    skip = m.sampling_scene((H, W), True, DEV, tile_batch=3, skip_known=True, **kw)
    assert_skip_equals_full(skip, full, gt, est, "sampling_scene as v")
    gt3, _, cond3 = _known_scene(34, B=3)
    stack = m.sampling_scene((H, W), True, DEV, n_scenes=3, **dict(kw, cond=cond3))
    single = m.sampling_scene((H, W), True, DEV, sample_offset=1, **dict(kw, cond=cond3[1:2]))
    assert stack.shape == (3, 3, H, W) and torch.equal(stack[1:2], single)
    assert torch.equal(D.sharded_sampling_scene(m, (H, W), 3, seed=9, cond=cond3, overlap=4, device=DEV), stack)
    # ... and the batch call: sharded_sampling on one rank is sampling
    plain = _scene_model(T=T)
    assert torch.equal(D.sharded_sampling(plain, 3, seed=9, device=DEV), plain.sampling(3, device=DEV, rng="philox", seed=9, progress=False))


# ------------------------------------------------------------------------------------------------------------ 9. training
GTOL = {"fp32": 2e-4, "fp16": 1e-2}                      # the gates of tests/test_gpu_training.py


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["x0", "v"])
def test_one_training_step_vs_autograd_of_the_oracle(kind, prec):
    """pred, target = model(x, noise, t=t, return_target=True); diffusion_loss(pred, target, weight = min-SNR of the target) on the tiny
    attention UNet at batch 4: the target, the loss and every parameter gradient against the oracle with the target formed on the CPU"""
    from eo_diffusion_amd import optim
    from eo_diffusion_amd.backbones import unet_openai as U
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from oracle import unet_ref as UR
    cfg = unet_cfgs()["u_a1_tiny"]
    sd = synth_state_dict(U.unet_param_shapes(**cfg), 11)
    unet = U.UNetModel(**cfg).set_precision(prec)
    unet.load_state_dict(sd)
    model = EODiffusion(unet, timesteps=1000, image_size=16, in_channels=3, parameterization=kind).to(DEV).train()
    x, noise = synth_input("trx", (4, 3, 16, 16), 3, uniform=True) * 2 - 1, synth_input("trn", (4, 3, 16, 16), 4)
    t = torch.tensor([7, 650, 999, 0])
    table = model.loss_weights("min_snr", 5.0)
    assert torch.equal(table, model.loss_weights("min_snr", 5.0, parameterization=kind))
    pred, target = model(x.to(DEV), noise.to(DEV), t=t.to(DEV), return_target=True)
    weight = table[t.to(DEV)]
    loss, dpred = optim.diffusion_loss(pred, target, weight=weight)
    pred.backward(dpred)
    torch.cuda.synchronize()
    # the CPU side
    tb = _tb(model)
    x_t, v = PR.q_sample_v(tb, x, noise, t)
    want_target = v if kind == "v" else x
    assert bits_equal(target.cpu(), want_target)
    assert bits_equal(model.target(x.to(DEV), noise.to(DEV), t.to(DEV)).cpu(), want_target)
    sdg = {k: p.clone().requires_grad_(True) for k, p in sd.items()}
    ref_pred = UR.unet_forward(sdg, cfg, x_t, t)
    w = table.cpu()[t]
    ref_loss = (w * ((ref_pred - want_target) ** 2).reshape(4, -1).mean(1)).mean()
    ref_loss.backward()
    e_loss = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    print(f"training step as {kind} [{prec}]: loss {float(loss):.6f} vs {float(ref_loss):.6f} (rel {e_loss:.2e}), weights {w.tolist()}")
    assert e_loss < GTOL[prec]
    gref = {k: p.grad for k, p in sdg.items() if p.grad is not None}
    gmax = max(float(g.norm()) for g in gref.values())
    worst, n_checked = ("", 0.0), 0
    for name, p in model.model.named_parameters():
        if name not in gref:
            continue
        assert p.grad is not None and p.grad.shape == p.shape, name
        if float(gref[name].norm()) < 1e-5 * gmax:                   # mathematically-zero gradients: round-off only
            assert float(p.grad.norm()) < 1e-3 * gmax, name
            continue
        e = rel_l2(p.grad.cpu(), gref[name])
        n_checked += 1
        if e > worst[1]:
            worst = (name, e)
    print(f"training step as {kind} [{prec}]: worst gradient {worst} over {n_checked} tensors (gate {GTOL[prec]:g})")
    assert n_checked > 20 and worst[1] < GTOL[prec], worst


def test_return_target_under_eps_returns_todays_tensor():
    from eo_diffusion_amd.diffusion.model import EODiffusion
    m = EODiffusion(_unet("fp32x3"), timesteps=1000, image_size=16, in_channels=3).to(DEV).eval()
    x, noise = synth_input("trx", (2, 3, 16, 16), 3).to(DEV), synth_input("trn", (2, 3, 16, 16), 4).to(DEV)
    t = torch.tensor([7, 650], device=DEV)
    with torch.no_grad():
        today = m(x, noise, t=t)
        assert torch.equal(m(x, noise, t=t, return_target=False), today)
        pred, target = m(x, noise, t=t, return_target=True)
    assert torch.equal(pred, today) and target is noise
    x0_model = EODiffusion(m.model, timesteps=1000, image_size=16, in_channels=3, parameterization="x0").to(DEV).eval()
    with torch.no_grad():
        pred, target = x0_model(x, noise, t=t, return_target=True)
    assert torch.equal(pred, today) and target is x


# ------------------------------------------------------------------------------------------------------------ 10. the default route is unchanged
class _Net(torch.nn.Module):
    """a stand-in for the UNet that launches nothing of the library: the record sees the samplers' own launches"""

    def forward(self, x, t, cond=None, y=None):
        return (x * 0.25).contiguous()


def _record(monkeypatch):
    L = _lib.lib()
    called = collections.Counter()

    def wrap(name, fn):
        def w(*a):
            called[name] += 1
            return fn(*a)
        w.__name__ = name
        return w
    for name in list(_lib.SYMBOLS) + list(_lib.PARAM_SYMBOLS):
        monkeypatch.setattr(L, name, wrap(name, getattr(L, name)))
    return called


def _every_call(m, n_evals):
    """sampling, DDIMSampler.sample, DPMSolverSampler.sample and the training forward; n_evals receives the evaluations of each"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    n, S = 2, 8
    outs = [m.sampling(n, True, device=DEV, progress=False), m.sampling(n, False, device=DEV, progress=False)]
    n_evals["ddpm"] = 2 * m.timesteps
    d = DDIMSampler(m)
    outs.append(d.sample(3, n, (3, S, S), eta=0.5, verbose=False, progress=False)[0])
    n_evals["ddim"] = len(d.ddim_timesteps)
    s = DPMSolverSampler(m)
    outs.append(s.sample(4, n, (3, S, S), order=2, progress=False)[0])
    n_evals["dpm"] = s.num_evaluations
    x = torch.randn(n, 3, S, S, device=DEV)
    outs.append(m(x, torch.randn_like(x), t=torch.tensor([1, 4], device=DEV)))
    outs.append(m(x, torch.randn_like(x), t=torch.tensor([1, 4], device=DEV), return_target=True)[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in outs)


def test_default_model_takes_todays_calls_and_a_v_model_one_prediction_per_evaluation(monkeypatch):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    called = _record(monkeypatch)
    n_evals = {}
    _every_call(EODiffusion(_Net(), timesteps=6, image_size=8, in_channels=3).to(DEV), n_evals)
    assert not any(called[k] for k in NEW), {k: called[k] for k in NEW}
    assert called["eod_ddpm_step"] == n_evals["ddpm"] and called["eod_ddim_step"] == n_evals["ddim"] and called["eod_dpmpp_step"] == n_evals["dpm"]
    assert called["eod_q_sample"] == 2
    for kind in ("v", "x0"):
        called.clear()
        _every_call(EODiffusion(_Net(), timesteps=6, image_size=8, in_channels=3, parameterization=kind).to(DEV), n_evals)
        print(f"calls of a {kind} model:", {k: v for k, v in sorted(called.items()) if k.startswith("eod_") and v})
        assert called["eod_ddpm_param_pred"] == n_evals["ddpm"] == called["eod_ddpm_step_p0"]
        assert called["eod_param_pred"] == n_evals["ddim"] + n_evals["dpm"]
        assert called["eod_ddim_step_p0"] == n_evals["ddim"] and called["eod_dpmpp_step_p0"] == n_evals["dpm"]
        assert not any(called[k] for k in ("eod_pred_x0", "eod_ddpm_pred_x0", "eod_ddim_step", "eod_dpmpp_step", "eod_ddpm_step"))
        # the training forward: without a target the plain forward move; with one, under v, the pair in one pass in its place
        assert (called["eod_q_sample_v"], called["eod_q_sample"]) == ((1, 1) if kind == "v" else (0, 2))
