"""GPU: learned variance (DESIGN.md sections 8.3 and 9.17) -- eod_ddpm_var_pred and eod_ddpm_step_p0_var against the existing kernels bit for
bit and against float64 within the derived sigma bound, eod_hybrid_loss against eod_diffusion_loss bit for bit (the simple term) and against
tests/var_ref.py within the float64 bound (the variational-bound term and its gradient), whole calls of every sampler on a tiny UNet with six
output channels, one training step under HybridLoss against autograd through the oracle, and the default route's launches.

The bounds are those of tests/test_var_host.py with E = 3 ulp for the device's expf: the device library's documentation states no figure, so
OpenCL's full-profile 3 ulp is allowed."""
import collections
import functools

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation
from eo_diffusion_amd.tiling import TilePlan
from oracle import schedule as SCH
from tests import param_ref as PR
from tests import var_ref as VR
from tests.gpu_util import DEV
from tests.helpers import bits_equal, rel_l2, unet_cfgs
from tests.synth import synth_input, synth_state_dict
from tests.test_gpu_sampling import TRAJ_TOL
from tests.test_var_host import K_KL, K_NLL, U24, U53, sigma_bound, step64

pytestmark = pytest.mark.gpu

T = 1000
N = 3
SHAPES = {105: (3, 5, 7), 192: (3, 8, 8)}                # chw: the element path (no multiple of 4) and the quad path
KINDS = {"eps": 0, "x0": 1, "v": 2}
E_DEVICE = 3.0
SUM_SLACK = 32.0                                          # additions an element passes on either side of a float64 sum of <= 192 terms, both sides


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _offset_by_4_bytes(t):
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


@functools.lru_cache(maxsize=None)
def _tables(T_):
    tb = SCH.eo_cosine_tables(T_)
    vt = VR.tables64(tb)
    dev = {k: v.to(DEV).contiguous() for k, v in tb.items()}
    dev.update({k: vt[k].to(DEV) for k in ("sigma_min", "half_gap")})
    dev.update({k: torch.from_numpy(vt[k]).to(DEV) for k in ("c1", "lmin", "gap")})
    return tb, vt, dev


def _rand(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def var_pred(x, o, t, kind, clip, p0, N_=None, chw=None, T_=T):
    d = _tables(T)[2]
    return _lib.lib().eod_ddpm_var_pred(_lib.ptr(x), _lib.ptr(o), _lib.ptr(t), d["alphas_cumprod"].data_ptr(), d["sqrt_alphas_cumprod"].data_ptr(),
                                        d["sqrt_one_minus_alphas_cumprod"].data_ptr(), kind, int(clip), _lib.ptr(p0), N if N_ is None else N_,
                                        (p0.numel() // N) if chw is None else chw, T_, _stream())


def step_var(x, p0, o, z, t, out, N_=None, chw=None, T_=T):
    d = _tables(T)[2]
    return _lib.lib().eod_ddpm_step_p0_var(_lib.ptr(x), _lib.ptr(p0), _lib.ptr(o), _lib.ptr(z), _lib.ptr(t), d["betas"].data_ptr(),
                                           d["alphas"].data_ptr(), d["alphas_cumprod"].data_ptr(), d["sigma_min"].data_ptr(),
                                           d["half_gap"].data_ptr(), _lib.ptr(out), N if N_ is None else N_,
                                           (out.numel() // N) if chw is None else chw, T_, _stream())


def step_p0(x, p0, z, t, out):
    d = _tables(T)[2]
    return _lib.lib().eod_ddpm_step_p0(x.data_ptr(), p0.data_ptr(), z.data_ptr(), t.data_ptr(), d["betas"].data_ptr(), d["alphas"].data_ptr(),
                                       d["alphas_cumprod"].data_ptr(), out.data_ptr(), N, out.numel() // N, T, _stream())


def _output(seed, chw, nan_half=None):
    """o [N, 2 C, H, W] on the host; one half NaN on request"""
    c, h, w = SHAPES[chw]
    o = _rand(seed, N, 2 * c, h, w, scale=1.2)
    if nan_half is not None:
        o[:, nan_half * c:(nan_half + 1) * c] = float("nan")
    return o


# ------------------------------------------------------------------------------------------------------------ 1. eod_ddpm_var_pred
@pytest.mark.parametrize("unaligned", [None, "x", "o", "p0"])
@pytest.mark.parametrize("chw", [105, 192])
@pytest.mark.parametrize("kind", ["eps", "x0", "v"])
def test_var_pred_is_the_existing_prediction_on_the_mean_half(kind, chw, unaligned):
    _, _, d = _tables(T)
    c, h, w = SHAPES[chw]
    x = _rand(1, N, c, h, w, scale=2.0).to(DEV)
    o = _output(2, chw, nan_half=1).to(DEV)                            # the variance half is NaN: it is never read
    dense = o[:, :c].contiguous()
    for t_host in ([0, 1, T - 1], [5, T, -1]):
        t = torch.tensor(t_host, dtype=torch.int64, device=DEV)
        for clip in (True, False):
            want = CO.ddpm_pred_x0(kind, x, dense, t, d["alphas_cumprod"], d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"], clip)
            xx = _offset_by_4_bytes(x) if unaligned == "x" else x
            oo = _offset_by_4_bytes(o) if unaligned == "o" else o
            got = torch.empty_like(x)
            got = _offset_by_4_bytes(got) if unaligned == "p0" else got
            assert var_pred(xx, oo, t, KINDS[kind], clip, got) == 0
            assert same(got, want), (kind, chw, clip, t_host)
            bad = [(v < 0 or v >= T) for v in t_host]
            assert [bool(torch.isnan(got[n]).all()) for n in range(N)] == bad and not bool(torch.isnan(got[0]).any())
    # ... and the Python entry: predict_x0 accepts the 2 C output
    from eo_diffusion_amd.diffusion.model import EODiffusion
    m = EODiffusion(torch.nn.Identity(), max(h, w), c, timesteps=T, parameterization=kind, learned_variance=True).to(DEV)
    t = torch.tensor([0, 1, T - 1], device=DEV)
    assert same(m.predict_x0(x, t, o, clip=True), CO.ddpm_pred_x0(kind, x, dense, t, d["alphas_cumprod"], d["sqrt_alphas_cumprod"],
                                                                   d["sqrt_one_minus_alphas_cumprod"], True))


def test_var_pred_and_step_refusals_leave_the_output_alone():
    c, h, w = SHAPES[192]
    x, o, z = _rand(1, N, c, h, w).to(DEV), _output(2, 192).to(DEV), _rand(3, N, c, h, w).to(DEV)
    t = torch.tensor([3, 1, T - 1], dtype=torch.int64, device=DEV)
    out = torch.full_like(x, 7.0)
    bad_pred = [dict(x=None), dict(o=None), dict(t=None), dict(N_=0), dict(chw=0), dict(T_=0), dict(kind=3), dict(kind=-1)]
    for kw in bad_pred:
        a = dict(x=x, o=o, t=t, kind=0, clip=1, p0=out)
        a.update(kw)
        assert var_pred(a.pop("x"), a.pop("o"), a.pop("t"), a.pop("kind"), a.pop("clip"), a.pop("p0"), **a) == -1, kw
    assert var_pred(x, o, t, 0, 1, None, chw=192) == -1
    assert var_pred(x, o, t, 0, 1, o[:, c:]) == -1                     # the output lies on the model output
    assert var_pred(x, o, t, 0, 1, x) == -1
    for kw in (dict(x=None), dict(p0=None), dict(o=None), dict(z=None), dict(t=None), dict(N_=0), dict(chw=-1), dict(T_=0)):
        a = dict(x=x, p0=x, o=o, z=z, t=t, out=out)
        a.update(kw)
        assert step_var(a.pop("x"), a.pop("p0"), a.pop("o"), a.pop("z"), a.pop("t"), a.pop("out"), **a) == -1, kw
    assert step_var(x, x, o, z, t, o[:, :c]) == -1 and step_var(x, x, o, z, t, z) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and b"overlap" in _lib.lib().eod_last_error()


# ------------------------------------------------------------------------------------------------------------ 2. eod_ddpm_step_p0_var
@pytest.mark.parametrize("unaligned", [None, "o"])
@pytest.mark.parametrize("chw", [105, 192])
def test_var_step_against_the_fixed_variance_step_float64_and_the_emulation(chw, unaligned):
    tb, vt, _ = _tables(T)
    c, h, w = SHAPES[chw]
    x, p0, z = _rand(4, N, c, h, w, scale=2.0), _rand(5, N, c, h, w).clamp(-1, 1), _rand(6, N, c, h, w)
    o = _output(7, chw, nan_half=0)                                    # the mean half is NaN: it is never read
    pick = (lambda u: _offset_by_4_bytes(u)) if unaligned else (lambda u: u)
    xd, pd, zd, od = x.to(DEV), p0.to(DEV), z.to(DEV), pick(o.to(DEV))
    t_pos = torch.tensor([3, 1, T - 1], dtype=torch.int64)
    got, want = torch.empty_like(xd), torch.empty_like(xd)
    # z = 0: the mean alone, eod_ddpm_step_p0's bits
    zero = torch.zeros_like(zd)
    assert step_var(xd, pd, od, zero, t_pos.to(DEV), got) == 0 and step_p0(xd, pd, zero, t_pos.to(DEV), want) == 0
    assert same(got, want) and bool(torch.isfinite(got).all())
    # a member at t = 0: std = 0 for the whole batch, any z, and v is not read (all of o is NaN here)
    t_zero = torch.tensor([0, 1, T - 1], dtype=torch.int64, device=DEV)
    assert step_var(xd, pd, pick(torch.full_like(o, float("nan")).to(DEV)), zd, t_zero, got) == 0 and step_p0(xd, pd, zd, t_zero, want) == 0
    assert same(got, want) and bool(torch.isfinite(got).all())
    # an out-of-range member: NaN, the others as without it
    assert step_var(xd, pd, od, zd, torch.tensor([3, T, 7], dtype=torch.int64, device=DEV), got) == 0
    assert bool(torch.isnan(got[1]).all()) and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())
    # every member at t > 0: within the bound of float64, and the emulation's bits wherever the device's expf is the host's
    assert step_var(xd, pd, od, zd, t_pos.to(DEV), got) == 0
    flat = lambda u: u.reshape(N, -1)
    v = flat(o[:, c:])
    want64, tol = step64({k: (tb[k] if k in tb else vt[k]) for k in ("betas", "alphas", "alphas_cumprod", "sigma_min", "half_gap")},
                         flat(x), flat(p0), v, flat(z), t_pos, E_DEVICE)
    err = np.abs(flat(got.cpu()).numpy().astype(np.float64) - want64)
    emu = VR.var_step(tb, vt, x, p0, o, z, t_pos)
    general = got.cpu().clone()
    agree = float((general == emu).double().mean())
    arg = (v.numpy().astype(np.float64) + 1) * 0.5 * vt["half_gap"][t_pos].numpy().astype(np.float64)[:, None]
    print(f"step chw {chw}: worst |error| / bound {float((err / tol).max()):.3f}; bit-equal to the emulation at {100 * agree:.2f} % of the elements; "
          f"|arg| <= {np.abs(arg).max():.3f}")
    assert (err <= tol).all()
    # sigma itself, read back through z = 1 and a zero mean (x = p0 = 0): out = sigma
    one, nil = torch.ones_like(zd), torch.zeros_like(xd)
    assert step_var(nil, nil, od, one, t_pos.to(DEV), got) == 0
    sig = flat(got.cpu()).numpy().astype(np.float64)
    sig64 = vt["sigma_min"][t_pos].numpy().astype(np.float64)[:, None] * np.exp(arg)
    rel = np.abs(sig - sig64) / sig64
    print(f"sigma chw {chw}: the device loses at most {rel.max() / U24:.2f} x 2^-24 (bound {sigma_bound(arg, E_DEVICE).max() / U24:.2f} at E = {E_DEVICE:g})")
    assert (rel <= sigma_bound(arg, E_DEVICE)).all()
    # where the device's sigma is the host's -- the only operation of the step that is not correctly rounded is expf -- the step's bits are too
    view = (N, 1, 1, 1)
    host_sig = VR.sigma(o[:, c:], vt["sigma_min"][t_pos].reshape(view), vt["half_gap"][t_pos].reshape(view))
    expf_same = got.cpu() == host_sig
    print(f"expf chw {chw}: the device's sigma is the host's at {100 * float(expf_same.double().mean()):.2f} % of the elements")
    assert bool((general[expf_same] == emu[expf_same]).all()) and float(expf_same.double().mean()) > 0.5
    # v = -1: sigma_min itself
    minus = o.clone()
    minus[:, c:] = -1.0
    assert step_var(nil, nil, pick(minus.to(DEV)), one, t_pos.to(DEV), got) == 0
    assert bits_equal(flat(got.cpu()), vt["sigma_min"][t_pos][:, None].expand(N, chw).contiguous())


# ------------------------------------------------------------------------------------------------------------ 3. eod_hybrid_loss
@functools.lru_cache(maxsize=None)
def _diffusion(kind, C=3):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    return EODiffusion(torch.nn.Identity(), 8, C, timesteps=T, parameterization=kind, learned_variance=True).to(DEV)


def _loss_inputs(kind, chw, seed, t_host):
    """fp32 host tensors (o, target, x_0, x_t) that meet the reference's conditions: x_0 in [-1, 1] with some values exactly +-1, a
    prediction of the mean half within 3 standard deviations of the model's variance, v in [-1.5, 1.5]"""
    tb, vt, _ = _tables(T)
    c, h, w = SHAPES[chw]
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (N, c, h, w))
    x0.reshape(N, -1)[:, ::9] = 1.0
    x0.reshape(N, -1)[:, 4::9] = -1.0
    x0 = x0.astype(np.float32)
    noise = rng.standard_normal((N, c, h, w)).astype(np.float32)
    t = torch.tensor(t_host, dtype=torch.int64)
    x_t, _ = PR.q_sample_v(tb, torch.from_numpy(x0), torch.from_numpy(noise), t)
    v = rng.uniform(-1.5, 1.5, (N, c, h, w))
    mean = np.empty((N, c, h, w))
    for n, tn in enumerate(t_host):
        sa, s1, c1 = vt["sqrt_alphas_cumprod"][tn], vt["sqrt_one_minus_alphas_cumprod"][tn], vt["c1"][tn]
        std = np.exp(0.5 * (vt["lmin"][tn] + (v[n] + 1) / 2 * vt["gap"][tn]))
        p0 = x0[n] + rng.uniform(-3, 3, (c, h, w)) * std / c1 if tn else (x0[n] + rng.uniform(-3, 3, (c, h, w)) * std) / c1
        xt = x_t[n].numpy().astype(np.float64)
        mean[n] = p0 if kind == "x0" else ((sa * xt - p0) / s1 if kind == "v" else (xt - sa * p0) / s1)
    o = torch.from_numpy(np.concatenate([mean, v], 1).astype(np.float32))
    target = torch.from_numpy(rng.standard_normal((N, c, h, w)).astype(np.float32))
    return o, target, torch.from_numpy(x0), x_t, t


def _masks(which, chw, seed):
    c, h, w = SHAPES[chw]
    rng = np.random.default_rng(seed)
    if which is None:
        return None
    shape = (1, 1, h, w) if which == "11" else (N, c, h, w)
    m = (rng.random(shape) < 0.7).astype(np.float32) * rng.choice([1.0, 0.5, 2.0], shape).astype(np.float32)
    return torch.from_numpy(m)


def _check_against_reference(kind, chw, lkind, mask, weight, ins, lam=1e-3):
    from eo_diffusion_amd import optim
    _, vt, _ = _tables(T)
    o, target, x0, x_t, t = ins
    c = SHAPES[chw][0]
    dev = lambda u: None if u is None else u.to(DEV)
    loss, grad, simple, vlb = optim.hybrid_loss(dev(o), dev(target), dev(x0), dev(x_t), dev(t), _diffusion(kind), mask=dev(mask), weight=dev(weight),
                                                kind=lkind, delta=0.75, vlb_weight=lam, return_terms=True)
    # the simple term: eod_diffusion_loss on a dense copy of the mean half, bit for bit
    l0, g0, s0 = optim.diffusion_loss(dev(o)[:, :c].contiguous(), dev(target), mask=dev(mask), weight=dev(weight), kind=lkind, delta=0.75,
                                      return_per_sample=True)
    assert bits_equal(simple, s0) and bits_equal(grad[:, :c].contiguous(), g0)
    # the variational-bound term: float64
    nm = lambda u: None if u is None else u.numpy()
    ref = VR.hybrid64(vt, nm(o), nm(target), nm(x0), nm(x_t), t.tolist(), KINDS[kind], nm(mask), nm(weight), lkind, 0.75, lam)
    lv = np.stack([vt["lmin"][tn] + (o[n, c:].numpy().astype(np.float64) + 1) / 2 * vt["gap"][tn] for n, tn in enumerate(t.tolist())])
    p0 = np.stack([VR.p0_64(KINDS[kind], x_t[n].numpy().astype(np.float64), o[n, :c].numpy().astype(np.float64), vt["sqrt_alphas_cumprod"][tn],
                            vt["sqrt_one_minus_alphas_cumprod"][tn]) for n, tn in enumerate(t.tolist())])
    c1 = np.array([vt["c1"][tn] for tn in t.tolist()])[:, None, None, None]
    t0 = np.array([tn == 0 for tn in t.tolist()])[:, None, None, None]
    x64 = x0.numpy().astype(np.float64)
    VR.check_conditions(ref, x64, np.where(t0, x64 - c1 * p0, c1 * (x64 - p0)), lv)        # x_0 - mu_theta (t = 0), mu_q - mu_theta (t > 0)
    K = np.array([K_NLL if tn == 0 else K_KL for tn in t.tolist()])
    e_vlb = np.abs(vlb.cpu().numpy() - ref["vlb"]) / (U53 * np.maximum(ref["vlb_scale"], 1e-300))
    gap = np.array([vt["gap"][tn] for tn in t.tolist()])[:, None, None, None]
    m = np.ones(target.shape) if mask is None else np.broadcast_to(mask.numpy().astype(np.float64), target.shape)
    S = m.reshape(N, -1).sum(1)[:, None, None, None]
    gv = grad[:, c:].cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(ref["gv"]).astype(np.float32)).astype(np.float64)
    tol_g = K[:, None, None, None] * U53 * (ref["scale"] + 1.0) * gap * (lam / (N * np.maximum(S, 1e-300))) * m + ulp
    e_g = np.abs(gv - ref["gv"]) / tol_g
    e_loss = abs(float(loss) - ref["loss"]) / max(abs(ref["loss"]), 1e-30)
    print(f"hybrid [{kind}, chw {chw}, {lkind}]: vlb within {e_vlb.max():.2f} units of 2^-53 x scale (gates {K.tolist()} + {SUM_SLACK:g}), "
          f"v gradient within {e_g.max():.3f} of its bound, loss rel {e_loss:.1e}; V_n {ref['vlb'].tolist()}")
    assert (e_vlb <= K + SUM_SLACK).all() and (e_g <= 1.0).all() and e_loss <= 4 * U24
    assert bool((grad[:, c:].cpu()[torch.from_numpy(m == 0)] == 0).all())
    return loss, grad, simple, vlb


@pytest.mark.parametrize("mask", [None, "11", "NC"])
@pytest.mark.parametrize("lkind", ["l2", "l1", "huber"])
def test_hybrid_loss_simple_term_bits_and_vlb_against_float64(lkind, mask):
    """t = 0 and t > 0 in one batch; the three parameterizations over the two shapes"""
    for kind, chw in (("eps", 105), ("x0", 192), ("v", 105)):
        ins = _loss_inputs(kind, chw, 11, [0, 1, T - 1])
        w = torch.tensor([0.5, 2.0, 1.25]) if mask != "11" else None
        _check_against_reference(kind, chw, lkind, _masks(mask, chw, 3), w, ins)


def test_hybrid_loss_masked_nan_full_mask_batch_independence_and_bad_timesteps():
    from eo_diffusion_amd import optim
    kind, chw = "eps", 105
    c = SHAPES[chw][0]
    ins = _loss_inputs(kind, chw, 12, [0, 400, 7])
    mask = _masks("NC", chw, 4)
    mask[1] = 0.0                                                     # a fully masked sample
    loss, grad, simple, vlb = _check_against_reference(kind, chw, "l2", mask, None, ins)
    assert float(simple[1]) == 0.0 and float(vlb[1]) == 0.0 and bool((grad[1] == 0).all())
    # NaN (and inf) under a zero mask: the same bits
    o, target, x0, x_t, t = (u.clone() for u in ins)
    hole = mask == 0
    o[:, :c][hole], o[:, c:][hole], target[hole], x0[hole], x_t[hole] = float("nan"), float("inf"), float("nan"), float("nan"), float("-inf")
    dev = lambda u: u.to(DEV)
    l2, g2, s2, v2 = optim.hybrid_loss(dev(o), dev(target), dev(x0), dev(x_t), dev(t), _diffusion(kind), mask=dev(mask), delta=0.75,
                                       return_terms=True)
    assert bits_equal(l2, loss) and bits_equal(g2, grad) and bits_equal(s2, simple) and torch.equal(v2, vlb)
    # sample 0's bits do not depend on what else is in the batch
    other = _loss_inputs(kind, chw, 99, [0, 3, 900])
    mixed = [torch.cat([a[:1], b[1:]]) for a, b in zip(ins, other)]
    l3, g3, s3, v3 = optim.hybrid_loss(*(dev(u) for u in mixed), _diffusion(kind), mask=dev(mask), delta=0.75, return_terms=True)
    assert bits_equal(s3[:1], simple[:1]) and torch.equal(v3[:1], vlb[:1]) and bits_equal(g3[:1].contiguous(), grad[:1].contiguous())
    # without a gradient: the same scalars
    l4, none = optim.hybrid_loss(*(dev(u) for u in ins), _diffusion(kind), mask=dev(mask), delta=0.75, want_grad=False)
    assert none is None and bits_equal(l4, loss)
    # a timestep outside [0, T) poisons its sample (a device tensor: no host check)
    tt = torch.tensor([0, T, 7], device=DEV)
    l5, g5, s5, v5 = optim.hybrid_loss(*(dev(u) for u in ins[:4]), tt, _diffusion(kind), return_terms=True)
    assert bool(torch.isnan(g5[1]).all()) and bool(torch.isnan(s5[1])) and bool(torch.isnan(v5[1])) and bool(torch.isnan(l5).all())
    assert bool(torch.isfinite(g5[0]).all()) and bool(torch.isfinite(g5[2]).all())


def test_hybrid_loss_refusals_leave_the_outputs_alone():
    L = _lib.lib()
    _, _, d = _tables(T)
    c, h, w = SHAPES[105]
    ins = [u.to(DEV) for u in _loss_inputs("eps", 105, 5, [0, 1, 7])]
    o, target, x0, x_t, t = ins
    loss, simple = torch.full((1,), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
    vlb, grad = torch.full((N,), 7.0, dtype=torch.float64, device=DEV), torch.full_like(o, 7.0)
    nbytes = L.eod_hybrid_loss_workspace_size(N, c, h, w)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)

    def call(**kw):
        a = dict(o=o, target=target, x0=x0, x_t=x_t, t=t, mask=None, mask_n=0, mask_c=0, weight=None, sa=d["sqrt_alphas_cumprod"],
                 s1=d["sqrt_one_minus_alphas_cumprod"], c1=d["c1"], lmin=d["lmin"], gap=d["gap"], N=N, C=c, H=h, W=w, T=T, pk=0, kind=0, delta=1.0,
                 lam=1e-3, h=1 / 255, loss=loss, simple=simple, vlb=vlb, grad=grad, ws=ws, nbytes=nbytes)
        a.update(kw)
        p = _lib.ptr
        return L.eod_hybrid_loss(p(a["o"]), p(a["target"]), p(a["x0"]), p(a["x_t"]), p(a["t"]), p(a["mask"]), a["mask_n"], a["mask_c"], p(a["weight"]),
                                 p(a["sa"]), p(a["s1"]), p(a["c1"]), p(a["lmin"]), p(a["gap"]), a["N"], a["C"], a["H"], a["W"], a["T"], a["pk"], a["kind"],
                                 a["delta"], a["lam"], a["h"], p(a["loss"]), p(a["simple"]), p(a["vlb"]), p(a["grad"]), p(a["ws"]), a["nbytes"], _stream())
    bad = [dict(o=None), dict(target=None), dict(x0=None), dict(x_t=None), dict(t=None), dict(sa=None), dict(c1=None), dict(gap=None), dict(loss=None),
           dict(simple=None), dict(vlb=None), dict(ws=None), dict(N=0), dict(C=0), dict(H=-1), dict(T=0), dict(pk=3), dict(kind=3), dict(kind=2, delta=0.0),
           dict(lam=float("nan")), dict(h=0.0), dict(h=float("inf")), dict(mask=target, mask_n=2, mask_c=c), dict(nbytes=nbytes - 8),
           dict(grad=o), dict(grad=target), dict(simple=x0), dict(loss=x_t), dict(vlb=ws)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(bool((u == 7.0).all()) for u in (loss, simple, vlb, grad))
    assert call() == 0 and call(grad=None) == 0


# ------------------------------------------------------------------------------------------------------------ 4. whole calls on a tiny UNet
T_CALL = 8
CFG6 = dict(unet_cfgs()["u_a0_tiny"], out_channels=6)
_UNETS = {}


def _unet(prec):
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    if prec not in _UNETS:
        u = UNetModel(**CFG6).set_precision(prec)
        u.load_state_dict(synth_state_dict(unet_param_shapes(**CFG6), 7))
        _UNETS[prec] = u.to(DEV).eval()
    return _UNETS[prec]


def _model(prec="fp32x3", kind="eps", T_=T_CALL, learned=True, net=None):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    return EODiffusion(_unet(prec) if net is None else net, timesteps=T_, image_size=16, in_channels=3, device=DEV, parameterization=kind,
                       learned_variance=learned).to(DEV).eval()


class _MeanNet(torch.nn.Module):
    """the 2 C UNet seen as a C-channel network: its mean half"""

    def __init__(self, unet):
        super().__init__()
        self.unet = unet

    def forward(self, x, t, cond=None, y=None):
        return self.unet(x, t, cond=cond, y=y)[:, :3].contiguous()


@functools.lru_cache(maxsize=None)
def _draws(n=2):
    return synth_input("vx", (n, 3, 16, 16), 91), synth_input("vn", (T_CALL, n, 3, 16, 16), 91)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("kind", ["eps", "v"])
def test_sampling_is_the_model_and_the_two_kernels(kind, clip):
    m = _model(kind=kind)
    x_T, noises = _draws()
    out = m.sampling(2, clipped_reverse_diffusion=clip, device=DEV, x_T=x_T, noises=noises, progress=False)
    L, tb = _lib.lib(), m.variance_tables()
    x = x_T.to(DEV)
    with torch.no_grad():
        for k, i in enumerate(range(T_CALL - 1, -1, -1)):
            t = torch.full((2,), i, dtype=torch.int64, device=DEV)
            o = m.model(x, t).clone()
            p, nxt = torch.empty_like(x), torch.empty_like(x)
            assert L.eod_ddpm_var_pred(x.data_ptr(), o.data_ptr(), t.data_ptr(), m.alphas_cumprod.data_ptr(), m.sqrt_alphas_cumprod.data_ptr(),
                                       m.sqrt_one_minus_alphas_cumprod.data_ptr(), KINDS[kind], int(clip), p.data_ptr(), 2, 768, T_CALL, _stream()) == 0
            assert L.eod_ddpm_step_p0_var(x.data_ptr(), p.data_ptr(), o.data_ptr(), noises[k].to(DEV).data_ptr(), t.data_ptr(), m.betas.data_ptr(),
                                          m.alphas.data_ptr(), m.alphas_cumprod.data_ptr(), tb["sigma_min"].data_ptr(), tb["half_gap"].data_ptr(),
                                          nxt.data_ptr(), 2, 768, T_CALL, _stream()) == 0
            x = nxt
    assert bool(torch.isfinite(out).all()) and torch.equal(out, x)
    # ... and it is not the fixed-variance chain of the mean half
    plain = _model(kind=kind, learned=False, net=_MeanNet(_unet("fp32x3")))
    assert not torch.equal(plain.sampling(2, clipped_reverse_diffusion=clip, device=DEV, x_T=x_T, noises=noises, progress=False), out)


@functools.lru_cache(maxsize=None)
def _oracle():
    from eo_diffusion_amd.backbones.unet_openai import unet_param_shapes
    from oracle import unet_ref as UR
    sd = synth_state_dict(unet_param_shapes(**CFG6), 7)
    return lambda x, t: UR.unet_forward(sd, CFG6, x, t)


@functools.lru_cache(maxsize=None)
def _cpu_reference(kind):
    x_T, noises = _draws()
    return VR.sampled(SCH.eo_cosine_tables(T_CALL), _oracle(), KINDS[kind], x_T, noises, True)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("kind", ["eps", "x0"])
def test_sampling_vs_cpu_loop_over_the_oracle(kind, prec):
    m = _model(prec, kind)
    x_T, noises = _draws()
    out = m.sampling(2, device=DEV, x_T=x_T, noises=noises, progress=False).cpu()
    err = rel_l2(out, _cpu_reference(kind))
    print(f"sampling T = {T_CALL} with learned variance as {kind} [{prec}]: rel-L2 vs the CPU loop {err:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert bool(torch.isfinite(out).all()) and err < TRAJ_TOL[prec]


def _cut(scene, plan):
    s = plan.tile
    return torch.cat([scene[:, :, y0:y0 + s, x0:x0 + s] for y0, x0 in plan.origins()]).contiguous()


def _stitch(tiles, plan):
    s = plan.tile
    out = torch.empty((1, tiles.shape[1], plan.H, plan.W), dtype=tiles.dtype, device=tiles.device)
    for i, (y0, x0) in enumerate(plan.origins()):
        out[0, :, y0:y0 + s, x0:x0 + s] = tiles[i]
    return out


def test_scene_calls():
    """overlap 0 on a scene that the tiles partition: sampling on the tiles, bit for bit (the three samplers); overlap 8 on 24 x 40: the result
    does not depend on tile_batch"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    m = _model()
    plan = TilePlan(32, 48, 16, 0)
    x_T, noises = synth_input("sx", (1, 3, 32, 48), 21), synth_input("sn", (T_CALL, 1, 3, 32, 48), 21)
    per_tile = torch.stack([_cut(noises[k], plan) for k in range(T_CALL)])
    scene = m.sampling_scene((32, 48), True, DEV, x_T=x_T, noises=noises, progress=False)
    tiles = m.sampling(6, True, DEV, x_T=_cut(x_T, plan), noises=per_tile, progress=False)
    assert bool(torch.isfinite(scene).all()) and torch.equal(scene, _stitch(tiles, plan))
    plain = _model(learned=False, net=_MeanNet(_unet("fp32x3")))
    for cls in (DPMSolverSampler, DDIMSampler):
        kw = dict(x_T=x_T, progress=False)
        got, _ = cls(m).sample_scene(4, (32, 48), **kw)
        want, _ = cls(plain).sample_scene(4, (32, 48), **kw)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    x_T2 = synth_input("sx", (1, 3, 24, 40), 22)
    kw = dict(overlap=8, x_T=x_T2, rng="philox", seed=4, progress=False)
    a = m.sampling_scene((24, 40), True, DEV, tile_batch=16, **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(m.sampling_scene((24, 40), True, DEV, tile_batch=2, **kw), a)


@pytest.mark.parametrize("kind", ["eps", "v"])
def test_ddim_and_dpm_solver_use_the_mean_half(kind):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    m, plain = _model(kind=kind), _model(kind=kind, learned=False, net=_MeanNet(_unet("fp32x3")))
    x_T, noises = _draws()
    for eta in (0.0, 1.0):
        kw = dict(eta=eta, x_T=x_T, verbose=False, progress=False, step_noises=noises[:4] if eta else None)
        got, _ = DDIMSampler(m).sample(4, 2, (3, 16, 16), **kw)
        want, _ = DDIMSampler(plain).sample(4, 2, (3, 16, 16), **kw)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    got, gi = DPMSolverSampler(m).sample(4, 2, (3, 16, 16), order=2, x_T=x_T, progress=False)
    want, wi = DPMSolverSampler(plain).sample(4, 2, (3, 16, 16), order=2, x_T=x_T, progress=False)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want) and torch.equal(gi["pred_x0"][-1], wi["pred_x0"][-1])


def test_an_observation_of_weight_one_is_met_by_the_returned_sample():
    m = _model()
    x_T, noises = _draws()
    values = CO.block_mean(synth_input("ov", (2, 3, 16, 16), 5, uniform=True).to(DEV) * 2 - 1, (1, 2, 4))
    out = m.sampling(2, device=DEV, x_T=x_T, noises=noises, progress=False, observation=Observation(values, (1, 2, 4), weight=1.0))
    res = float((CO.block_mean(out, (1, 2, 4)) - values).abs().max())
    print(f"block-mean residual of the returned sample: {res:.2e}")
    # (the bound of tests/test_gpu_ancestral_obs.py: at t = 0 the posterior step returns the projected prediction)
    assert bool(torch.isfinite(out).all()) and res <= 4 * float(np.finfo(np.float32).eps) * max(1.0, float(out.abs().max()))


# ------------------------------------------------------------------------------------------------------------ 5. one training step
GTOL = {"fp32": 2e-4, "fp16": 1e-2}                      # the gates of tests/test_gpu_training.py


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_one_training_step_under_hybrid_loss_vs_autograd_of_the_oracle(prec):
    from eo_diffusion_amd import optim
    from eo_diffusion_amd.backbones import unet_openai as U
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from oracle import unet_ref as UR
    cfg = dict(unet_cfgs()["u_a1_tiny"], out_channels=6)
    sd = synth_state_dict(U.unet_param_shapes(**cfg), 11)
    unet = U.UNetModel(**cfg).set_precision(prec)
    unet.load_state_dict(sd)
    model = EODiffusion(unet, timesteps=1000, image_size=16, in_channels=3, learned_variance=True).to(DEV).train()
    x, noise = synth_input("trx", (4, 3, 16, 16), 3, uniform=True) * 2 - 1, synth_input("trn", (4, 3, 16, 16), 4)
    t = torch.tensor([7, 650, 999, 0])
    lam = 1e-3
    loss_fn = optim.HybridLoss(model, "l2", vlb_weight=lam)
    o, target, x_t, tt = model(x.to(DEV), noise.to(DEV), t=t.to(DEV), return_target=True, return_state=True)
    assert o.shape == (4, 6, 16, 16) and target.shape == (4, 3, 16, 16) and torch.equal(tt.cpu(), t)
    weight = model.loss_weights("min_snr", 5.0)[t.to(DEV)]
    loss = loss_fn(o, target, x.to(DEV), x_t, tt, weight=weight)
    loss.backward()
    torch.cuda.synchronize()
    # the CPU side: the oracle UNet, the loss as a torch float64 expression with the mean detached in the variational-bound term
    tb = {k: getattr(model, k).detach().cpu() for k in ("betas", "alphas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
    vt = VR.tables64(tb)
    ref_xt, _ = PR.q_sample_v(tb, x, noise, t)
    assert bits_equal(x_t.cpu(), ref_xt)
    sdg = {k: p.clone().requires_grad_(True) for k, p in sd.items()}
    ro = UR.unet_forward(sdg, cfg, ref_xt, t)
    mean, v = ro[:, :3], ro[:, 3:].double()
    w = weight.cpu()
    simple = (w * ((mean - noise) ** 2).reshape(4, -1).mean(1)).mean()
    vlb = []
    for n, tn in enumerate(t.tolist()):
        p0 = torch.from_numpy(VR.p0_64(0, ref_xt[n].numpy().astype(np.float64), mean[n].detach().numpy().astype(np.float64),
                                       vt["sqrt_alphas_cumprod"][tn], vt["sqrt_one_minus_alphas_cumprod"][tn]))
        vlb.append(VR.vlb_torch(x[n].double(), p0, v[n], tn == 0, vt["c1"][tn], vt["lmin"][tn], vt["gap"][tn]).mean())
    ref_loss = simple.double() + lam * torch.stack(vlb).mean()
    ref_loss.backward()
    e_loss = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    print(f"training step under HybridLoss [{prec}]: loss {float(loss):.6f} vs {float(ref_loss):.6f} (rel {e_loss:.2e}); "
          f"L_n {loss_fn.per_sample.tolist()}, V_n {loss_fn.per_sample_vlb.tolist()}")
    assert e_loss < GTOL[prec]
    gref = {k: p.grad for k, p in sdg.items() if p.grad is not None}
    gmax = max(float(g.norm()) for g in gref.values())
    worst, n_checked = ("", 0.0), 0
    for name, p in model.model.named_parameters():
        if name not in gref:
            continue
        assert p.grad is not None and p.grad.shape == p.shape, name
        if float(gref[name].norm()) < 1e-5 * gmax:
            assert float(p.grad.norm()) < 1e-3 * gmax, name
            continue
        e = rel_l2(p.grad.cpu(), gref[name])
        n_checked += 1
        if e > worst[1]:
            worst = (name, e)
    print(f"training step under HybridLoss [{prec}]: worst gradient {worst} over {n_checked} tensors (gate {GTOL[prec]:g})")
    assert n_checked > 20 and worst[1] < GTOL[prec], worst
    # without return_state nothing changed
    with torch.no_grad():
        pair = model(x.to(DEV), noise.to(DEV), t=t.to(DEV), return_target=True)
    assert len(pair) == 2 and pair[1].shape == (4, 3, 16, 16)


# ------------------------------------------------------------------------------------------------------------ 6. the default route
class _Net(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x, t, cond=None, y=None):
        return torch.cat([x * 0.25] * self.out, 1).contiguous()


def test_a_model_without_the_switch_calls_no_new_entry_point(monkeypatch):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion
    L = _lib.lib()
    called = collections.Counter()

    def wrap(name, fn):
        def w(*a):
            called[name] += 1
            return fn(*a)
        return w
    for name in list(_lib.SYMBOLS) + list(_lib.PARAM_SYMBOLS) + list(_lib.VAR_SYMBOLS):
        monkeypatch.setattr(L, name, wrap(name, getattr(L, name)))

    def every_call(m):
        outs = [m.sampling(2, True, device=DEV, progress=False), m.sampling(2, False, device=DEV, progress=False),
                m.sampling_scene((16, 24), True, DEV, overlap=4, progress=False),
                DDIMSampler(m).sample(3, 2, (3, 8, 8), eta=0.5, verbose=False, progress=False)[0],
                DPMSolverSampler(m).sample(4, 2, (3, 8, 8), order=2, progress=False)[0]]
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(o).all()) for o in outs)
    every_call(EODiffusion(_Net(1), timesteps=6, image_size=8, in_channels=3).to(DEV))
    assert not any(called[k] for k in _lib.VAR_SYMBOLS) and called["eod_ddpm_step"] == 18
    called.clear()
    every_call(EODiffusion(_Net(2), timesteps=6, image_size=8, in_channels=3, learned_variance=True).to(DEV))
    print("calls of a learned-variance model:", {k: v for k, v in sorted(called.items()) if v})
    assert called["eod_ddpm_var_pred"] == called["eod_ddpm_step_p0_var"] == 18
    assert not any(called[k] for k in ("eod_ddpm_step", "eod_ddpm_pred_x0", "eod_ddpm_step_p0", "eod_ddpm_param_pred"))
