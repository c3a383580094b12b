"""CPU: the references of tests/train_objective_ref.py against torch float64 autograd of the same objective written independently with
F.mse_loss / F.l1_loss / F.huber_loss(reduction="none"), and EODiffusion.loss_weights against its formulas.

Gates.  The loss agrees to 1e-12 relative (both sides are float64 sums of the same float64 terms).  The float32 gradient is held to
1 float32 ulp of the float64 autograd gradient rounded to float32 on inputs whose intermediate values are exact in float32 -- pred and
target on a dyadic grid (the difference is exact), N * S_n and the weights powers of two (s_n is exact), 0/1 masks (s_n * m is exact) -- so
that the documented operation order (s_n rounded, s_n * m rounded, d rounded, the product rounded) leaves ONE rounding, and one rounding
is within 1 ulp of the rounded exact value.  On general inputs each of the four roundings moves the result by up to 2^-24 relative, i.e.
up to one unit in the last place of a result whose significand is near 1, so the same comparison is held to 4 ulp there (three inherited
roundings of up to 1 ulp each, the last rounding and the rounding of the exact value half an ulp each); the worst observed distance is
printed."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_objective_ref as R

f32, f64 = np.float32, np.float64


def _autograd(pred, target, mask, weight, kind, delta):
    """float64 torch: elementwise loss, times the broadcast mask, per-sample sum over the sum of the mask (0 where that is 0), times the
    weight, batch mean; returns (loss, per_sample, dLoss/dpred)"""
    p = torch.tensor(np.asarray(pred, f64), requires_grad=True)
    t = torch.tensor(np.asarray(target, f64))
    N = p.shape[0]
    if kind == "l2":
        el = F.mse_loss(p, t, reduction="none")
    elif kind == "l1":
        el = F.l1_loss(p, t, reduction="none")
    else:
        el = F.huber_loss(p, t, reduction="none", delta=float(f32(delta)))
    m = torch.ones_like(p) if mask is None else torch.tensor(np.asarray(mask, f64)).expand_as(p)
    S = m.flatten(1).sum(1)
    num = (el * m).flatten(1).sum(1)
    per = torch.where(S > 0, num / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S))
    w = torch.ones(N, dtype=torch.float64) if weight is None else torch.tensor(np.asarray(weight, f64))
    loss = (w * per).sum() / N
    loss.backward()
    return float(loss.detach()), per.detach().numpy(), p.grad.numpy()


def _ulps(a, b):
    """distance of float32 arrays in units of the last place (across zero: through the signed integer line)"""
    def line(x):
        i = np.ascontiguousarray(x, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(line(a) - line(b))


def _masks(rng, N, C, H, W, which, soft):
    if which is None:
        return None
    shape = {"n1": (N, 1, H, W), "nc": (N, C, H, W), "11": (1, 1, H, W)}[which]
    m = (rng.random(shape) < 0.6).astype(f32)
    if soft:
        m = m * (rng.integers(1, 257, shape) / 256.0).astype(f32)
    return m


def _exact_case(rng, N, C, H, W, which):
    """inputs on which the float32 gradient has one rounding: dyadic pred / target (|values| < 8, step 2^-10), a 0/1 mask whose per-sample
    sum times N * C is a power of two, weights that are powers of two"""
    pred = (rng.integers(-4096, 4096, (N, C, H, W)) / 1024.0).astype(f32)
    target = (rng.integers(-4096, 4096, (N, C, H, W)) / 1024.0).astype(f32)
    mask = None
    if which is not None:
        shape = {"n1": (N, 1, H, W), "nc": (N, C, H, W), "11": (1, 1, H, W)}[which]
        mask = np.zeros(shape, f32)
        flat = mask.reshape(shape[0], -1)
        for n in range(shape[0]):
            count = 2 ** int(rng.integers(0, int(math.log2(flat.shape[1])) + 1))
            flat[n, rng.permutation(flat.shape[1])[:count]] = 1.0
    weight = (2.0 ** rng.integers(-3, 3, N)).astype(f32)
    return pred, target, mask, weight


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("which", [None, "n1", "nc", "11"])
def test_loss_ref_matches_float64_autograd_where_one_rounding_is_left(kind, which):
    rng = np.random.default_rng(7)
    N, C, H, W = 4, 4, 8, 8   # N * C * (a power of two) is a power of two
    for use_weight in (False, True):
        pred, target, mask, weight = _exact_case(rng, N, C, H, W, which)
        if mask is not None and mask.shape[0] == N:
            mask[2] = 0.0                                            # a fully clouded sample
        live = np.nonzero((np.broadcast_to(mask, pred.shape)[0] if mask is not None else np.ones(pred.shape[1:])).reshape(-1) != 0)[0]
        assert live.size >= 1
        spots = [int(live[k % live.size]) for k in range(3)]         # live elements of sample 0
        P0, T0 = pred[0].reshape(-1), target[0].reshape(-1)           # (views)
        if kind == "l1":                                             # d = +0, d = -0 + 0, d = 0 - 0: the slope is 0, not +-1
            P0[spots[0]] = T0[spots[0]]
            P0[spots[1]], T0[spots[1]] = -0.0, 0.0
            P0[spots[2]], T0[spots[2]] = 0.0, -0.0
        if kind == "huber":                                          # |d| exactly delta, from both sides
            P0[spots[0]], T0[spots[0]] = 2.5, 1.0
            P0[spots[1]], T0[spots[1]] = -0.5, 1.0
        delta = 1.5
        w = weight if use_weight else None
        ref = R.loss_ref(pred, target, mask, w, kind, delta)
        loss, per, grad = _autograd(pred, target, mask, w, kind, delta)
        assert abs(ref["loss64"] - loss) <= 1e-12 * abs(loss), (ref["loss64"], loss)
        assert np.all(np.abs(ref["per64"] - per) <= 1e-12 * np.abs(per)), (ref["per64"], per)
        if mask is not None and mask.shape[0] == N:
            assert ref["per64"][2] == 0.0 and not ref["dpred"][2].any() and not np.signbit(ref["dpred"][2]).any()
        u = _ulps(ref["dpred"], grad.astype(f32))
        assert u.max() <= 1, (kind, which, use_weight, int(u.max()))
        if kind == "l1":
            z = ref["dpred"][0].reshape(-1)[spots]
            assert not z.any() and not np.signbit(z).any()
        if mask is not None:
            dead = np.broadcast_to(mask, pred.shape) == 0
            assert not ref["dpred"][dead].any() and not np.signbit(ref["dpred"][dead]).any()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("which,soft", [(None, False), ("n1", False), ("nc", True), ("11", True)])
def test_loss_ref_matches_float64_autograd_on_general_inputs(kind, which, soft):
    rng = np.random.default_rng(11)
    N, C, H, W = 3, 5, 7, 9
    worst = 0
    for use_weight in (False, True):
        pred = rng.standard_normal((N, C, H, W)).astype(f32)
        target = rng.standard_normal((N, C, H, W)).astype(f32)
        mask = _masks(rng, N, C, H, W, which, soft)
        w = (0.1 + rng.random(N)).astype(f32) if use_weight else None
        ref = R.loss_ref(pred, target, mask, w, kind, 0.7)
        loss, per, grad = _autograd(pred, target, mask, w, kind, 0.7)
        assert abs(ref["loss64"] - loss) <= 1e-12 * abs(loss), (ref["loss64"], loss)
        assert np.all(np.abs(ref["per64"] - per) <= 1e-12 * np.abs(per))
        worst = max(worst, int(_ulps(ref["dpred"], grad.astype(f32)).max()))
    print(f"loss_ref dpred vs float64 autograd, {kind} mask={which} soft={soft}: worst {worst} ulp (bound 4)")
    assert worst <= 4


def test_loss_ref_skips_masked_nan_and_inf():
    rng = np.random.default_rng(13)
    N, C, H, W = 2, 3, 4, 5
    pred, target = rng.standard_normal((N, C, H, W)).astype(f32), rng.standard_normal((N, C, H, W)).astype(f32)
    mask = (rng.random((N, 1, H, W)) < 0.5).astype(f32)
    dead = np.broadcast_to(mask, pred.shape) == 0
    clean = R.loss_ref(np.where(dead, f32(0), pred), np.where(dead, f32(0), target), mask, None, "huber", 1.0)
    pred[dead] = np.nan
    target[dead] = np.inf
    dirty = R.loss_ref(pred, target, mask, None, "huber", 1.0)
    assert dirty["loss"] == clean["loss"] and np.array_equal(dirty["per_sample"], clean["per_sample"])
    assert np.array_equal(dirty["dpred"].view(np.uint32), clean["dpred"].view(np.uint32))


def test_grad_norm_and_clip_refs():
    g = np.array([3.0, -4.0, 0.0, -0.0], f32)
    assert R.grad_sumsq_ref(g) == 25.0 and R.grad_norm_ref(g[:2], g[2:]) == 5.0
    assert R.clip_coef_ref(5.0, math.inf) == 1.0 and R.clip_coef_ref(5.0, 10.0) == 1.0
    assert R.clip_coef_ref(5.0, 2.5) == f32(2.5 / (5.0 + 1e-6))
    assert math.isinf(R.grad_sumsq_ref(np.array([1.0, np.inf], f32))) and math.isnan(R.grad_sumsq_ref(np.array([np.nan, 1.0], f32)))
    p, m, v = np.ones(4, f32), np.zeros(4, f32), np.zeros(4, f32)
    a = R.adamw_clipped_ref(p, g, m, v, f32(0.5), 0.99, 0.9, 0.999, 1e-8, 0.03, -0.01)
    b = R.adamw_step_scalars(p, g * f32(0.5), m, v, 0.99, 0.9, 0.999, 1e-8, 0.03, -0.01)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(a[1], (f32(1.0 - 0.9) * (g * f32(0.5))).astype(f32))


@pytest.mark.parametrize("T", [250, 1000])
def test_loss_weights_follow_their_formulas(T):
    """the [T] tables against Python-float arithmetic on the same fp32 alphas_cumprod.  torch's float64 division and pow may differ from
    Python's by an ulp of float64, which moves the float32 rounding by at most one unit: held to 1 ulp, equality counted"""
    from eo_diffusion_amd import _lib
    from eo_diffusion_amd.diffusion.model import EODiffusion
    d = EODiffusion(None, image_size=16, in_channels=3, timesteps=T)
    acp = d.alphas_cumprod.numpy()
    for kind, gamma, k in (("min_snr", 5.0, 1.0), ("min_snr", 1.0, 1.0), ("p2", 0.0, 1.0), ("p2", 1.0, 1.0), ("p2", 0.5, 2.0), ("uniform", 0.0, 1.0)):
        w = d.loss_weights(kind, gamma, k)
        assert w.dtype == torch.float32 and tuple(w.shape) == (T,) and w.device == d.alphas_cumprod.device
        w = w.numpy()
        ref = R.loss_weights_ref(acp, kind, gamma, k)
        assert np.isfinite(w).all() and not np.isnan(w[[0, T - 1]]).any(), (kind, gamma)
        u = _ulps(w, ref)
        print(f"loss_weights T={T} {kind} gamma={gamma} k={k}: {int((u == 0).sum())} of {T} equal, worst {int(u.max())} ulp")
        assert u.max() <= 1, (kind, gamma, k, int(u.max()))
        if kind == "min_snr":
            assert (w > 0).all() and (w <= 1).all()
        if kind == "uniform" or (kind == "p2" and gamma == 0.0):
            assert (w == 1).all()
    zero = torch.tensor([0.5, 0.0, 1.0])   # a schedule that reaches both ends
    from eo_diffusion_amd.diffusion.model import loss_weight_table
    assert loss_weight_table(zero, "min_snr", 5.0).tolist() == [1.0, 1.0, 0.0]
    assert torch.isfinite(loss_weight_table(zero, "p2", 1.0)).all() and loss_weight_table(zero, "p2", 1.0)[2] == 0.0
    for bad in (("snr", 1.0), ("min_snr", 0.0)):
        with pytest.raises(_lib.EodError):
            d.loss_weights(*bad)


def test_diffusion_loss_refuses_on_the_host():
    """everything optim.diffusion_loss refuses is refused before the library is touched (CPU tensors are one of the refusals)"""
    from eo_diffusion_amd import _lib, optim
    x = torch.zeros(2, 3, 4, 4)
    for kw in (dict(kind="l3"), dict(delta=0.0), dict(delta=-1.0), dict()):
        with pytest.raises(_lib.EodError):
            optim.diffusion_loss(x, x, **kw)
    with pytest.raises(_lib.EodError):
        optim.DiffusionLoss("mse")
    with pytest.raises(_lib.EodError):
        optim.DiffusionLoss("huber", delta=0)
