"""CPU: the numpy restatements of tests/sampler_edge_ref.py against oracle/sampler_ref.py, tests/dpm_ref.py, tests/ancestral_ref.py,
oracle/harness_ref.py, tests/repaint_ref.py and float64 on small inputs; the float64 Box-Muller against oracle.philox_ref.philox_randn;
and NaN propagation exactly where torch.clamp puts it.  No GPU, no libeodiff.so."""
import numpy as np
import pytest
import torch

from eo_diffusion_amd.diffusion.util import dpm_coefficients
from oracle import harness_ref as HR
from oracle import philox_ref as PR
from oracle import sampler_ref as SR
from oracle import schedule as SCH
from tests import ancestral_ref as AR
from tests import dpm_ref as DR
from tests import repaint_ref as RR
from tests import sampler_edge_ref as R

T = 1000
NAN, INF = float("nan"), float("inf")


def _same(a, b):
    """bit equality, NaN matching NaN"""
    a = np.ascontiguousarray(a.numpy() if isinstance(a, torch.Tensor) else a).reshape(-1)
    b = np.ascontiguousarray(b.numpy() if isinstance(b, torch.Tensor) else b).reshape(-1)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn])


def _xez(n, chw, seed, scale=1.5):
    g = np.random.default_rng(seed)
    return tuple((g.standard_normal((n, chw)) * scale).astype(np.float32) for _ in range(3))


def _t4(a):
    return torch.from_numpy(np.ascontiguousarray(a))[:, None, None, :]


@pytest.fixture(scope="module")
def tb():
    t = SCH.eo_cosine_tables(T)
    return t, R.tables(t)


TS = [[0, 0, 0], [5, 0, 7], [0, 5, 7], [1, 1, 1], [T - 1, 1, T - 1], [999, 500, 2]]


@pytest.mark.parametrize("tl", TS, ids=str)
def test_step_restatements_have_the_oracles_bits(tl, tb):
    tt, tn = tb
    x, e, z = _xez(3, 37, sum(tl))
    x[0, 0], e[1, 1], z[2, 2], x[1, 5], e[2, 6], z[0, 7], x[2, 9] = NAN, NAN, NAN, INF, -INF, INF, -INF
    t = torch.tensor(tl)
    assert _same(R.q_sample(tn, x, z, tl), SR.q_sample(tt, _t4(x), t, _t4(z)))
    assert _same(R.ddpm_step(tn, x, e, z, tl, 1), SR.ddpm_step_clip(tt, _t4(x), t, _t4(z), _t4(e)))
    assert _same(R.ddpm_step(tn, x, e, z, tl, 0), SR.ddpm_step_noclip(tt, _t4(x), t, _t4(z), _t4(e)))
    assert _same(R.ddpm_step(tn, x, e, z, tl, 1), AR.step(tt, _t4(x), _t4(e), _t4(z), t)[0])
    C, hw = 3, 5
    g = np.random.default_rng(1)
    mask = np.asarray([0.0, 1.0, 0.25, -0.5, 1.5], np.float32)[g.integers(0, 5, (3, hw))]
    xs, es, zs = x[:, :C * hw], e[:, :C * hw], z[:, :C * hw]
    want = SR.repaint_mix(tt, torch.from_numpy(xs).reshape(3, C, 1, hw), torch.from_numpy(es).reshape(3, C, 1, hw),
                          torch.from_numpy(mask).reshape(3, 1, 1, hw), t, torch.from_numpy(zs).reshape(3, C, 1, hw))
    assert _same(R.repaint_mix(tn, xs, es, mask, zs, tl, C), want)


@pytest.mark.parametrize("bad_t", [-1, T, T + 5, 2 ** 40, -2 ** 40])
def test_a_timestep_out_of_range_poisons_its_sample_and_keeps_the_batch_minimum_as_given(bad_t, tb):
    tt, tn = tb
    x, e, z = _xez(3, 21, 4)
    for pos in range(3):
        tl = [5, 900, 17]
        tl[pos] = bad_t
        keep = [i for i in range(3) if i != pos]
        tk = [tl[i] for i in keep]
        for clip in (0, 1):
            got = R.ddpm_step(tn, x, e, z, tl, clip)
            assert np.isnan(got[pos]).all() and np.isfinite(got[keep]).all()
            # the others: the step of the two alone, in the branch the minimum AS GIVEN selects (a negative member: the t == 0 branch)
            if bad_t > 0:
                assert _same(got[keep], R.ddpm_step(tn, x[keep], e[keep], z[keep], tk, clip))
                fn = SR.ddpm_step_clip if clip else SR.ddpm_step_noclip
                assert _same(got[keep], fn(tt, _t4(x[keep]), torch.tensor(tk), _t4(z[keep]), _t4(e[keep])))
            else:
                zero = R.ddpm_step(tn, np.concatenate([x[keep], x[:1]]), np.concatenate([e[keep], e[:1]]), np.concatenate([z[keep], z[:1]]), tk + [0], clip)
                assert _same(got[keep], zero[:2])
        q = R.q_sample(tn, x, z, tl)
        assert np.isnan(q[pos]).all() and _same(q[keep], SR.q_sample(tt, _t4(x[keep]), torch.tensor(tk), _t4(z[keep])))
        assert _same(R.ddpm_step(tn, x, e, z, tl, 1), AR.step(tt, _t4(x), _t4(e), _t4(z), torch.tensor(tl))[0])


def test_the_clamp_propagates_nan_exactly_where_torch_clamp_does():
    v = np.array([NAN, -NAN, INF, -INF, 0.5, -0.0, 1.0, -1.0, 3.0, -3.0, 1e-40], np.float32)
    got = R.clamp_pm1(v)
    assert _same(got, torch.clamp(torch.from_numpy(v), -1.0, 1.0))
    assert np.isnan(got[:2]).all() and not np.isnan(got[2:]).any() and got[2] == 1.0 and got[3] == -1.0 and np.signbit(got[5])
    eat = np.fmin(np.fmax(v, np.float32(-1.0)), np.float32(1.0))            # fminf(fmaxf(v, -1), 1): what the kernels did before
    assert eat[0] == -1.0 and _same(eat[2:], got[2:])


def test_chain_halves_compose_to_the_whole_steps():
    x, e, d = (v.reshape(-1) for v in _xez(1, 101, 7))
    x[3], e[4], d[5] = NAN, INF, -INF
    a_s, a_t = np.float32(0.37), np.float32(0.61)
    s1m = float(np.sqrt(np.float32(1.0) - a_s))
    for second in (False, True):
        c = dpm_coefficients(a_s, a_t, 0.4 if second else None, 2 if second else 1)
        for clip in (False, True):
            wx, wp = DR.step(torch.from_numpy(x), torch.from_numpy(e), torch.from_numpy(d) if second else None, float(a_s), s1m, *c, clip)
            assert _same(R.dpmpp_step_p0(x, wp.numpy(), d if second else None, *c), wx)
    for noisy in (True, False):
        sg = 0.21 if noisy else 0.0
        wx, wp = SR.ddim_step(_t4(x[None]), _t4(e[None]), float(a_s), float(a_t), sg, s1m, _t4(d[None]) if noisy else torch.zeros(1, 1, 1, 101), 0.9)
        assert _same(R.ddim_step_p0(e, wp.numpy().reshape(-1), d if noisy else None, float(a_t), sg, 0.9), wx)
    assert _same(R.renoise(x, d, 0.61, 0.37), RR.renoise(torch.from_numpy(x), torch.from_numpy(d), 0.61, 0.37))


def test_flat_and_harness_restatements():
    x, e, _ = _xez(2, 3 * 35, 9)
    x[0, 0], x[0, 1], x[1, 2], x[1, 3] = NAN, INF, -INF, -0.0
    xt, et = torch.from_numpy(x), torch.from_numpy(e)
    for s in (3.5, 0.0, -1.25):
        assert _same(R.cfg_combine(x, e, s), xt + s * (et - xt))
    assert _same(R.postprocess(x, 0), xt.clip(0, 1)) and _same(R.postprocess(x, 1), (xt + 1.0) / 2.0)
    mask = np.asarray([0.0, 1.0, 0.25, -0.5, 1.5, NAN], np.float32)[np.random.default_rng(2).integers(0, 6, (2, 35))]
    img, m4 = xt.reshape(2, 3, 5, 7), torch.from_numpy(mask).reshape(2, 1, 5, 7)
    assert _same(R.masked_preview(x, mask, 3, 0.7), HR.masked_preview(img, m4))
    assert _same(R.masked_preview(x, mask, 3, 0.0), img * m4.clip(0, 1))
    assert np.isnan(mask).any() and np.array_equal(np.isnan(R.masked_preview(e, mask, 3, 0.7)), np.tile(np.isnan(mask), (1, 3)))
    for inv in (0, 1):
        assert _same(R.repaint_cond(x, mask, 3, inv), HR.repaint_cond(img, m4, invert=bool(inv)))


def test_ldm_parts_follow_the_oracle_and_t0_is_exact():
    lt = SCH.ldm_register_schedule(SCH.ldm_beta_schedule("linear", T))
    ln = R.tables(lt)
    x, e, z = _xez(3, 30, 11)
    for tl in ([999, 500, 1], [0, 0, 7], [3, 0, 250]):
        for clip in (True, False):
            mean, sd64, bad = R.ldm_p_sample_parts(ln, x, e, tl, clip)
            want = SR.ldm_p_sample(lt, _t4(x), torch.tensor(tl), _t4(e), _t4(z), clip_denoised=clip).numpy().reshape(3, -1)
            got = mean.astype(np.float64) + sd64 * z
            assert not bad.any() and np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max())
            for n, t in enumerate(tl):
                if t == 0:
                    assert sd64[n, 0] == 0.0 and _same(mean[n] + np.float32(0.0) * z[n], want[n])
    mean, sd64, bad = R.ldm_p_sample_parts(ln, x, e, [T, 3, -1], True)
    assert bad.tolist() == [True, False, True] and sd64[0, 0] == 0.0 and sd64[1, 0] > 0.0


def test_timestep_embedding64_follows_the_reference_formula():
    import math
    for dim in (1, 2, 3, 64, 513):
        half = dim // 2
        t = np.array([0.0, 999.0, 1.0, 500.5, 0.123, 37.0], np.float32)
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).numpy() if half else np.zeros(0, np.float32)
        got = R.timestep_embedding64(t, freqs, dim)
        assert got.shape == (6, dim)
        if half:
            args = torch.from_numpy(t)[:, None].float() * torch.from_numpy(freqs)[None]       # unet_openai.py:95
            want = torch.cat([torch.cos(args), torch.sin(args)], dim=-1).numpy()
            assert np.abs(got[:, :2 * half] - want).max() <= 3e-7
            exact = np.cos(args.numpy().astype(np.float64))
            assert np.array_equal(got[:, :half], exact)
            assert (got[0, :half] == 1.0).all() and (got[0, half:2 * half] == 0.0).all()
        if dim % 2:
            assert (got[:, -1] == 0.0).all()


KEYS = [dict(seed=1234, sample0=0, step=7, stream_id=1), dict(seed=(0x1234 << 32) | 0x9abcdef1, sample0=2 ** 32 - 1, step=2 ** 31 - 1, stream_id=2),
        dict(seed=(1 << 63) | 5, sample0=2 ** 20, step=0, stream_id=0)]


@pytest.mark.parametrize("key", KEYS, ids=lambda k: hex(k["seed"]))
def test_float64_box_muller_against_philox_randn(key):
    """the fp32 numpy Box-Muller of oracle/philox_ref.py lies within the GPU test's own bound of the float64 one (numpy's float32 log,
    sqrt, cos and sin are within an ulp), for chw % 4 = 0 .. 3; and the uniforms are multiples of 2^-25 in (0, 1]"""
    for chw in (1028, 1029, 1030, 1031, 3):
        ur, ua = R.philox_uniforms(2, chw, **key)
        z, r, a = R.box_muller64(ur, ua, chw)
        ref = PR.philox_randn(2, chw, key["seed"], key["sample0"], key["step"], key["stream_id"])
        assert z.shape == ref.shape == (2, chw)
        assert (np.abs(z - ref) <= r * (a + 2.5) * 2.0 ** -23).all()
        for u in (ur, ua):
            k = u.astype(np.float64) * 2.0 ** 25
            assert (k == np.round(k)).all() and u.min() > 0 and u.max() <= 1   # (above 1/2 the + 0.5f rounds to even: a multiple of 2^-24)
    assert not np.array_equal(R.philox_uniforms(1, 8, **key)[0], R.philox_uniforms(1, 8, **dict(key, seed=key["seed"] ^ (1 << 32)))[0])
