"""GPU: observations on the ancestral samplers -- eod_ddpm_pred_x0, eod_ddpm_step_p0 (csrc/sampler.hip, csrc/ddpm_p0_body.h) and
`observation=` on EODiffusion.sampling / sampling_scene and dist.sharded_sampling*.  DESIGN.md section 9.8.

The two kernels are held bit for bit (torch.equal) to the torch fp32 emulation of tests/ancestral_ref.py and, with the clamp, their
composition to eod_ddpm_step(clip = 1); bad arguments to -1 with the outputs untouched; whole calls with injected draws to CPU loops of the
oracle UNet and the emulated steps under the gates of tests/test_gpu_repaint_resample.py; observation=None to the launches of the version
before; weight 0 to the call without an observation; weight 1 to the observation's block means in the RETURNED sample; scenes to sampling()
on the tiles, to the emulation on the recorded inputs of the scene-level step, members of a stack and shards of a batch to the calls on
their own; every refusal to a forward hook that sees no call."""
import functools

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, SpectralObservation
from eo_diffusion_amd.tiling import TilePlan
from oracle import schedule as SCH
from tests import ancestral_ref as AR
from tests import consistency_ref as CR
from tests import psf_ref as PR
from tests import repaint_ref as RR
from tests import spectral_ref as XR
from tests.gpu_util import DEV
from tests.helpers import rel_l2
from tests.synth import rect_mask, synth_input
from tests.test_gpu_repaint_resample import TRAJ_TOL, _nan, _offset_by_4_bytes, _tiny
from tests.test_gpu_sampling import _model
from tests.test_gpu_scene import _diffusion, cut, stitch
from tests.test_gpu_scene_skip import Calls

pytestmark = pytest.mark.gpu

EPS = AR.EPS
SHAPES = [(3, 6, 7), (3, 16, 16), (13, 12, 12)]          # chw = 126 (no multiple of 4), 768, 1872


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _tables(T):
    tb = SCH.eo_cosine_tables(T)
    return tb, {k: v.to(DEV).contiguous() for k, v in tb.items()}


def pred_x0_(T, x, e, t, clip, out, N=None, chw=None, acp=None, T_arg=None):
    """eod_ddpm_pred_x0 itself; returns (rc, out)"""
    d = _tables(T)[1]
    like = next(v for v in (x, e, out) if v is not None)
    n = like.shape[0] if N is None else N
    rc = _lib.lib().eod_ddpm_pred_x0(_lib.ptr(x), _lib.ptr(e), _lib.ptr(t), d["alphas_cumprod"].data_ptr() if acp is None else acp, _lib.ptr(out), n,
                                     (like.numel() // like.shape[0]) if chw is None else chw, T if T_arg is None else T_arg, int(clip), _stream())
    return rc, out


def step_p0_(T, x, p, z, t, out, N=None, chw=None, tabs=None, T_arg=None):
    """eod_ddpm_step_p0 itself; returns (rc, out)"""
    d = _tables(T)[1]
    b, a, c = (d["betas"].data_ptr(), d["alphas"].data_ptr(), d["alphas_cumprod"].data_ptr()) if tabs is None else tabs
    like = next(v for v in (x, p, z, out) if v is not None)
    n = like.shape[0] if N is None else N
    rc = _lib.lib().eod_ddpm_step_p0(_lib.ptr(x), _lib.ptr(p), _lib.ptr(z), _lib.ptr(t), b, a, c, _lib.ptr(out), n,
                                     (like.numel() // like.shape[0]) if chw is None else chw, T if T_arg is None else T_arg, _stream())
    return rc, out


def ddpm_step_(T, x, e, z, t, clip):
    d = _tables(T)[1]
    out = torch.empty_like(x)
    n = x.shape[0]
    rc = _lib.lib().eod_ddpm_step(x.data_ptr(), e.data_ptr(), z.data_ptr(), t.data_ptr(), d["betas"].data_ptr(), d["alphas"].data_ptr(),
                                  d["alphas_cumprod"].data_ptr(), d["sqrt_one_minus_alphas_cumprod"].data_ptr(), out.data_ptr(), n, x.numel() // n, T,
                                  int(clip), _stream())
    assert rc == 0
    return out


def same(a, b):
    """torch.equal with NaN equal to NaN"""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _t_cases(N, T):
    if N == 1:
        return [[5], [0], [T - 1], [T + 2], [-1]]
    return [[5] * 3, [0] * 3, [T - 1] * 3, [0, 3, 7], [5, T + 2, 3], [5, -1, 3]]


def _kernel_inputs(N, shape, seed, scale=2.0):
    return {k: (synth_input("k" + k, (N,) + shape, seed) * scale).to(DEV) for k in ("x", "e", "z")}


def _check_kernels(T, d, off=()):
    """every timestep case on the tensors of d (name in `off`: that pointer 4 bytes behind a 16-byte boundary)"""
    tb = _tables(T)[0]
    N = d["x"].shape[0]
    x, e, z = (d[k].cpu() for k in ("x", "e", "z"))
    g = {k: (_offset_by_4_bytes(v) if k in off else v) for k, v in d.items()}
    for tc in _t_cases(N, T):
        t = torch.tensor(tc, dtype=torch.int64)
        td = t.to(DEV)
        in_range = [n for n, v in enumerate(tc) if 0 <= v < T]
        for clip in (1, 0):
            p_out = _offset_by_4_bytes(_nan(*x.shape)) if "p" in off else _nan(*x.shape)
            rc, p = pred_x0_(T, g["x"], g["e"], td, clip, p_out)
            want_p = AR.pred_x0(tb, x, e, t, bool(clip))
            assert rc == 0 and same(p, want_p), (tc, clip)
            out = _offset_by_4_bytes(_nan(*x.shape)) if "out" in off else _nan(*x.shape)
            rc, got = step_p0_(T, g["x"], p, g["z"], td, out)
            assert rc == 0 and same(got, AR.finish(tb, x, want_p, z, t)), (tc, clip)
            assert bool(torch.isfinite(got[in_range]).all()) and bool(torch.isnan(got).reshape(N, -1).all(1).sum() == N - len(in_range))
            if clip and (len(in_range) == N or min(tc) < 0):          # (the composition: the bits of the unsplit kernel)
                assert same(got, ddpm_step_(T, d["x"], d["e"], d["z"], td, 1)), tc


# ------------------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("T", [8, 1000])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_are_bit_exact(shape, N, T, unaligned):
    """t all 5, all 0, all T - 1, mixed [0, 3, 7] (batch minimum 0), one member out of range (its rows NaN, the others exact); clip on and
    off; every pointer aligned, or every pointer 4 bytes off"""
    _check_kernels(T, _kernel_inputs(N, shape, 31), ("x", "e", "z", "p", "out") if unaligned else ())


@pytest.mark.parametrize("one", ["x", "e", "z", "p", "out"])
def test_one_unaligned_pointer_takes_the_scalar_form_with_the_same_bits(one):
    _check_kernels(8, _kernel_inputs(3, (3, 16, 16), 32), (one,))


def test_a_sample_wider_than_the_grid_is_walked_by_the_stride_loop():
    """chw = 3 * 1024 * 1024: 786432 quads per sample, more than the 2048 x 256 threads of a sample's row of the grid"""
    T = 8
    tb = _tables(T)[0]
    d = {k: synth_input("w" + k, (2, 3, 1024, 1024), 33).to(DEV) for k in ("x", "e", "z")}
    t = torch.tensor([5, 2])
    rc, p = pred_x0_(T, d["x"], d["e"], t.to(DEV), 1, _nan(2, 3, 1024, 1024))
    rc2, got = step_p0_(T, d["x"], p, d["z"], t.to(DEV), _nan(2, 3, 1024, 1024))
    assert (rc, rc2) == (0, 0) and torch.equal(got, ddpm_step_(T, d["x"], d["e"], d["z"], t.to(DEV), 1))
    assert torch.equal(p.cpu(), AR.pred_x0(tb, d["x"].cpu(), d["e"].cpu(), t))


def test_bad_arguments_return_the_error_and_leave_the_outputs_alone():
    T, N, shape = 8, 2, (3, 8, 8)
    d = _kernel_inputs(N, shape, 34)
    x, e, z = d["x"], d["e"], d["z"]
    n = x.numel()
    t = torch.tensor([5, 3], device=DEV)
    out, buf = _nan(N, *shape), _nan(2 * n)
    dt = _tables(T)[1]
    tabs = (dt["betas"].data_ptr(), dt["alphas"].data_ptr(), dt["alphas_cumprod"].data_ptr())
    p = x.clone()
    calls = []
    pr = lambda **kw: calls.append(pred_x0_(T, **{**dict(x=x, e=e, t=t, clip=1, out=out), **kw})[0])
    st = lambda **kw: calls.append(step_p0_(T, **{**dict(x=x, p=p, z=z, t=t, out=out), **kw})[0])
    pr(x=None), pr(e=None), pr(t=None), pr(out=None), pr(acp=0)
    st(x=None), st(p=None), st(z=None), st(t=None), st(out=None), st(tabs=(0,) + tabs[1:]), st(tabs=(tabs[0], 0, tabs[2])), st(tabs=tabs[:2] + (0,))
    for run in (pr, st):
        run(N=0), run(N=-1), run(chw=0), run(chw=-4), run(T_arg=0), run(T_arg=-8)
    # an output on top of an input: the same tensor, a partial overlap in one buffer, t, a table
    pr(out=x), pr(out=e), pr(x=buf[:n].view(N, *shape), out=buf[n - 4:2 * n - 4].view(N, *shape))
    st(out=x), st(out=p), st(out=z), st(z=buf[:n].view(N, *shape), out=buf[n // 2:n // 2 + n].view(N, *shape))
    t_in_buf = buf[:4].view(torch.int64)
    pr(t=t_in_buf, out=buf[:n].view(N, *shape)), st(t=t_in_buf, out=buf[:n].view(N, *shape))
    tab = _nan(64)
    pr(acp=tab.data_ptr(), out=tab[: N * 3 * 2 * 2].view(N, 3, 2, 2), x=x[:, :, :2, :2].contiguous(), e=e[:, :, :2, :2].contiguous())
    torch.cuda.synchronize()
    assert calls and all(rc == -1 for rc in calls), calls
    for v in (out, buf, tab):
        assert bool(torch.isnan(v).all())
    for v in (x, e, z, p):
        assert bool(torch.isfinite(v).all())
    with pytest.raises(EodError):
        _lib.check(pred_x0_(T, None, e, t, 1, out)[0], "eod_ddpm_pred_x0")


# ------------------------------------------------------------------------------------------------------------ 2. whole calls
T_CALL, RESAMPLE = 20, (4, 3)
FORMS = ("block", "spec", "chain", "psf")
VARIANTS = {"plain": dict(), "mix": dict(masked=True), "resample": dict(masked=True, resample=RESAMPLE)}
PAN = np.array([[0.3, 0.5, 0.2]], np.float32)
H7 = PR.gaussian(2, 0.3, radius=3)                                   # f = 2, 7 taps


def _n_eval(resample):
    return len(RR.walk_of(T_CALL, resample)[0])


def _links(form, shape, n_eval, seed, weight=None):
    """the observations of a call on a state of `shape` = (B, 3, H, W) as plain data, one weight per evaluation and link (weight: that
    constant instead).  "block": factors (1, 2, 4) under a soft mask; "spec": a pan band at f = 2; "chain": [a pan band at f = 1, the three
    bands at f = 4]; "psf": the three bands through 7 taps at f = 2."""
    B, C, H, W = shape
    truth = synth_input("lt", shape, seed, uniform=True) * 2 - 1
    w_down = [float(np.float32(w)) for w in np.linspace(1.0, 0.5, n_eval)] if weight is None else [float(weight)] * n_eval
    w_up = [float(np.float32(w)) for w in np.linspace(0.25, 1.0, n_eval)] if weight is None else [float(weight)] * n_eval
    block = lambda fs, mask, w: dict(kind="block", values=CR.block_mean(truth, fs), factors=fs, mask=mask, weights=w)
    spec = lambda f, w: dict(kind="spec", values=XR.apply(truth, PAN, f), R=PAN, f=f, mask=None, weights=w)
    if form == "block":
        return [block((1, 2, 4), synth_input("lm", (B, 1, H, W), seed, uniform=True), w_down)]
    if form == "spec":
        return [spec(2, w_down)]
    if form == "chain":
        return [spec(1, w_up), block((4, 4, 4), None, w_down)]
    return [dict(kind="psf", values=PR.apply(truth, H7, 2), h=H7, f=2, channels=None, iters=1, step=PR.step32(H7, 2, H, W), mask=None, weights=w_down)]


def _observation(links, sl=None, per_evaluation=True):
    """the product's objects for the links; sl(z, f): cuts a tensor that lives on the grid f times coarser (members, tiles)"""
    sl = sl or (lambda z, f: z)
    out = []
    for l in links:
        w = l["weights"] if per_evaluation else l["weights"][0]
        m = lambda f: None if l["mask"] is None else sl(l["mask"], f)
        if l["kind"] == "block":
            out.append(Observation(sl(l["values"], 1), l["factors"], m(1), w))
        elif l["kind"] == "spec":
            out.append(SpectralObservation(sl(l["values"], 1), l["R"], l["f"], m(1), w))
        else:
            out.append(PsfObservation(sl(l["values"], l["f"]), l["h"], l["f"], l["channels"], m(l["f"]), w, l["iters"]))
    return out[0] if len(out) == 1 else out


def _cpu_links(links, k):
    out = []
    for l in links:
        if l["kind"] == "block":
            out.append(XR.obs_link(l["values"], l["factors"], l["mask"], l["weights"][k]))
        elif l["kind"] == "spec":
            out.append(XR.spec_link(l["values"], l["R"], l["f"], l["mask"], l["weights"][k]))
        else:
            out.append(PR.psf_link(l["values"], l["h"], l["f"], l["channels"], l["mask"], l["weights"][k], l["iters"], l["step"]))
    return out


def _masked_cond(n, s, seed):
    return torch.cat([synth_input("cg", (n, 3, s, s), seed, uniform=True) * 2 - 1, rect_mask(n, s, s, seed)], 1)


@functools.lru_cache(maxsize=None)
def _case(form, variant, seed=71, weight=None):
    kw = VARIANTS[variant]
    resample = kw.get("resample")
    n_eval = _n_eval(resample)
    n_jump = len(RR.resample_schedule(T_CALL, *resample)[1]) if resample else 0
    c = dict(x_T=synth_input("qx", (2, 3, 16, 16), seed), noises=synth_input("qn", (n_eval, 2, 3, 16, 16), seed),
             jump_noises=synth_input("qj", (n_jump, 2, 3, 16, 16), seed) if n_jump else None, cond=_masked_cond(2, 16, seed) if kw.get("masked") else None,
             resample=resample, links=_links(form, (2, 3, 16, 16), n_eval, seed, weight) if form else [])
    return c


@functools.lru_cache(maxsize=None)
def _reference(form, variant, clip, observed=True):
    c = _case(form, variant)
    links = c["links"] if observed else []
    gt, mask = (None, None) if c["cond"] is None else (c["cond"][:, :3], c["cond"][:, 3:])
    return AR.ddpm_sampled(SCH.eo_cosine_tables(T_CALL), _tiny(), c["x_T"], c["noises"], lambda k: _cpu_links(links, k), clip, gt, mask, c["resample"],
                           c["jump_noises"])


def _call(m, c, clip=True, **kw):
    return m.sampling(2, clipped_reverse_diffusion=clip, device=DEV, cond=None if c["cond"] is None else c["cond"].to(DEV), x_T=c["x_T"],
                      noises=c["noises"], jump_noises=c["jump_noises"], resample=c["resample"], progress=False, **kw)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS)
def test_sampling_call_vs_cpu_loop(form, variant, clip, prec):
    """T = 20 on u_a0_tiny, batch 2, injected draws, one weight per evaluation and link; plain, with the RePaint mix of a known region, with
    resample = (4, 3) (52 evaluations, 8 jumps).  The CPU loop: the oracle UNet and the emulated split step with the emulated links."""
    c = _case(form, variant)
    ref = _reference(form, variant, clip)
    m = _model(prec, T=T_CALL, cond_type="sum" if c["cond"] is not None else None)
    out = _call(m, c, clip, observation=_observation(c["links"]))
    err = rel_l2(out.cpu(), ref)
    print(f"ancestral + {form}, {variant}, clip {clip} [{prec}]: rel-L2 vs the CPU loop = {err:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert bool(torch.isfinite(out).all()) and err < TRAJ_TOL[prec]
    assert rel_l2(_reference(form, variant, clip, False), ref) > 10 * TRAJ_TOL["fp32"]       # (the observation matters)


# ------------------------------------------------------------------------------------------------------------ 3. bits
class Counted:
    """a wrapper on the bound symbol eod_ddpm_pred_x0 that counts its calls"""

    def __init__(self):
        self.calls, self.lib = 0, _lib.lib()
        self.real = self.lib.eod_ddpm_pred_x0

    def __enter__(self):
        def counted(*a):
            self.calls += 1
            return self.real(*a)
        self.lib.eod_ddpm_pred_x0 = counted
        return self

    def __exit__(self, *exc):
        self.lib.eod_ddpm_pred_x0 = self.real


@torch.no_grad()
def _parent_sampling(m, c, clip):
    """the parent's path: the same chain with the update pinned to EODiffusion._ddpm_update (eod_ddpm_step on the model's buffers), step by step"""
    x = c["x_T"].to(DEV)
    gt, mask = (None, None) if c["cond"] is None else (c["cond"][:, :3].contiguous().to(DEV), c["cond"][:, 3:].contiguous().to(DEV))
    visits, _ = RR.walk_of(T_CALL, c["resample"])
    jumps = RR.resample_schedule(T_CALL, *c["resample"])[1] if c["resample"] else []
    after = {k: (j, a, b) for j, (k, a, b) in enumerate(jumps)}
    acp = m.alphas_cumprod.tolist()
    for k, i in enumerate(visits):
        t = torch.full((2,), i, dtype=torch.int64, device=DEV)
        z = c["noises"][k].to(DEV)
        if gt is not None:
            x = m._repaint_mix(x, gt, mask, t, z)
        x = m._ddpm_update(x, m.model(x, t), z, t, clip=clip)
        if k + 1 in after:
            j, a, b = after[k + 1]
            x = m._renoise(x, acp[a], acp[b], c["jump_noises"][j].to(DEV))
    return x


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_without_an_observation_the_parent_path_is_taken(variant):
    c = _case(None, variant)
    m = _model("fp32x3", T=T_CALL, cond_type="sum" if c["cond"] is not None else None)
    for clip in (True, False):
        with Counted() as n:
            got = _call(m, c, clip, observation=None)
            assert n.calls == 0 and torch.equal(got, _call(m, c, clip))
        assert bool(torch.isfinite(got).all()) and torch.equal(got, _parent_sampling(m, c, clip))
    with Counted() as n:
        _call(m, c, True, observation=_observation(_case("block", variant)["links"]))
        assert n.calls == _n_eval(c["resample"])


@pytest.mark.parametrize("form", FORMS)
def test_weight_0_with_the_clamp_is_the_call_without_an_observation(form):
    c = _case(form, "mix", weight=0.0)
    m = _model("fp32x3", T=T_CALL, cond_type="sum")
    free = _call(m, c, True)
    assert torch.equal(_call(m, c, True, observation=_observation(c["links"])), free)
    assert torch.equal(_call(m, c, True, observation=_observation(c["links"], per_evaluation=False)), free)
    assert not torch.equal(_call(m, c, True, observation=_observation(_case(form, "mix")["links"])), free)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("variant", ["plain", "resample"])
def test_weight_1_puts_the_observations_block_means_into_the_returned_sample(variant, clip):
    """at t = 0 the posterior step returns the projected prediction (beta_0 / (1 - acp_0) is 1.0f in the cosine schedule), so the RETURNED
    sample -- not merely the last pred_x0 -- has the observation's block means: 4 eps * max(1, |x|max).  The observation has no mask; the
    "resample" variant also mixes a known region in, in front of the UNet, which the projection behind it overrides."""
    c = _case(None, variant)
    truth = synth_input("wt", (2, 3, 16, 16), 5, uniform=True) * 2 - 1
    factors = (1, 2, 4)
    values = CR.block_mean(truth, factors)
    m = _model("fp32x3", T=T_CALL, cond_type="sum" if c["cond"] is not None else None)
    out = _call(m, c, clip, observation=Observation(values, factors, weight=1.0))
    miss = float((CO.block_mean(out, factors).cpu() - values).abs().max())
    bound = 4 * EPS * max(1.0, float(out.abs().max()))
    free = float((CO.block_mean(_call(m, c, clip), factors).cpu() - values).abs().max())
    print(f"{variant}, clip {clip}: max |block mean of the returned sample - values| = {miss:.3e} (bound {bound:.3e}; without the observation {free:.3e})")
    assert miss <= bound and free > 1e-2


# ------------------------------------------------------------------------------------------------------------ 4. scenes, stacks, shards
def _scene_links(form, H, W, n, seed, B=1):
    """links on a scene: "block" factors (1, 2, 4) under a soft mask; "spec" a pan band at f = 2; "psf" r = 0 (identity taps) at f = 4, bands
    0 and 2; "psf7": 7 taps at f = 2 (a footprint that crosses tile edges)"""
    truth = synth_input("st", (B, 3, H, W), seed, uniform=True) * 2 - 1
    w = [float(np.float32(v)) for v in np.linspace(1.0, 0.25, n)]
    if form == "block":
        return [dict(kind="block", values=CR.block_mean(truth, (1, 2, 4)), factors=(1, 2, 4), mask=synth_input("sm", (B, 1, H, W), seed, uniform=True), weights=w)]
    if form == "block8":
        return [dict(kind="block", values=CR.block_mean(truth, (8, 8, 4)), factors=(8, 8, 4), mask=None, weights=w)]
    if form == "spec":
        return [dict(kind="spec", values=XR.apply(truth, PAN, 2), R=PAN, f=2, mask=None, weights=w)]
    h, f = (np.array([1.0], np.float32), 4) if form == "psf" else (H7, 2)
    return [dict(kind="psf", values=PR.apply(truth, h, f, (0, 2)), h=h, f=f, channels=(0, 2), iters=2, step=PR.step32(h, f, H, W),
                 mask=synth_input("sm", (B, 1, H // f, W // f), seed, uniform=True), weights=w)]


def _cut_links(links, plan, s):
    out = []
    for l in links:
        f = l["f"] if l["kind"] == "psf" else 1
        cp = TilePlan(plan.H // f, plan.W // f, s // f, 0)
        out.append(dict(l, values=cut(l["values"], cp), mask=None if l["mask"] is None else cut(l["mask"], cp), step=PR.step32(l["h"], f, s, s) if l["kind"] == "psf" else None))
    return out


@pytest.mark.parametrize("form", ["block", "spec", "psf"])
def test_scene_with_overlap_0_equals_sampling_on_the_tiles(form):
    s, T, H, W = 16, 8, 32, 48
    m = _diffusion("fp32x3", False, T, s=s)
    plan = TilePlan(H, W, s, 0)
    x_T, noises = synth_input("sx", (1, 3, H, W), 81), synth_input("sn", (T, 1, 3, H, W), 81)
    links = _scene_links(form, H, W, T, 81)
    scene = m.sampling_scene((H, W), True, DEV, x_T=x_T, noises=noises, progress=False, observation=_observation(links))
    tiles = m.sampling(plan.n_tiles, True, DEV, x_T=cut(x_T, plan), noises=torch.stack([cut(z, plan) for z in noises]), progress=False,
                       observation=_observation(_cut_links(links, plan, s)))
    assert bool(torch.isfinite(scene).all()) and torch.equal(scene, stitch(tiles, plan))
    assert not torch.equal(scene, m.sampling_scene((H, W), True, DEV, x_T=x_T, noises=noises, progress=False))


@pytest.mark.parametrize("form", ["block8", "psf7"])
def test_blocks_that_a_tile_edge_cuts_equal_the_emulation_on_the_recorded_inputs(form):
    """overlap 8, tile 16, scene 24 x 40: the tiles start at multiples of 8 that are no multiples of 16 while blocks of 8 are anchored at the
    scene origin (and every PSF footprint crosses an edge).  The scene-level step is one pass over the scene: the recorded inputs of the
    call's last evaluations go through the emulation, which it equals bit for bit"""
    s, T, H, W = 16, 6, 24, 40
    plan = TilePlan(H, W, s, 8)
    assert len(plan.origins_x) > 2
    m = _diffusion("fp32x3", False, T, s=s)
    tb = _tables(T)[0]
    links = _scene_links(form, H, W, T, 82)
    seen, real = [], CO.ddpm_step

    def recording(bound, k, x_t, pred, noise, t, *rest):
        out = real(bound, k, x_t, pred, noise, t, *rest)
        seen.append((k, x_t.cpu(), pred.cpu(), noise.cpu(), t.cpu(), out.cpu()))
        return out
    CO.ddpm_step = recording
    try:
        scene = m.sampling_scene((H, W), True, DEV, overlap=8, x_T=synth_input("sx", (1, 3, H, W), 82), noises=synth_input("sn", (T, 1, 3, H, W), 82),
                                 progress=False, observation=_observation(links))
    finally:
        CO.ddpm_step = real
    assert [v[0] for v in seen] == list(range(T)) and seen[-1][1].shape == (1, 3, H, W)
    for k, x, e, z, t, out in seen[-2:]:
        assert t.tolist() == [T - 1 - k] and torch.equal(out, AR.step(tb, x, e, z, t, _cpu_links(links, k))[0])
    assert torch.equal(scene.cpu(), seen[-1][-1])


def test_member_b_of_a_stack_equals_the_single_scene_call():
    s, T, H, W, B = 16, 6, 24, 40, 2
    m = _diffusion("fp32x3", False, T, s=s)
    for form in ("block8", "psf7"):
        links = _scene_links(form, H, W, T, 83, B)
        x_T, noises = synth_input("sx", (B, 3, H, W), 83), synth_input("sn", (T, B, 3, H, W), 83)
        stack = m.sampling_scene((H, W), True, DEV, overlap=8, x_T=x_T, noises=noises, progress=False, n_scenes=B, observation=_observation(links))
        assert stack.shape == (B, 3, H, W) and bool(torch.isfinite(stack).all()) and not torch.equal(stack[:1], stack[1:])
        for b in range(B):
            one = m.sampling_scene((H, W), True, DEV, overlap=8, x_T=x_T[b:b + 1], noises=noises[:, b:b + 1], progress=False,
                                   observation=_observation(links, lambda z, f: z[b:b + 1]))
            assert torch.equal(stack[b:b + 1], one)
    # philox: member b is sample sample_offset + b, and the sharded call (one rank: the whole stack) is the stacked call
    from eo_diffusion_amd import dist as D
    obs = _observation(_scene_links("block8", H, W, T, 84, B))
    stack = m.sampling_scene((H, W), True, DEV, overlap=8, seed=5, progress=False, n_scenes=B, observation=obs)
    one = m.sampling_scene((H, W), True, DEV, overlap=8, seed=5, progress=False, sample_offset=1, observation=obs.shard(B, 1, 2))
    assert torch.equal(stack[1:], one)
    assert torch.equal(D.sharded_sampling_scene(m, (H, W), B, seed=5, overlap=8, device=DEV, observation=obs), stack)


def test_a_shard_of_a_philox_batch_equals_the_call_on_the_sharded_observation():
    from eo_diffusion_amd import dist as D
    m = _model("fp32x3", T=8)
    links = _links("chain", (4, 3, 16, 16), 8, 85) + _links("block", (4, 3, 16, 16), 8, 86)
    obs = _observation(links)
    full = m.sampling(4, device=DEV, rng="philox", seed=3, progress=False, observation=obs)
    part = m.sampling(2, device=DEV, rng="philox", seed=3, sample_offset=1, progress=False, observation=[o.shard(4, 1, 3) for o in obs])
    assert bool(torch.isfinite(full).all()) and torch.equal(full[1:3], part)
    assert torch.equal(D.sharded_sampling(m, 4, seed=3, device=DEV, observation=obs), full)
    assert not torch.equal(full, m.sampling(4, device=DEV, rng="philox", seed=3, progress=False))


def test_refusals_come_before_any_launch():
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    s, T, H, W = 16, 20, 32, 48
    m = EODiffusion(Never(), timesteps=T, image_size=s, in_channels=3, cond_type="sum", device=DEV).to(DEV)
    z = torch.zeros
    ok = Observation(z(1, 3, H, W), (1, 2, 4))
    psf = lambda *shape, **kw: PsfObservation(z(*shape), H7, 2, **kw)
    cond = z(1, 4, H, W)
    with Calls(m.model) as calls:
        for kw in (dict(observation=ok, skip_known=True), dict(observation=[ok, psf(1, 3, H // 2, W // 2)], skip_known=True),       # skip_known
                   dict(observation=Observation(z(1, 4, H, W), (1, 2, 4, 1))), dict(observation=SpectralObservation(z(1, 1, H, W), [[.5, .5]])),
                   dict(observation=psf(1, 4, H // 2, W // 2)),                                                                        # channel count
                   dict(observation=Observation(z(2, 3, H, W), (1, 2, 4))), dict(observation=Observation(z(3, 3, H, W), (1, 2, 4)), n_scenes=2),
                   dict(observation=Observation(z(1, 3, H, W), (1, 2, 4), mask=z(2, 1, H, W))), dict(observation=psf(3, 3, H // 2, W // 2), n_scenes=2),
                   dict(observation=Observation(z(1, 3, s, s), (1, 2, 4))),                                                            # not scene-sized
                   dict(observation=Observation(z(1, 3, H, W), (1, 2, 4), weight=[1.0] * (T + 1))),                                    # weights, walk
                   dict(observation=Observation(z(1, 3, H, W), (1, 2, 4), weight=[1.0] * T), resample=(4, 3)),
                   dict(observation=[ok, psf(1, 3, H // 2, W // 2, weight=[1.0] * 51)], resample=(4, 3)),
                   dict(observation=Observation(z(2, 3, H, W), (1, 2, 4), weight=[1.0] * 51), resample=(4, 3), n_scenes=2),
                   dict(observation=[ok] * 5), dict(observation=[ok, None]), dict(observation="obs")):
            with pytest.raises(EodError):
                m.sampling_scene((H, W), True, DEV, cond=cond, progress=False, **kw)
        for kw in (dict(observation=ok), dict(observation=Observation(z(3, 3, s, s), (1, 2, 4))), dict(observation=Observation(z(2, 4, s, s), (1, 2, 4, 1))),
                   dict(observation=[Observation(z(2, 3, s, s), (1, 2, 4), weight=[0.5] * (T - 1))]),
                   dict(observation=Observation(z(2, 3, s, s), (1, 2, 4), weight=[0.5] * T), resample=(4, 3)),
                   dict(observation=psf(2, 3, s // 4, s // 4)), dict(observation=[[ok]])):
            with pytest.raises(EodError):
                m.sampling(2, device=DEV, progress=False, **kw)
    assert calls.batches == []
