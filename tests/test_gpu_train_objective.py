"""GPU: the training objective -- eod_diffusion_loss, eod_grad_sumsq, eod_adamw_step_clipped -- through the C ABI against the numpy
references of tests/train_objective_ref.py (checked on the CPU in tests/test_train_objective_host.py), and the Python surface on top
(optim.diffusion_loss, optim.DiffusionLoss, optim.AdamW(max_grad_norm=...), EODiffusion.forward(t=...), EODiffusion.loss_weights).

Gates.  csrc/train.hip is built with -ffp-contract=off, so the float32 gradient (one IEEE operation at a time, s_n formed in double from
an exactly summed mask) and the AdamW update (given the device's own three scalars) are held to BIT EQUALITY.  The float64 sums are not
added in math.fsum's order; a float64 sum of E terms in any order lies within (E - 1) 2^-53 sum|terms| of the exact one and the division
by S_n adds one more 2^-53, so
    |per_sample[n] - fsum / S_n| <= E 2^-53 sum|terms| / S_n + half a float32 ulp of fsum / S_n         (the final rounding)
    |loss - fsum_n(w_n L_n) / N| <= sum_n |w_n| (the first term above) / N + (N + 1) 2^-53 sum_n |w_n L_n| / N + half a float32 ulp
and sqrt(sum g^2) within n 2^-53 relative of the exactly summed norm.  The worst observed ratio to each bound is printed (-s).

Every output lies between two 4 KiB guard bands and is NaN-filled before each launch; every launch runs twice and the two runs must agree
bit for bit (Out / twice of tests/test_gpu_glue_ops.py).  In-place kernels get their state copied in after the NaN fill."""
import collections
import gc
import math

import numpy as np
import pytest
import torch

from tests import train_objective_ref as R
from tests import train_tail_ref as RT
from tests.helpers import unet_cfgs
from tests.test_gpu_glue_ops import Out, Rng, _L, _lib, _ok, _p, _st, twice
from tests.test_gpu_train_tail import HP, GuardedAdamW, _bits_to_f32, _eq, _first_diff, _grad, _np, _opt_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, I32 = torch.float32, torch.float64, torch.int32
f32 = np.float32
EPS53 = 2.0 ** -53
WORST = collections.defaultdict(float)   # worst observed ratio to each derived bound (printed with -s)
KIND_ID = {"l2": 0, "l1": 1, "huber": 2}
NEW_ENTRY_POINTS = {"eod_diffusion_loss", "eod_diffusion_loss_workspace_size", "eod_grad_sumsq", "eod_grad_sumsq_workspace_size", "eod_adamw_step_clipped"}


def _half_ulp32(v):
    """half the float32 spacing at |v| (a float64 value)"""
    if v == 0.0 or not math.isfinite(v):
        return 0.0
    return 2.0 ** (max(math.frexp(abs(v))[1], -125) - 25)


def _put(a):
    """a numpy array (or tensor) as a device tensor between guard bands"""
    a = torch.as_tensor(np.ascontiguousarray(a)) if not isinstance(a, torch.Tensor) else a
    o = Out(tuple(a.shape), a.dtype)
    o.t.copy_(a)
    return o


class Loss:
    """one eod_diffusion_loss problem: inputs, outputs and the workspace between guard bands, the call made twice into NaN-filled outputs"""

    def __init__(self, pred, target, mask=None, weight=None, kind="l2", delta=1.0, want_grad=True):
        self.np = [None if a is None else np.ascontiguousarray(a, f32) for a in (pred, target, mask, weight)]
        self.kind, self.delta = kind, delta
        N, C, H, W = self.np[0].shape
        self.ins = [None if a is None else _put(a) for a in self.np]
        L = _L()
        nbytes = L.eod_diffusion_loss_workspace_size(N, C, H, W)
        assert nbytes > 0 and nbytes % 8 == 0
        LOSS, PER, WS = Out((1,)), Out((N,)), Out((nbytes // 8,), F64)
        DP = Out((N, C, H, W)) if want_grad else None
        m = self.np[2]
        ptrs = [0 if o is None else o.ptr for o in self.ins]

        def launch():
            _ok(L.eod_diffusion_loss(ptrs[0], ptrs[1], ptrs[2], 0 if m is None else m.shape[0], 0 if m is None else m.shape[1], ptrs[3], N, C, H, W,
                                     KIND_ID[kind], delta, LOSS.ptr, PER.ptr, 0 if DP is None else DP.ptr, WS.ptr, nbytes, _st()), "diffusion_loss")
        got = twice(launch, [LOSS, PER, WS] + ([DP] if want_grad else []))
        for o, a in zip(self.ins, self.np):
            assert o is None or (o.g.intact() and _eq(o.t, a)), "an input was written"
        self.loss, self.per = _np(got[0]), _np(got[1])
        self.dpred = _np(got[3]) if want_grad else None

    def check(self, tag):
        """against loss_ref: dpred bit for bit, loss and per_sample within the derived bounds"""
        pred, target, mask, weight = self.np
        ref = R.loss_ref(pred, target, mask, weight, self.kind, self.delta)
        N, E = pred.shape[0], pred[0].size
        assert _eq(self.dpred, ref["dpred"]), (tag, _first_diff(torch.from_numpy(self.dpred), ref["dpred"]))
        w = np.ones(N) if weight is None else weight.astype(np.float64)
        sum_err = np.zeros(N)
        for n in range(N):
            if ref["S"][n] <= 0:
                assert self.per[n] == 0 and not np.signbit(self.per[n]), (tag, n)
                continue
            sum_err[n] = E * EPS53 * ref["abs_terms"][n] / ref["S"][n]
            bound = sum_err[n] + _half_ulp32(ref["per64"][n])
            err = abs(float(self.per[n]) - ref["per64"][n])
            if bound > 0:
                WORST["per_sample"] = max(WORST["per_sample"], err / bound)
            assert err <= bound, (tag, n, float(self.per[n]), ref["per64"][n], err, bound)
        bound = float(np.sum(np.abs(w) * sum_err)) / N + (N + 1) * EPS53 * float(np.sum(np.abs(w * ref["per64"]))) / N + _half_ulp32(ref["loss64"])
        err = abs(float(self.loss[0]) - ref["loss64"])
        if bound > 0:
            WORST["loss"] = max(WORST["loss"], err / bound)
        assert err <= bound, (tag, float(self.loss[0]), ref["loss64"], err, bound)
        return ref


SHAPES = {1: (1, 1, 1), 7: (7, 1, 1), 2047: (23, 1, 89), 2048: (2, 32, 32), 2049: (3, 1, 683), 4097: (17, 1, 241), 3 * 64 * 64: (3, 64, 64)}
MASKS = [None, ("n1", False), ("n1", True), ("nc", True), ("11", False)]   # (shape, values k / 256 instead of 0 / 1)
DELTA = 0.75


def _mask(rng, N, C, H, W, spec):
    if spec is None:
        return None
    which, soft = spec
    shape = {"n1": (N, 1, H, W), "nc": (N, C, H, W), "11": (1, 1, H, W)}[which]
    m = (rng.random(shape) < 0.7).astype(f32)
    if soft:
        m = m * (rng.integers(1, 257, shape) / 256.0).astype(f32)
    m.reshape(shape[0], -1)[:, 0] = 1.0 if not soft else 0.5   # (no empty sample here: that is a test of its own)
    return m


def _data(rng, N, C, H, W):
    """pred / target with |d| exactly delta (both signs), d = +0 and -0 + 0, a subnormal d and a subnormal operand in front of every sample"""
    pred = rng.standard_normal((N, C, H, W)).astype(f32)
    target = rng.standard_normal((N, C, H, W)).astype(f32)
    P, T = pred.reshape(N, -1), target.reshape(N, -1)
    special = [(1.0 + DELTA, 1.0), (-0.25 - DELTA, -0.25), (0.5, 0.5), (-0.0, 0.0), (1e-40, 0.0), (3e-39, 2e-39), (2.0 * DELTA, DELTA)]
    E = P.shape[1]
    for n in range(N):
        for k, (a, b) in enumerate(special):
            P[n, (k + n) % E], T[n, (k + n) % E] = a, b
    return pred, target


@pytest.mark.parametrize("E", list(SHAPES))
def test_edge_diffusion_loss_sizes_masks_kinds(E):
    """E = C H W around one and two 2048-element chunks, N in {1, 2, 5}, no mask / [N,1,H,W] / [N,C,H,W] / [1,1,H,W] with 0/1 values and with
    values k / 256 (sums exact in double, so s_n is), the three kinds, with and without weights"""
    C, H, W = SHAPES[E]
    rng = np.random.default_rng(1000 + E)
    count = 0
    for N in (1, 2, 5):
        for mi, spec in enumerate(MASKS):
            for ki, kind in enumerate(R.KINDS):
                pred, target = _data(rng, N, C, H, W)
                mask = _mask(rng, N, C, H, W, spec)
                weight = (0.25 + rng.random(N)).astype(f32) if (N + mi + ki) % 2 else None
                Loss(pred, target, mask, weight, kind, DELTA).check((E, N, spec, kind, weight is not None))
                count += 1
    print(f"diffusion_loss E={E}: {count} problems; worst ratio to the bounds so far: per_sample {WORST['per_sample']:.4f}, loss {WORST['loss']:.4f}")


def test_edge_diffusion_loss_without_a_gradient_writes_the_same_loss():
    rng = np.random.default_rng(5)
    pred, target = _data(rng, 2, 3, 1, 683)
    mask = _mask(rng, 2, 3, 1, 683, ("n1", True))
    a, b = Loss(pred, target, mask, None, "huber", DELTA), Loss(pred, target, mask, None, "huber", DELTA, want_grad=False)
    assert _eq(a.loss, b.loss) and _eq(a.per, b.per)


@pytest.mark.parametrize("kind", R.KINDS)
def test_edge_diffusion_loss_skips_nan_and_inf_under_a_zero_mask(kind):
    """NaN / +-inf in pred and target wherever m = 0: loss and per_sample finite and bit-equal to the run with those positions zeroed, dpred
    there +0.0 (sign bit checked)"""
    rng = np.random.default_rng(6)
    N, C, H, W = 2, 3, 1, 683
    for spec in (("n1", False), ("nc", True), ("11", False)):
        pred, target = _data(rng, N, C, H, W)
        mask = _mask(rng, N, C, H, W, spec)
        dead = np.broadcast_to(mask, pred.shape) == 0
        assert dead.any() and not dead.all()
        clean = Loss(np.where(dead, f32(0), pred), np.where(dead, f32(0), target), mask, None, kind, DELTA)
        clean.check((kind, spec, "zeroed"))
        poison = np.array([np.nan, np.inf, -np.inf], f32)[rng.integers(0, 3, pred.shape)]
        pred[dead] = poison[dead]
        target[dead] = np.array([np.inf, np.nan, -np.inf, 1.0], f32)[rng.integers(0, 4, pred.shape)][dead]
        dirty = Loss(pred, target, mask, None, kind, DELTA)
        assert np.isfinite(dirty.loss).all() and np.isfinite(dirty.per).all()
        assert _eq(dirty.loss, clean.loss) and _eq(dirty.per, clean.per) and _eq(dirty.dpred, clean.dpred), (kind, spec)
        assert not dirty.dpred[dead].any() and not np.signbit(dirty.dpred[dead]).any(), (kind, spec, "dpred under m = 0 is not +0.0")


def test_edge_diffusion_loss_fully_masked_sample():
    """a sample whose mask is all zero: L_n = 0, dpred all +0.0, it still counts in N; the other samples' bits are those of the run in
    which it has a mask"""
    rng = np.random.default_rng(7)
    N, C, H, W = 3, 3, 1, 683
    for spec in (("n1", False), ("nc", True)):
        pred, target = _data(rng, N, C, H, W)
        mask = _mask(rng, N, C, H, W, spec)
        weight = (0.25 + rng.random(N)).astype(f32)
        full = Loss(pred, target, mask, weight, "huber", DELTA)
        mask0 = mask.copy()
        mask0[1] = 0.0
        pred[1, 0, 0, 5] = np.nan
        one = Loss(pred, target, mask0, weight, "huber", DELTA)
        ref = one.check((spec, "empty sample"))
        assert ref["S"][1] == 0 and one.per[1] == 0 and not np.signbit(one.per[1])
        assert not one.dpred[1].any() and not np.signbit(one.dpred[1]).any()
        for n in (0, 2):
            assert _eq(one.per[n:n + 1], full.per[n:n + 1]) and _eq(one.dpred[n], full.dpred[n]), (spec, n)
        assert math.isfinite(float(one.loss[0]))


def test_edge_diffusion_loss_a_sample_does_not_depend_on_its_batch():
    """per_sample[n] has the same bits alone (N = 1) and inside N = 5; dpred of sample n inside N = 5 with weight[n] = 5 has the bits of the
    run alone with weight 1: s_n = (float)(5 / (5 S)) against (float)(1 / (1 S)) -- 5 S is exact in double for these S (sums of k / 256 below
    2^14), so the two quotients are the correctly rounded value of the same real number 1 / S"""
    rng = np.random.default_rng(8)
    N, C, H, W = 5, 3, 1, 683
    for spec in (None, ("n1", True), ("nc", False)):
        pred, target = _data(rng, N, C, H, W)
        mask = _mask(rng, N, C, H, W, spec)
        weight = np.full(N, 5.0, f32)
        batch = Loss(pred, target, mask, weight, "huber", DELTA)
        batch.check((spec, "batch"))
        for n in range(N):
            alone = Loss(pred[n:n + 1], target[n:n + 1], None if mask is None else mask[n:n + 1], np.ones(1, f32), "huber", DELTA)
            assert _eq(alone.per, batch.per[n:n + 1]), (spec, n, "per_sample")
            assert _eq(alone.dpred[0], batch.dpred[n]), (spec, n, "dpred")


def test_edge_diffusion_loss_plain_l2_is_the_mse_loss():
    """no mask, no weight, l2 against eod_mse_loss.  Its float32 sum of n = 24 576 squares takes at most K = 1 + 8 + 96 additions along any
    path (one per thread, an 8-level tree, the serial sum of 96 workgroups), so it lies within K 2^-24 of the exact mean, relative; the
    gradient 2 d / n against (1 / n) (2 d): the same two roundings of the same real number up to the order, within 1 ulp"""
    from tests.test_train_objective_host import _ulps
    rng = np.random.default_rng(9)
    N, C, H, W = 2, 3, 64, 64
    pred, target = _data(rng, N, C, H, W)
    mine = Loss(pred, target, None, None, "l2", 1.0)
    ref = mine.check("plain l2")
    P, T = _put(pred), _put(target)
    LOSS, DP, SCR = Out((1,)), Out((N, C, H, W)), Out((1024,))
    n = pred.size
    got = twice(lambda: _ok(_L().eod_mse_loss(P.ptr, T.ptr, n, LOSS.ptr, DP.ptr, SCR.ptr, 1024, _st()), "mse_loss"), [LOSS, DP])
    K = 1 + 8 + 96
    assert abs(float(_np(got[0])[0]) - ref["loss64"]) <= (K + 3) * 2.0 ** -24 * ref["loss64"]   # (+ the squares, 1 / n and the product)
    assert abs(float(mine.loss[0]) - float(_np(got[0])[0])) <= (K + 4) * 2.0 ** -24 * ref["loss64"]
    u = _ulps(mine.dpred, _np(got[1]))
    print(f"plain l2 against eod_mse_loss: loss {float(mine.loss[0])!r} / {float(_np(got[0])[0])!r}, dpred worst {int(u.max())} ulp")
    assert u.max() <= 1


def test_edge_diffusion_loss_refusals():
    """the C entry point (return code, nothing written) and the Python surface (EodError before any launch)"""
    from eo_diffusion_amd import optim
    lib, L, st = _lib(), _L(), _st()
    N, C, H, W = 2, 3, 4, 4
    x = torch.zeros((N, C, H, W), device=DEV)
    LOSS, PER = Out((1,)), Out((N,))
    nbytes = L.eod_diffusion_loss_workspace_size(N, C, H, W)
    WS = Out((nbytes // 8,), F64)
    for o in (LOSS, PER):
        o.t.fill_(float("nan"))
    m = torch.ones((N, 1, H, W), device=DEV)
    bad = [("kind 3", (_p(x), _p(x), 0, 0, 0, 0, N, C, H, W, 3, 1.0, LOSS.ptr, PER.ptr, 0, WS.ptr, nbytes)),
           ("delta 0", (_p(x), _p(x), 0, 0, 0, 0, N, C, H, W, 2, 0.0, LOSS.ptr, PER.ptr, 0, WS.ptr, nbytes)),
           ("mask batch 3", (_p(x), _p(x), _p(m), 3, 1, 0, N, C, H, W, 0, 1.0, LOSS.ptr, PER.ptr, 0, WS.ptr, nbytes)),
           ("mask channels 2", (_p(x), _p(x), _p(m), N, 2, 0, N, C, H, W, 0, 1.0, LOSS.ptr, PER.ptr, 0, WS.ptr, nbytes)),
           ("short workspace", (_p(x), _p(x), 0, 0, 0, 0, N, C, H, W, 0, 1.0, LOSS.ptr, PER.ptr, 0, WS.ptr, nbytes - 8)),
           ("unaligned workspace", (_p(x), _p(x), 0, 0, 0, 0, N, C, H, W, 0, 1.0, LOSS.ptr, PER.ptr, 0, WS.ptr + 4, nbytes)),
           ("no pred", (0, _p(x), 0, 0, 0, 0, N, C, H, W, 0, 1.0, LOSS.ptr, PER.ptr, 0, WS.ptr, nbytes))]
    for what, args in bad:
        assert L.eod_diffusion_loss(*args, st) != 0, what
        torch.cuda.synchronize()
        assert bool(LOSS.t.isnan().all()) and bool(PER.t.isnan().all()), what
    assert L.eod_diffusion_loss_workspace_size(0, 3, 4, 4) == -1 and L.eod_grad_sumsq_workspace_size(0) == -1
    E = lib.EodError
    for kw in (dict(kind="mse"), dict(delta=0.0), dict(delta=float("nan")), dict(weight=torch.ones(3, device=DEV)), dict(weight=torch.ones((N, 1), device=DEV)),
               dict(mask=torch.ones((N, 2, H, W), device=DEV)), dict(mask=torch.ones((3, 1, H, W), device=DEV)), dict(mask=torch.ones((N, 1, H, 5), device=DEV)),
               dict(mask=torch.ones((N, 1, H, W))), dict(weight=torch.ones(N, device=DEV, dtype=torch.float64)), dict(mask=torch.ones((H, W), device=DEV))):
        with pytest.raises(E):
            optim.diffusion_loss(x, x, **kw)
    for a, b in ((x, x[:1]), (x.half(), x.half()), (x.cpu(), x.cpu()), (x[0], x[0])):
        with pytest.raises(E):
            optim.diffusion_loss(a, b)
    with pytest.raises(E):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, device=DEV))], max_grad_norm=1.0, skip_nonfinite=False)
    for v in (0.0, -1.0, "1"):
        with pytest.raises(E):
            optim.AdamW([torch.nn.Parameter(torch.zeros(4, device=DEV))], max_grad_norm=v)


# ================================================================================================ DiffusionLoss under autograd
@pytest.mark.parametrize("kind", R.KINDS)
def test_diffusion_loss_module_under_autograd(kind):
    from eo_diffusion_amd import optim
    rng = np.random.default_rng(21)
    N, C, H, W = 2, 3, 1, 683
    pred, target = _data(rng, N, C, H, W)
    mask, weight = _mask(rng, N, C, H, W, ("n1", True)), (0.25 + rng.random(N)).astype(f32)
    dev = [torch.from_numpy(a).to(DEV) for a in (pred, target, mask, weight)]
    loss0, dp, per = optim.diffusion_loss(dev[0], dev[1], mask=dev[2], weight=dev[3], kind=kind, delta=DELTA, return_per_sample=True)
    ref = R.loss_ref(pred, target, mask, weight, kind, DELTA)
    assert _eq(dp, ref["dpred"]) and tuple(loss0.shape) == (1,) and tuple(per.shape) == (N,)
    fn = optim.DiffusionLoss(kind, DELTA)
    for factor in (None, 3.0):
        leaf = dev[0].clone().requires_grad_(True)
        loss = fn(leaf, dev[1], mask=dev[2], weight=dev[3])
        assert loss.dim() == 0 and loss.requires_grad and _eq(loss.detach().reshape(1), _np(loss0))
        (loss if factor is None else loss * factor).backward()
        want = dp if factor is None else dp * factor
        assert _eq(leaf.grad, _np(want)), (kind, factor)
        assert _eq(fn.per_sample, _np(per))
    lo, none = optim.diffusion_loss(dev[0], dev[1], kind=kind, delta=DELTA, want_grad=False)
    assert none is None and math.isfinite(float(lo))


# ================================================================================================ eod_grad_sumsq + eod_adamw_step_clipped
class ClippedAdamW:
    """p / m / v, the 10-int state, the group's double and the scan's slots of direct eod_grad_sumsq + eod_adamw_step_clipped calls, every
    buffer between guard bands.  Each call runs twice from the same state and returns (before, after, state after as a dict)"""

    def __init__(self, n, slots, seed, wd=0.01):
        self.n, self.slots, self.wd = n, slots, wd
        self.cur = list(_opt_state(Rng(seed), n))
        self.state = torch.zeros((10,), dtype=I32, device=DEV)
        self.P, self.M, self.V, self.G = Out((n,)), Out((n,)), Out((n,)), Out((n,))
        self.S, self.Q = Out((10,), I32), Out((1,), F64)
        self.nbytes = _L().eod_grad_sumsq_workspace_size(slots)
        self.W = Out((self.nbytes // 8,), F64)
        self.calls = 0

    def step(self, g, max_norm):
        self.calls += 1
        L, st = _L(), _st()
        states = []
        self.G.t.copy_(g)

        def prefill():
            for o, s in zip((self.P, self.M, self.V), self.cur):
                o.t.copy_(s)
            self.S.t.copy_(self.state)

        def launch():
            _ok(L.eod_grad_sumsq(self.G.ptr, self.n, self.Q.ptr, self.W.ptr, self.nbytes, self.slots, st), "grad_sumsq")
            _ok(L.eod_adamw_step_clipped(self.P.ptr, self.G.ptr, self.M.ptr, self.V.ptr, self.n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], self.wd,
                                         self.calls, max_norm, self.Q.ptr, 1, self.S.ptr, st), "adamw_step_clipped")
            states.append(self.S.t.clone())
        got = twice(launch, [self.P, self.M, self.V, self.Q, self.W], prefill)[:3]
        assert torch.equal(states[0], states[1]), "two runs of the same call leave different states"
        assert self.S.g.intact() and self.G.g.intact(), "write outside the state / into the gradient's guard bands"
        assert _eq(self.G.t, _np(g)), "the gradient was written"
        before = self.cur
        self.cur, self.state = [t.clone() for t in got], states[0]
        s = states[0].cpu()
        return before, got, dict(skip=int(s[0]), skipped=int(s[1]), clip=int(s[2]), clipped=int(s[3]), bc2_sqrt=_bits_to_f32(int(s[4])),
                                 neg_step_size=_bits_to_f32(int(s[5])), coef=_bits_to_f32(int(s[6])), pad=int(s[7]),
                                 norm=float(s[8:10].view(F64)[0]))


def _check_clipped_call(o, g, max_norm, before, got, s, skipped, clipped):
    """counters; the norm within n 2^-53 relative and coef within 1 ulp of the rule on the exactly summed norm; the update bit for bit given
    the device's three scalars"""
    gn = _np(g)
    assert s["skip"] == 0 and s["skipped"] == skipped and s["pad"] == 0, (o.calls, s)
    norm = R.grad_norm_ref(gn)
    err = abs(s["norm"] - norm)
    if norm > 0:
        WORST["total_norm"] = max(WORST["total_norm"], err / (o.n * EPS53 * norm))
    assert err <= o.n * EPS53 * norm, (o.n, o.slots, s["norm"], norm)
    want = R.clip_coef_ref(norm, max_norm)
    assert RT.ulps32(s["coef"], want) <= 1 and 0 < s["coef"] <= 1, (s["coef"], want)
    assert s["clip"] == int(s["coef"] < 1) and s["clipped"] == clipped + s["clip"], (o.calls, s, clipped)
    applied = o.calls - skipped
    for name, h in zip(("bc2_sqrt", "neg_step_size"), RT.host_scalars(HP["lr"], HP["beta1"], HP["beta2"], applied)):
        assert np.isfinite(s[name]) and RT.ulps32(s[name], f32(h)) <= 1, (name, o.calls, applied, float(s[name]), h)
    ref = R.adamw_clipped_ref(_np(before[0]), gn, _np(before[1]), _np(before[2]), s["coef"], 1.0 - HP["lr"] * o.wd, HP["beta1"], HP["beta2"], HP["eps"],
                              s["bc2_sqrt"], s["neg_step_size"])
    for name, a, b in zip("pmv", got, ref):
        assert _eq(a, b), (o.n, o.slots, o.calls, name, _first_diff(a, b))
    return s["clipped"]


BIG_N = 8192 * 256 + 3   # the update's grid is capped at 8192 blocks of 256 threads: its second trip; 1025 chunks for at most 8192 slots


@pytest.mark.parametrize("slots", [1, 7, 8192])
@pytest.mark.parametrize("n", [1, 4, 255, 256, 257, 2047, 2049, BIG_N])
def test_edge_adamw_clipped_sizes_and_slots(n, slots):
    """three consecutive steps: max_norm half the norm (clipped), twice the norm (coef exactly 1), then a quarter (clipped again)"""
    o = ClippedAdamW(n, slots, seed=71)
    r = Rng(72)
    clipped = 0
    for k, factor in enumerate((0.5, 2.0, 0.25)):
        g = _grad(r, n, k)
        if n <= 4:
            g[n - 1] = 0.3 * (k + 1)   # (_grad zeroes element 0: keep a norm)
        max_norm = factor * R.grad_norm_ref(_np(g))
        before, got, s = o.step(g, max_norm)
        clipped = _check_clipped_call(o, g, max_norm, before, got, s, 0, clipped)
        assert s["clip"] == int(factor < 1) and (factor < 1 or s["coef"] == 1.0)
    assert clipped == 2
    print(f"clipped AdamW n={n} slots={slots}: worst ratio of the norm's error to n 2^-53 so far: {WORST['total_norm']:.4f}")


@pytest.mark.parametrize("n,slots", [(257, 1), (2049, 7), (BIG_N, 8192)])
def test_edge_adamw_clipped_with_coef_one_is_the_guarded_step(n, slots):
    """max_norm = inf and max_norm above the norm: coef is exactly 1.0 and p / m / v are, bit for bit, eod_adamw_step_guarded's on the same
    inputs (both compute their two step-dependent scalars with the same device expressions)"""
    a, b = ClippedAdamW(n, slots, seed=73), GuardedAdamW(n, 8192, seed=73)
    r = Rng(74)
    for k, max_norm in enumerate((math.inf, None, math.inf)):
        g = _grad(r, n, k)
        norm = R.grad_norm_ref(_np(g))
        before, got, s = a.step(g, 1.5 * norm + 1.0 if max_norm is None else max_norm)
        _, want, state = b.step(g)
        assert s["coef"] == 1.0 and s["clip"] == 0 and s["clipped"] == 0 and s["skip"] == 0
        assert abs(s["norm"] - norm) <= n * EPS53 * norm
        assert (s["bc2_sqrt"], s["neg_step_size"]) == (_bits_to_f32(state[2]), _bits_to_f32(state[3]))
        for name, x, y in zip("pmv", got, want):
            assert _eq(x, _np(y)), (n, k, name, _first_diff(x, _np(y)))


@pytest.mark.parametrize("slots", [1, 7])
def test_edge_adamw_clipped_skips_on_one_bad_value_anywhere(slots):
    """one +inf / -inf / NaN at the first, a middle and the last index: the step is skipped -- p / m / v untouched, the counters advance, no
    clip is counted, the norm reads inf or NaN -- and the next finite call is the FIRST applied step (bias corrections for a = 1)"""
    n = 5000
    r = Rng(75)
    for bad in (math.inf, -math.inf, math.nan):
        for idx in (0, n // 2 + 1, n - 1):
            o = ClippedAdamW(n, slots, seed=76)
            g = _grad(r, n, 0)
            g[idx] = bad
            before, got, s = o.step(g, 0.01)
            assert (s["skip"], s["skipped"], s["clip"], s["clipped"]) == (1, 1, 0, 0) and not math.isfinite(s["norm"]) and s["coef"] == 1.0, (bad, idx, s)
            for name, x, y in zip("pmv", got, before):
                assert _eq(x, _np(y)), (bad, idx, name, "a skipped call changed it")
    g = _grad(r, n, 1)
    max_norm = 0.5 * R.grad_norm_ref(_np(g))
    before, got, s = o.step(g, max_norm)
    assert _check_clipped_call(o, g, max_norm, before, got, s, 1, 0) == 1
    assert RT.ulps32(s["neg_step_size"], f32(-HP["lr"] / (1.0 - HP["beta1"]))) <= 1
    g = _grad(r, n, 2)
    g[7] = 3.0e38   # finite extremes are not flagged: the square is far inside the double range
    g[8] = -3.4028234663852886e38
    max_norm = 1.0
    before, got, s = o.step(g, max_norm)
    assert _check_clipped_call(o, g, max_norm, before, got, s, 1, 1) == 2


def test_edge_adamw_clipped_refusals():
    L, st = _L(), _st()
    n = 64
    t = [torch.zeros((n,), device=DEV) for _ in range(4)]
    state, q = torch.zeros((10,), dtype=I32, device=DEV), torch.zeros((2,), dtype=F64, device=DEV)
    ws = torch.zeros((8,), dtype=F64, device=DEV)
    args = lambda **kw: [_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, kw.get("step", 1), kw.get("max_norm", 1.0),
                         kw.get("q", _p(q)), kw.get("groups", 1), kw.get("state", _p(state)), st]
    for what, kw in (("max_norm 0", dict(max_norm=0.0)), ("max_norm NaN", dict(max_norm=math.nan)), ("no groups", dict(groups=0)), ("step 0", dict(step=0)),
                     ("state unaligned", dict(state=_p(state) + 4)), ("sumsq unaligned", dict(q=_p(q) + 4)), ("no state", dict(state=0))):
        assert L.eod_adamw_step_clipped(*args(**kw)) != 0, what
    assert L.eod_grad_sumsq(_p(t[1]), n, _p(q), _p(ws), 64, 8, st) == 0
    for what, a in (("n 0", (_p(t[1]), 0, _p(q), _p(ws), 64, 8)), ("short workspace", (_p(t[1]), n, _p(q), _p(ws), 56, 8)), ("no slots", (_p(t[1]), n, _p(q), _p(ws), 64, 0)),
                    ("sumsq unaligned", (_p(t[1]), n, _p(q) + 4, _p(ws), 64, 8))):
        assert L.eod_grad_sumsq(*a, st) != 0, what
    torch.cuda.synchronize()
    assert not any(bool(x.any()) for x in t) and not bool(state.any())


def test_adamw_two_parameter_groups_share_one_global_norm():
    """optim.AdamW(max_grad_norm=...) with groups of 257 and 2049 parameters (the copy path of step(): the gradients are tensors of their
    own): last_grad_norm() is the norm of the concatenation, both groups use one coef, and p.grad keeps the raw gradient"""
    from eo_diffusion_amd import optim
    r = Rng(81)
    ps = [torch.nn.Parameter(r.randn((257,))), torch.nn.Parameter(r.randn((2049,)))]
    gs = [r.randn((257,), 0.5), r.randn((2049,), 0.25)]
    norm = R.grad_norm_ref(_np(gs[0]), _np(gs[1]))
    opt = optim.AdamW([dict(params=[ps[0]]), dict(params=[ps[1]], lr=2e-3)], lr=1e-3, max_grad_norm=0.5 * norm)
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    opt.step()
    got = opt.last_grad_norm()
    assert abs(got - norm) <= (257 + 2049) * EPS53 * norm, (got, norm)
    coefs = [_bits_to_f32(int(st["clip"][6])) for st in opt._flat]
    assert coefs[0] == coefs[1] and RT.ulps32(coefs[0], R.clip_coef_ref(norm, 0.5 * norm)) <= 1 and opt.last_clip_coef() == float(coefs[0])
    assert opt.clipped_steps() == 1 and opt.skipped_steps() == 0
    for st, g in zip(opt._flat, gs):
        _check_first_moment(st, [g], coefs[0], torch.zeros_like(st["m"]))
    for p, g in zip(ps, gs):   # a second step above the norm, then one with an inf in the SECOND group: both groups skip
        p.grad = g.clone()
    opt.max_grad_norm = 4.0 * norm
    opt.step()
    assert opt.last_clip_coef() == 1.0 and opt.clipped_steps() == 1
    before = [p.detach().clone() for p in ps]
    ps[1].grad[100] = float("inf")
    opt.step()
    assert opt.skipped_steps() == 1 and math.isinf(opt.last_grad_norm()) and all(int(st["clip"][0]) == 1 for st in opt._flat)
    assert all(_eq(p.detach(), _np(b)) for p, b in zip(ps, before))


# ================================================================================================ end to end
def _check_first_moment(st, raws, coef, m0, b1=0.9):
    """the group's m buffer is beta1 m0 + (1 - beta1) (g coef) in float32, bit for bit, over every parameter that had a gradient
    (raws: the raw gradients in the group's parameter order, None where there was none: those keep m0)"""
    off = 0
    for p, g in zip(st["params"], raws):
        sl = slice(off, off + p.numel())
        old = _np(m0[sl])
        if g is None:
            assert _eq(st["m"][sl], old), "a parameter without a gradient lost its moment"
        else:
            want = (old * f32(b1) + (_np(g).reshape(-1) * f32(coef)).astype(f32) * f32(1.0 - b1)).astype(f32)
            assert _eq(st["m"][sl], want), ("m is not beta1 m + (1 - beta1) (g coef)", _first_diff(st["m"][sl], want))
            assert _eq(p.grad, _np(g)), "p.grad was scaled"
        off += (p.numel() + 3) // 4 * 4


def _blob_mask(N, H, W, seed):
    """a synthetic cloud per chip: 0 inside a disc, 1 outside"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.ones((N, 1, H, W), f32)
    for n in range(N):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.2, 0.4) * H
        m[n, 0][(yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2] = 0.0
    return m


def _record(monkeypatch):
    lib = _lib()
    L = lib.lib()
    called = collections.Counter()

    def wrap(name, fn):
        def w(*a):
            called[name] += 1
            return fn(*a)
        w.__name__ = name
        return w
    for name in lib.SYMBOLS:
        monkeypatch.setattr(L, name, wrap(name, getattr(L, name)))
    return called


def _model(prec, seed=7):
    from eo_diffusion_amd.backbones import unet_openai as U
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from tests.synth import synth_state_dict
    cfg = unet_cfgs()["u_a1_tiny"]
    unet = U.UNetModel(**cfg).set_precision(prec)
    unet.load_state_dict(synth_state_dict(U.unet_param_shapes(**cfg), seed))
    S = cfg["image_size"]
    return EODiffusion(unet, timesteps=1000, image_size=S, in_channels=cfg["in_channels"]).to(DEV).train(), S, cfg["in_channels"]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_training_step_end_to_end_with_mask_weights_and_clipping(prec, monkeypatch):
    """forward(t=t) -> DiffusionLoss("huber") with a blob mask and min-SNR weights -> loss.backward() -> AdamW(max_grad_norm).step() on
    u_a1_tiny at batch 2"""
    from eo_diffusion_amd import optim
    model, S, C = _model(prec)
    r = Rng(91)
    x, noise = r.rand((2, C, S, S)), r.randn((2, C, S, S))
    t = torch.tensor([37, 801], dtype=torch.int64)
    mask = torch.from_numpy(_blob_mask(2, S, S, 3)).to(DEV)
    assert 0 < float(mask.mean()) < 1
    weight = model.loss_weights("min_snr", 5.0)[t.to(DEV)]
    assert weight.dtype == F32 and tuple(weight.shape) == (2,) and 0 < float(weight[0]) < 1 and float(weight[1]) == 1.0   # (SNR above / below gamma)
    # 1. the timesteps handed in are the timesteps used: the same bits as the internal draw returning them
    with torch.no_grad():
        given = model(x, noise, t=t).clone()
        with monkeypatch.context() as mp:
            mp.setattr(torch, "randint", lambda *a, **k: t.clone())
            drawn = model(x, noise).clone()
    assert _eq(given, _np(drawn)) and bool(torch.isfinite(given).all())
    with pytest.raises(_lib().EodError):
        model(x, noise, t=t.int())
    with pytest.raises(_lib().EodError):
        model(x, noise, t=t[:1])
    # 2. - 3. one backward to see the norm
    loss_fn = optim.DiffusionLoss("huber", 0.5)

    def backward():
        loss = loss_fn(model(x, noise, t=t.to(DEV)), noise, mask=mask, weight=weight)
        loss.backward()
        return float(loss.detach())
    backward()
    grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
    seen = R.grad_norm_ref(*[_np(g) for g in grads])
    assert math.isfinite(seen) and seen > 0
    model.zero_grad(set_to_none=True)
    # 4. the clipped step
    b1 = 0.9
    opt = optim.AdamW(model.parameters(), lr=1e-3, betas=(b1, 0.999), max_grad_norm=0.5 * seen)
    losses = [backward()]
    st = opt._flat[0]
    raw = [None if p.grad is None else p.grad.detach().clone() for p in st["params"]]
    opt.step()
    norm, coef = opt.last_grad_norm(), f32(opt.last_clip_coef())
    assert abs(norm - seen) <= 1e-3 * seen and opt.clipped_steps() == 1 and opt.skipped_steps() == 0
    assert RT.ulps32(coef, R.clip_coef_ref(norm, 0.5 * seen)) <= 1 and coef < 1
    assert any(g is not None for g in raw)
    _check_first_moment(st, raw, coef, torch.zeros_like(st["m"]), b1)
    opt.zero_grad()
    for _ in range(9):
        losses.append(backward())
        opt.step()
        opt.zero_grad()
    losses.append(backward())
    print(f"end to end {prec}: norm {norm:.4g}, coef {float(coef):.4g}, clipped {opt.clipped_steps()} of 10, loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    assert tuple(loss_fn.per_sample.shape) == (2,)
    del opt, model
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_default_training_loop_takes_todays_calls(prec, monkeypatch):
    """max_grad_norm=None: the optimizer's calls are today's (eod_adamw_step_guarded, no scan of the new kind, no clipped step) with
    DiffusionLoss("l2") as with nn.MSELoss, and the nn.MSELoss loop touches none of the new entry points; with max_grad_norm set the same
    loop runs the new ones and no guarded step -- on the copy path (autograd bridge) and on the in-place path (UNetTrainer.backward)"""
    from eo_diffusion_amd import optim
    from eo_diffusion_amd.training import UNetTrainer
    called = _record(monkeypatch)
    r = Rng(95)

    def loop(loss_fn, max_grad_norm):
        model, S, C = _model(prec)
        opt = optim.AdamW(model.parameters(), lr=1e-3, max_grad_norm=max_grad_norm)
        x, noise = r.rand((2, C, S, S)), r.randn((2, C, S, S))
        called.clear()
        for _ in range(2):
            loss = loss_fn(model(x, noise), noise)
            loss.backward()
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        assert math.isfinite(float(loss.detach()))
        return {n for n in called if called[n]}, opt, model, S, C
    names, *_ = loop(torch.nn.MSELoss(reduction="mean"), None)
    assert "eod_adamw_step_guarded" in names and not names & NEW_ENTRY_POINTS, sorted(names & NEW_ENTRY_POINTS)
    names, *_ = loop(optim.DiffusionLoss("l2"), None)
    assert "eod_adamw_step_guarded" in names and "eod_diffusion_loss" in names and not names & {"eod_grad_sumsq", "eod_adamw_step_clipped"}
    names, opt, model, S, C = loop(optim.DiffusionLoss("l2"), 1e-3)
    assert {"eod_grad_sumsq", "eod_adamw_step_clipped", "eod_diffusion_loss"} <= names and "eod_adamw_step_guarded" not in names
    assert opt.clipped_steps() == 2
    # the in-place path: the trainer's flat gradient is read where it lies
    tr = UNetTrainer(model.model, 2, S, S, DEV, loss_scale=(256.0 if prec == "fp16" else 1.0))
    x, noise, t = r.rand((2, C, S, S)), r.randn((2, C, S, S)), torch.tensor([7, 650], device=DEV)
    loss, dpred = optim.diffusion_loss(tr.forward(x, t), noise, kind="l1")
    tr.backward(dpred, allreduce=True)   # (one process: the buckets stay local)
    st0 = opt._flat[0]
    raws = [None if p.grad is None else p.grad.detach().clone() for p in st0["params"]]
    flat, m0 = tr.flat_grad.detach().clone(), st0["m"].clone()
    assert all(g is None or p.grad.untyped_storage().data_ptr() == tr.flat_grad.untyped_storage().data_ptr() for p, g in zip(st0["params"], raws))
    opt.step()
    n = st0["p"].numel()
    norm = R.grad_norm_ref(_np(flat)[:n])
    assert abs(opt.last_grad_norm() - norm) <= n * EPS53 * norm and opt.clipped_steps() == 3
    assert _eq(tr.flat_grad, _np(flat)), "the flat gradient was written"
    _check_first_moment(st0, raws, opt.last_clip_coef(), m0)
    del tr, opt, model
    gc.collect()
    torch.cuda.empty_cache()
