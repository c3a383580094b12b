"""GPU: the kernels of a UNetTrainer step that the chain tests of tests/test_gpu_train_kernels.py do not see -- the one-launch weight
re-pack (eod_pack_jobs, and the single-job entry points it replaced), eod_dropout, eod_add, eod_adamw_step, eod_ema_update and
eod_adamw_step_guarded -- each called through the C ABI and compared with the numpy references of tests/train_tail_ref.py and
oracle/train_ref.py (checked on the CPU in tests/test_train_tail_ref.py and tests/test_oracle_golden.py).

csrc/train.hip is built with -ffp-contract=off and these kernels are single IEEE operations per element, so every gate is BIT EQUALITY
(NaNs compare as NaNs: the payload of inf + -inf is the hardware's), with one exception: the two step-dependent scalars that
eod_adamw_step_guarded computes on the device in double `pow`, which are held to 1 ulp (float32) of the same expression in host double --
both sides round a double that is accurate to a few double ulps, so they can differ only where that double lies next to a float32
rounding boundary, and then by one unit.  The update itself is compared bit for bit given the device's own scalars.

Every output lies between two 4 KiB guard bands and is NaN-filled before each launch (Out / twice of tests/test_gpu_glue_ops.py); every
launch runs twice and the two runs must agree bit for bit.  In-place kernels get their state copied in after the NaN fill (prefill).

Not testable: the high counter word of the dropout draw (element // 4 >> 32) needs more than 2^34 elements; and at p = 0 the kernel keeps
an element iff its draw is < 0xFFFFFFFF, so a draw of exactly 0xFFFFFFFF (a 2^-32 event per element) is dropped -- no test reaches it
(DESIGN section 4)."""
import collections
import gc
import math

import numpy as np
import pytest
import torch

from oracle import train_ref as TR
from tests import train_tail_ref as R
from tests.helpers import unet_cfgs
from tests.test_gpu_conv_programs import Guarded  # noqa: F401  (Out is built on it)
from tests.test_gpu_glue_ops import Out, Rng, _L, _lib, _ok, _p, _st, twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, I32 = torch.float16, torch.float32, torch.int32
NPT = {F16: np.float16, F32: np.float32}
FLT_MAX = 3.4028234663852886e38
COUNT = collections.Counter()  # device / host scalar comparisons of this session (printed with -s)


def _dt(dtype):
    return _lib().EOD_F16 if dtype == F16 else _lib().EOD_F32


def _np(t):
    return t.detach().cpu().numpy()


def _eq(got, ref):
    """bit equality of a tensor (or array) with a numpy array; NaN matches NaN of any payload"""
    g = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    if g.dtype != ref.dtype or g.shape != ref.shape:
        return False
    u = {2: np.uint16, 4: np.uint32}[g.dtype.itemsize]
    gn, rn = np.isnan(g), np.isnan(ref)
    return bool(np.array_equal(gn, rn)) and bool(np.array_equal(np.ascontiguousarray(g).view(u)[~gn], np.ascontiguousarray(ref).view(u)[~rn]))


def _first_diff(got, ref):
    g, ref = _np(got).reshape(-1), np.asarray(ref).reshape(-1)
    if g.shape != ref.shape or g.dtype != ref.dtype:
        return f"shape / dtype: got {g.shape} {g.dtype}, want {ref.shape} {ref.dtype}"
    bad = np.nonzero(~((g == ref) | (np.isnan(g) & np.isnan(ref))))[0]
    return f"{bad.size} of {g.size} differ, first at {bad[:4].tolist()}: got {g[bad[:4]].tolist()} want {ref[bad[:4]].tolist()}" if bad.size else "sign of zero"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================================================ 2. eod_pack_jobs
def _job_total(j):
    return j["taps"] * (j["nci"] if j["kind"] else j["Cout"]) * j["cpad"]


def _launch_jobs(jobs, dtype):
    """jobs: dicts with w / dst pointers and the geometry -> one eod_pack_jobs launch (table and block lists built here, the way
    include/eodiff.h describes them: one block per EOD_PACK_CHUNK destination elements of a job)"""
    lib = _lib()
    arr = (lib.PackJob * len(jobs))()
    blk_job, blk_first = [], []
    for k, j in enumerate(jobs):
        a = arr[k]
        a.w, a.dst, a.kind, a.Cout, a.Cin, a.taps, a.ci0, a.nci, a.cpad = (j[f] for f in ("w", "dst", "kind", "Cout", "Cin", "taps", "ci0", "nci", "cpad"))
        for first in range(0, _job_total(j), lib.PACK_CHUNK):
            blk_job.append(k)
            blk_first.append(first)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    bj = torch.tensor(blk_job, dtype=torch.int32, device=DEV)
    bf = torch.tensor(blk_first, dtype=torch.int64, device=DEV)
    return lambda: _ok(_L().eod_pack_jobs(_p(tab), _p(bj), _p(bf), len(blk_job), _dt(dtype), _st()), "pack_jobs")


def _hand_jobs(up4_taps):
    """(kind, Cout, Cin, taps, ci0, nci, cpad).  Destination sizes: 48 (below one 256-thread step), 4096, 4096 + 1, 3 * 4096 - 255"""
    return [
        (0, 3, 3, 1, 0, 0, 16),              # 48 elements
        (0, 32, 3, 9, 0, 0, 16),             # the first conv, 3 input channels padded to 16
        (0, 8, 13, 9, 0, 0, 16),             # ... and 13
        (0, 64, 64, 1, 0, 0, 64),            # exactly one chunk
        (1, 240, 40, 1, 5, 17, 241),         # one chunk + 1; ci0 > 0, ci0 + nci < Cin, nci % 4 != 0, cpad > Cout
        (1, 190, 20, 9, 3, 7, 191),          # 3 chunks - 255
        (1, 3, 32, 9, 0, 32, 8),             # the head conv: cpad > Cout
        (1, 48, 96, 9, 64, 32, 48),          # second concat source: ci0 > 0
        (0, 4 * 8, 16, up4_taps, 0, 0, 16),  # the parity-class tensor [4 Cout][Cin][3][3], forward
        (1, 4 * 8, 16, up4_taps, 0, 16, 32),  # ... and backward-data (cpad = 4 C of dY)
    ]


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_pack_jobs_hand_built_table(dtype, trainers):
    """(2a) one launch with ten jobs, each destination between its own guard bands; against pack_job and against the single-job entry
    points eod_pack_conv_weight / eod_pack_conv_weight_dgrad on the same weights"""
    taps = {int(wc.shape[2] * wc.shape[3]) for _, tr in trainers for _, wc in tr.up4_sums}
    assert len(taps) == 1, f"parity-class source tensors of the trainers: tap counts {taps}"
    specs = _hand_jobs(taps.pop())
    totals = [s[3] * (s[5] if s[0] else s[1]) * s[6] for s in specs]
    assert min(totals) < 256 and {4096, 4097, 3 * 4096 - 255} <= set(totals) and {s[3] for s in specs} >= {1, 9}
    r = Rng(11)
    jobs, outs, ws = [], [], []
    for kind, Cout, Cin, tp, ci0, nci, cpad in specs:
        w = r.randn((Cout, Cin, tp), 0.2)
        w.view(-1)[0] = 70000.0     # above the fp16 range
        w.view(-1)[-1] = -3e-8      # rounds to the smallest fp16 subnormal
        o = Out((tp, nci if kind else Cout, cpad), dtype)
        jobs.append(dict(w=_p(w), dst=o.ptr, kind=kind, Cout=Cout, Cin=Cin, taps=tp, ci0=ci0, nci=nci, cpad=cpad))
        outs.append(o)
        ws.append(w)
    got = twice(_launch_jobs(jobs, dtype), outs)
    L, st = _L(), _st()
    for j, w, g in zip(jobs, ws, got):
        geo = {k: v for k, v in j.items() if k not in ("w", "dst")}
        ref = R.pack_job(_np(w), dtype=NPT[dtype], **geo)
        assert _eq(g, ref), (geo, _first_diff(g, ref))
        single = Out(tuple(g.shape), dtype)
        ks = math.isqrt(j["taps"])
        if j["kind"] == 0:
            launch = lambda: _ok(L.eod_pack_conv_weight(_p(w), single.ptr, _dt(dtype), j["Cout"], j["Cin"], ks, j["cpad"], st), "pack_conv_weight")
        else:
            launch = lambda: _ok(L.eod_pack_conv_weight_dgrad(_p(w), single.ptr, _dt(dtype), j["Cout"], j["Cin"], ks, j["ci0"], j["nci"],
                                                              j["cpad"], st), "pack_conv_weight_dgrad")
        one, = twice(launch, [single])
        assert _eq(one, ref), ("single-job entry point", geo, _first_diff(one, ref))


UP4_CFG = dict(image_size=32, in_channels=13, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[], channel_mult=[1, 3],
               num_heads=1)  # a 96-channel Upsample conv on a 16 x 16 map: the parity-class form, forward and backward-data (fp16)


@pytest.fixture(scope="module")
def trainers():
    """small trainers, fp16 and fp32: u_a1_tiny (attention, concat sources), u_film_updown (resblock_updown) at batch 2, 16 x 16, and one
    whose Upsample conv runs in the parity-class form (32 x 32)"""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.training import UNetTrainer
    cfgs = unet_cfgs()
    out = []
    for name, cfg in (("u_a1_tiny", cfgs["u_a1_tiny"]), ("u_film_updown", cfgs["u_film_updown"]), ("up4", UP4_CFG)):
        for prec in ("fp16", "fp32"):
            torch.manual_seed(5)
            unet = UNetModel(**cfg).set_precision(prec).to(DEV).train()
            S = cfg["image_size"]
            out.append((f"{name} {prec}", UNetTrainer(unet, 2, S, S, DEV, loss_scale=(256.0 if prec == "fp16" else 1.0))))
    yield out
    out.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _at(cands, ptr, numel, dtype):
    """a tensor of `numel` elements at device address `ptr`, found inside the storage of one of the trainer's own tensors"""
    esize = torch.empty((), dtype=dtype).element_size()
    for t in cands:
        s = t.untyped_storage()
        if s.data_ptr() <= ptr and ptr + numel * esize <= s.data_ptr() + s.nbytes():
            return torch.empty(0, dtype=dtype, device=t.device).set_(s, (ptr - s.data_ptr()) // esize, (numel,))
    raise AssertionError(f"pack job pointer {ptr:#x} ({numel * esize} bytes) lies in no tensor of the trainer")


def _harvest(label, tr, seed):
    """overwrite every source weight of tr.pack_jobs in place, NaN-fill every destination, run the trainer's own launch (twice), compare
    each destination with pack_job of the NEW weights.  Returns the job geometries"""
    td = tr.prog.tdtype
    cands = [t for t in list(tr.prog.keep) + list(tr.bprog.keep) if isinstance(t, torch.Tensor)]
    cands += [p.data for p in tr.unet.parameters()] + [wc for _, wc in tr.up4_sums] + [vc.weight for vc in tr.virt]
    up4 = {wc.data_ptr() for _, wc in tr.up4_sums}
    r = Rng(seed)
    geos, srcs, dsts = [], {}, []
    assert tr.pack_jobs and len(tr.pack_jobs) == len({j.dst for j in tr.pack_jobs}), label
    for j in tr.pack_jobs:
        g = dict(kind=j.kind, Cout=j.Cout, Cin=j.Cin, taps=j.taps, ci0=j.ci0, nci=j.nci, cpad=j.cpad)
        if j.w not in srcs:
            srcs[j.w] = _at(cands, j.w, j.Cout * j.Cin * j.taps, F32)
            srcs[j.w].copy_(r.randn((j.Cout * j.Cin * j.taps,), 0.3))
        dsts.append(_at(cands, j.dst, _job_total(g), td))
        geos.append(dict(g, up4=j.w in up4))
    assert tr._pack_nblocks == sum(-(-_job_total(g) // _lib().PACK_CHUNK) for g in geos), label
    runs = []
    for _ in range(2):
        for d in dsts:
            d.fill_(float("nan"))
        tr._run_pack_jobs()
        torch.cuda.synchronize()
        runs.append([d.clone() for d in dsts])
    for j, g, a, b in zip(tr.pack_jobs, geos, *runs):
        ref = R.pack_job(_np(srcs[j.w]), dtype=NPT[td], **{k: v for k, v in g.items() if k != "up4"}).reshape(-1)
        assert _eq(a, ref), (label, g, _first_diff(a, ref))
        assert _eq(b, ref), (label, g, "second run")
    return geos


def test_edge_pack_jobs_of_real_trainers_refresh_every_destination(trainers):
    """(2b) every destination of every trainer's job list follows its source weights; and the ledger: the jobs the trainers really issue
    contain each feature the hand-built table is made of (a trainer change that moves re-packing elsewhere fails here)"""
    seen = {}
    for k, (label, tr) in enumerate(trainers):
        seen[label] = _harvest(label, tr, 100 + k)
        print(f"pack jobs {label}: {len(seen[label])} jobs, {tr._pack_nblocks} blocks")
    chunk = _lib().PACK_CHUNK
    for prec in ("fp16", "fp32"):
        gs = [g for label, v in seen.items() if label.endswith(prec) for g in v]
        assert {g["kind"] for g in gs} == {0, 1}, prec
        assert {g["taps"] for g in gs} >= {1, 9}, prec
        assert any(g["kind"] == 1 and g["ci0"] > 0 for g in gs), f"{prec}: the second concat source"
        assert any(g["kind"] == 0 and g["cpad"] > g["Cin"] for g in gs), f"{prec}: the first conv (input channels padded)"
        assert any(g["kind"] == 1 and g["cpad"] > g["Cout"] for g in gs), f"{prec}: the head conv (cout_pad > Cout)"
        assert any(_job_total(g) < chunk for g in gs), f"{prec}: a job below one chunk"
        assert any(_job_total(g) > chunk and _job_total(g) % chunk for g in gs), f"{prec}: a job that ends inside a chunk"
    f16 = [g for label, v in seen.items() if label.endswith("fp16") for g in v]
    assert any(g["up4"] and g["kind"] == 0 for g in f16) and any(g["up4"] and g["kind"] == 1 for g in f16), "the parity-class source tensors"


def test_edge_pack_dgrad_second_trip_of_the_grid_stride_loop():
    """(2c) eod_pack_conv_weight_dgrad beyond its 4096-block grid: 9 * 256 * 512 = 1 179 648 > 1 048 576 destination elements"""
    Cout, Cin, ci0, nci, cpad = 500, 300, 20, 256, 512
    w = Rng(13).randn((Cout, Cin, 9), 0.2)
    o = Out((9, nci, cpad), F16)
    got, = twice(lambda: _ok(_L().eod_pack_conv_weight_dgrad(_p(w), o.ptr, _dt(F16), Cout, Cin, 3, ci0, nci, cpad, _st()), "pack_dgrad"), [o])
    ref = R.pack_job(_np(w), 1, Cout, Cin, 9, ci0, nci, cpad, np.float16)
    assert _eq(got, ref), _first_diff(got, ref)


# ================================================================================================ 3. eod_dropout
KEYS = [  # (seed, layer, step)
    (1234, 0, 1),
    ((7 << 32) | 0x9abcdef1, 3, 2),                        # both key halves live
    (2 ** 63 - 1, 0x12345, 0x54321),                       # layer and step >= 2^16
    (0x5eadbeef12345678, 0xffffffff, 0x7fffffff),
]


def _drop(x, y, dtype, n, p, key):
    return lambda: _ok(_L().eod_dropout(_p(x), y.ptr, _dt(dtype), n, p, key[0], key[1], key[2], _st()), "dropout")


def _drop_input(r, n, dtype):
    x = r.randn((n,), 1.0, dtype)
    if n >= 5:
        x[0] = 65504.0 if dtype == F16 else FLT_MAX  # times 1 / keep: inf
        x[1] = -0.0
        x[2] = 6e-8 if dtype == F16 else 1e-40        # subnormal
    return x


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_dropout_output_and_mask(dtype, p):
    """the output of a random x (with the largest finite value, -0 and a subnormal in front) and the mask (x = ones), sizes around one
    draw of four and one block, keys with every field large"""
    r = Rng(21)
    for n in (1, 3, 4, 5, 1023, 1025, 4 * 256 * 3 + 2):
        x, ones, y = _drop_input(r, n, dtype), torch.ones((n,), dtype=dtype, device=DEV), Out((n,), dtype)
        xn = _np(x)
        for key in KEYS:
            got, = twice(_drop(x, y, dtype, n, p, key), [y])
            ref = R.dropout(xn, p, *key)
            assert _eq(got, ref), (n, p, key, _first_diff(got, ref))
            mask, = twice(_drop(ones, y, dtype, n, p, key), [y])
            keep = R.dropout_keep(n, p, *key)
            ref = np.where(keep, np.float32(1.0 / (1.0 - float(np.float32(p)))), np.float32(0)).astype(NPT[dtype])
            assert _eq(mask, ref), (n, p, key, "mask", _first_diff(mask, ref))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_dropout_draw_equal_to_the_threshold_is_dropped(dtype):
    """keep iff draw < threshold.  Below p = 2^-8 every integer is a threshold: p = k / 2^32 with k < 2^24 is a float32, 1 - p is exact in
    double, so the threshold is 2^32 - k.  k is chosen so that the threshold IS the draw of one element, and of the next larger and the
    next smaller draw in turn: the element at the threshold is dropped, the one below it kept (`<=` keeps both)"""
    n, key = 4099, KEYS[1]
    draws = R.dropout_draws(n, *key).astype(np.int64)
    cand = np.sort(draws[(draws > 2 ** 32 - 2 ** 24) & (draws < 2 ** 32 - 2 ** 23)])
    assert cand.size >= 3
    x, y = torch.full((n,), 3.0, dtype=dtype, device=DEV), Out((n,), dtype)
    for thr in cand[:3].tolist():
        p = float(np.float32((2 ** 32 - thr) / 2.0 ** 32))
        assert R.keep_threshold(p)[0] == thr
        got, = twice(_drop(x, y, dtype, n, p, key), [y])
        ref = R.dropout(_np(x), p, *key)
        at = int(np.nonzero(draws == thr)[0][0])
        assert ref[at] == 0 and (ref[draws < thr] != 0).all() and (ref[draws > thr] == 0).all()
        assert _eq(got, ref), (thr, at, _first_diff(got, ref))


def test_edge_dropout_second_trip_of_the_grid_stride_loop():
    n, p, key = 4 * 2097152 + 5, 0.25, KEYS[1]
    x, y = Rng(22).randn((n,), 1.0, F16), Out((n,), F16)
    got, = twice(_drop(x, y, F16, n, p, key), [y])
    ref = R.dropout(_np(x), p, *key)
    assert _eq(got, ref), _first_diff(got, ref)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_dropout_forward_op_and_backward_call_share_one_mask(dtype):
    """forward through the executor op (OP_DROPOUT, how UNetTrainer and the train-mode inference program reach the kernel: seed in an
    int64 slot, layer and step in int32 slots), backward through the direct call with the same key: one reference mask for both"""
    from eo_diffusion_amd.engine import Program
    n, p = 2 * 16 * 16 * 32 + 3, 0.3
    r = Rng(23)
    for key in [((9 << 32) | 77, 0x10001, 0x7fffffff), (1234, 5, 0x10000)]:
        x, g = _drop_input(r, n, dtype), r.randn((n,), 1.0, dtype)
        y, dx = Out((n,), dtype), Out((n,), dtype)
        prog = Program(DEV, "fp16" if dtype == F16 else "fp32")
        prog._small(_lib().OP_DROPOUT, p=(_p(x), y.ptr), l=(n, key[0]), i=(prog.dt, key[1], key[2]), f=(p,))
        fwd, = twice(lambda: prog.run(), [y])
        bwd, = twice(_drop(g, dx, dtype, n, p, key), [dx])
        keep = R.dropout_keep(n, p, *key)
        assert 0.6 < keep.mean() < 0.8
        assert _eq(fwd, R.dropout(_np(x), p, *key)), (key, "forward op")
        assert _eq(bwd, R.dropout(_np(g), p, *key)), (key, "backward call")
        gn, xn = _np(g), _np(x)
        assert np.array_equal(_np(bwd)[gn != 0] != 0, keep[gn != 0]) and np.array_equal(_np(fwd)[3:] != 0, keep[3:] & (xn[3:] != 0))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_dropout_p0_is_the_identity(dtype):
    """x comes back bit for bit, -0, subnormals and infinities included.  Regression: the fp16 kernel returned +0 for a kept -0 (the
    product and its rounding were one fused multiply-add with a +0 addend)"""
    r = Rng(24)
    for n in (1, 5, 1025, 4 * 256 * 3 + 2):
        x, y = _drop_input(r, n, dtype), Out((n,), dtype)
        if n >= 5:
            x[3], x[4] = float("inf"), float("-inf")
        for key in KEYS[:2]:
            got, = twice(_drop(x, y, dtype, n, 0.0, key), [y])
            assert _eq(got, _np(x)), (n, key)
            assert _eq(got, R.dropout(_np(x), 0.0, *key))


# ================================================================================================ 4. eod_add
def _add_inputs(r, n, dtype):
    a, b = r.randn((n,), 1.0, dtype), r.randn((n,), 1.0, dtype)
    sub = 6e-8 if dtype == F16 else 1e-40
    big = 60000.0 if dtype == F16 else 3e38
    inf = float("inf")
    pairs = [(inf, -inf), (big, big), (sub, sub), (0.0, -0.0), (-0.0, -0.0), (inf, 1.0), (-inf, -inf), (sub, -sub), (-big, -big), (3 * sub, -sub)]
    for k, (u, v) in enumerate(pairs[:n]):
        a[k], b[k] = u, v
    return a, b


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_add(dtype):
    epc = 16 // torch.empty((), dtype=dtype).element_size()
    r = Rng(31)
    for chunks in (1, 255, 256, 257, 1048576 + 3):   # one chunk; around one block; past the 4096-block grid
        n = chunks * epc
        a, b = _add_inputs(r, n, dtype)
        y = Out((n,), dtype)
        got, = twice(lambda: _ok(_L().eod_add(_p(a), _p(b), y.ptr, _dt(dtype), n, _st()), "add"), [y])
        with np.errstate(all="ignore"):
            ref = _np(a) + _np(b)
        assert ref.dtype == NPT[dtype] and _eq(got, ref), (chunks, _first_diff(got, ref))
        assert np.isnan(ref[0]) and np.isinf(ref[1])


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_edge_add_rejects_partial_chunks_and_unaligned_pointers(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    epc = 16 // es
    a, b = torch.ones((4 * epc,), dtype=dtype, device=DEV), torch.ones((4 * epc,), dtype=dtype, device=DEV)
    y = Out((4 * epc,), dtype)
    L, st, dt = _L(), _st(), _dt(dtype)
    for what, args in [("n not a whole number of chunks", (_p(a), _p(b), y.ptr, dt, 2 * epc - 1)), ("n = 0", (_p(a), _p(b), y.ptr, dt, 0)),
                       ("a unaligned", (_p(a) + es, _p(b), y.ptr, dt, 2 * epc)), ("b unaligned", (_p(a), _p(b) + es, y.ptr, dt, 2 * epc)),
                       ("y unaligned", (_p(a), _p(b), y.ptr + es, dt, 2 * epc))]:
        y.t.fill_(float("nan"))
        rc = L.eod_add(*args, st)
        torch.cuda.synchronize()
        assert rc != 0, what
        assert bool(y.t.isnan().all()) and y.g.intact(), what


# ================================================================================================ 5. eod_adamw_step, eod_ema_update
HP = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8)
BIG_N = 8192 * 256 + 257  # the grid is capped at 8192 blocks of 256 threads: the second trip of every grid-stride loop


def _opt_state(r, n):
    """p, m, v with +-0, a zero denominator candidate and subnormal second moments in front"""
    p, m, v = r.randn((n,)), r.randn((n,), 0.01), r.randn((n,), 1e-3).abs()
    for k, (a, b, c) in enumerate([(0.0, 0.0, 0.0), (-0.0, -0.0, 0.0), (1.0, 0.01, 1e-40), (-1.0, 0.0, 3e-39), (0.5, 1e-39, 0.0)][:n]):
        p[k], m[k], v[k] = a, b, c
    return p, m, v


def _grad(r, n, k):
    g = r.randn((n,), 0.05 * (1.0 + 0.3 * k))
    g[0] = 0.0           # with m = v = 0: the denominator is eps alone
    if n > 3:
        g[3] = 0.0
    if n > 5:
        g[5] = -0.0
    return g


@pytest.mark.parametrize("n", [1, 255, 257, BIG_N])
def test_edge_adamw_step(n):
    r = Rng(41)
    L, st = _L(), _st()
    P, M, V = Out((n,)), Out((n,)), Out((n,))
    for wd in (0.0, 0.01):
        for step0 in (1, 1000):   # bias corrections near 0 and near 1
            state = [_np(t) for t in _opt_state(r, n)]
            for k in range(4):
                g = _grad(r, n, k)
                cur = [_dev(s) for s in state]

                def prefill():
                    for o, s in zip((P, M, V), cur):
                        o.t.copy_(s)
                got = twice(lambda: _ok(L.eod_adamw_step(P.ptr, _p(g), M.ptr, V.ptr, n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd,
                                                         step0 + k, st), "adamw_step"), [P, M, V], prefill)
                ref = TR.adamw_step(state[0], _np(g), state[1], state[2], weight_decay=wd, step=step0 + k, **HP)
                for name, a, b in zip("pmv", got, ref):
                    assert _eq(a, b), (n, wd, step0 + k, name, _first_diff(a, b))
                state = list(ref)


@pytest.mark.parametrize("n", [1, 255, 257, BIG_N])
def test_edge_ema_update(n):
    r = Rng(42)
    A = Out((n,))
    for decay in (0.995, 0.0):
        avg0, p = r.randn((n,)), r.randn((n,))
        for k, (a, b) in enumerate([(0.0, -0.0), (-0.0, -0.0), (1e-40, 1e-40), (-0.0, 0.0), (1.0, 1e-39)][:n]):
            avg0[k], p[k] = a, b
        got, = twice(lambda: _ok(_L().eod_ema_update(A.ptr, _p(p), n, decay, _st()), "ema_update"), [A], prefill=lambda: A.t.copy_(avg0))
        ref = TR.ema_update(_np(avg0), _np(p), decay)
        assert _eq(got, ref), (n, decay, _first_diff(got, ref))


# ================================================================================================ 6. eod_adamw_step_guarded
class GuardedAdamW:
    """p / m / v, the 4-int state and the block-flag scratch of direct eod_adamw_step_guarded calls, every buffer between guard bands.
    Each call runs twice from the same state (bit-identical results required) and returns (before, after, state after)"""

    def __init__(self, n, scratch_len, seed, wd=0.01):
        self.n, self.slen, self.wd = n, scratch_len, wd
        r = Rng(seed)
        self.cur = list(_opt_state(r, n))
        self.state = torch.zeros((4,), dtype=I32, device=DEV)
        self.P, self.M, self.V = Out((n,)), Out((n,)), Out((n,))
        self.S, self.F = Out((4,), I32), Out((scratch_len,), I32)
        self.calls = 0

    def step(self, g):
        self.calls += 1
        L, st = _L(), _st()
        states = []

        def prefill():
            for o, s in zip((self.P, self.M, self.V), self.cur):
                o.t.copy_(s)
            self.S.t.copy_(self.state)
            self.F.t.fill_(1)   # a flag the detection kernel does not write reads as "not finite"

        def launch():
            _ok(L.eod_adamw_step_guarded(self.P.ptr, _p(g), self.M.ptr, self.V.ptr, self.n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], self.wd,
                                         self.calls, self.S.ptr, self.F.ptr, self.slen, st), "adamw_step_guarded")
            states.append(self.S.t.clone())
        got = twice(launch, [self.P, self.M, self.V], prefill)
        assert torch.equal(states[0], states[1]), "two runs of the same call leave different states"
        assert self.S.g.intact() and self.F.g.intact(), "write outside the state / the block flags"
        before = self.cur
        self.cur, self.state = [t.clone() for t in got], states[0]
        return before, got, [int(v) for v in states[0].cpu()]


def _bits_to_f32(i):
    return np.array([i], np.int32).view(np.float32)[0]


def _check_guarded_call(o, g, before, got, state, skip, skipped):
    """state[0] / state[1]; on an applied call the scalars within 1 ulp of host double and the update bit for bit given the device's
    scalars; on a skipped call p / m / v untouched.  Returns the device's two scalars (or None)"""
    assert state[0] == int(skip) and state[1] == skipped, (o.calls, state, skip, skipped)
    if skip:
        for name, a, b in zip("pmv", got, before):
            assert _eq(a, _np(b)), (o.calls, name, "a skipped call changed it")
        return None
    applied = o.calls - skipped
    dev = (_bits_to_f32(state[2]), _bits_to_f32(state[3]))
    for name, d, h in zip(("bc2_sqrt", "neg_step_size"), dev, R.host_scalars(HP["lr"], HP["beta1"], HP["beta2"], applied)):
        u = R.ulps32(d, np.float32(h))
        COUNT[name + " checked"] += 1
        COUNT[name + " exactly equal"] += int(u == 0)
        assert np.isfinite(d) and u <= 1, (name, o.calls, applied, float(d), h, u)
    ref = R.adamw_step_scalars(_np(before[0]), _np(g), _np(before[1]), _np(before[2]), 1.0 - HP["lr"] * o.wd, HP["beta1"], HP["beta2"], HP["eps"], *dev)
    for name, a, b in zip("pmv", got, ref):
        assert _eq(a, b), (o.calls, name, _first_diff(a, b))
    return dev


PATTERNS = [[1, 0, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 0, 1, 0, 0]]


@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: "".join("s" if s else "a" for s in p))
def test_edge_adamw_guarded_call_patterns(pattern):
    """the state machine over a run of calls (1 = this call's gradient holds a non-finite value): applied = calls - skipped"""
    n = 1000
    o = GuardedAdamW(n, 8192, seed=51)
    plain = [t.clone() for t in o.cur] if not any(pattern) else None   # the same run through eod_adamw_step
    r = Rng(52)
    skipped = 0
    bad = [float("inf"), float("nan"), float("-inf")]
    for k, skip in enumerate(pattern):
        g = _grad(r, n, k)
        if skip:
            g[(37 * k + 1) % n] = bad[k % 3]
        skipped += skip
        before, got, state = o.step(g)
        dev = _check_guarded_call(o, g, before, got, state, skip, skipped)
        if plain is not None:
            _ok(_L().eod_adamw_step(_p(plain[0]), _p(g), _p(plain[1]), _p(plain[2]), n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], o.wd,
                                    k + 1, _st()), "adamw_step")
            host = tuple(np.float32(h) for h in R.host_scalars(HP["lr"], HP["beta1"], HP["beta2"], k + 1))
            COUNT["all-applied steps"] += 1
            if all(R.ulps32(a, b) == 0 for a, b in zip(dev, host)):   # then the guarded step IS the plain step
                COUNT["all-applied steps with equal scalars"] += 1
                for name, a, b in zip("pmv", got, plain):
                    assert _eq(a, _np(b)), (k + 1, name, "guarded and plain AdamW differ with equal scalars")
            else:   # one scalar differs in its last bit: continue the plain run from the guarded state
                plain = [t.clone() for t in got]
    print("guarded AdamW:", dict(COUNT))


def _set_bits(g, idx, bits):
    g.view(I32)[idx] = bits
    return g


@pytest.mark.parametrize("scratch_len", [1, 3])
def test_edge_adamw_guarded_detects_one_bad_value_anywhere(scratch_len):
    """one +inf / -inf / quiet NaN / negative NaN at index 0, at n - 1, and at an index only the SECOND trip of the detection kernel's
    grid-stride loop reads (scratch_len blocks of 256 threads over n = 2000)"""
    n = 2000
    r = Rng(53)
    second_trip = scratch_len * 256 + 5
    for bits in (0x7f800000, -0x00800000, 0x7fc00000, -0x00400000):   # +inf, -inf (0xff800000), NaN, -NaN (0xffc00000)
        for idx in (0, n - 1, second_trip):
            o = GuardedAdamW(n, scratch_len, seed=54)
            g = _set_bits(_grad(r, n, 0), idx, bits)
            assert not bool(torch.isfinite(g[idx]))
            before, got, state = o.step(g)
            _check_guarded_call(o, g, before, got, state, 1, 1)
    o = GuardedAdamW(n, scratch_len, seed=55)   # and the call after a skipped first call is the FIRST applied step
    g = _grad(r, n, 0)
    g[n - 1] = float("inf")
    _check_guarded_call(o, g, *o.step(g), 1, 1)
    g = _grad(r, n, 1)
    dev = _check_guarded_call(o, g, *o.step(g), 0, 1)
    assert R.ulps32(dev[1], np.float32(-HP["lr"] / (1.0 - HP["beta1"]))) <= 1


@pytest.mark.parametrize("scratch_len", [1, 3, 8192])
def test_edge_adamw_guarded_does_not_flag_finite_extremes(scratch_len):
    n = 2000
    r = Rng(56)
    o = GuardedAdamW(n, scratch_len, seed=57)
    g = _grad(r, n, 0)
    for k, v in enumerate([FLT_MAX, -FLT_MAX, 1e-40, -1e-45, 1.1754944e-38]):
        g[k * 397 + 1] = v
    g[n - 1] = -FLT_MAX
    _check_guarded_call(o, g, *o.step(g), 0, 0)


def test_edge_adamw_guarded_second_trip_of_the_grid_stride_loops():
    """n past the 8192-block grid: a bad value in the LAST element is seen, and an applied step updates every element"""
    n = BIG_N
    o = GuardedAdamW(n, 8192, seed=58, wd=0.0)
    r = Rng(59)
    g = _grad(r, n, 0)
    g[n - 1] = float("nan")
    _check_guarded_call(o, g, *o.step(g), 1, 1)
    g[n - 1] = 0.25
    _check_guarded_call(o, g, *o.step(g), 0, 1)
    print("guarded AdamW:", dict(COUNT))


# ================================================================================================ 7. ledger of one whole training step
PINNED_HERE = {
    "eod_pack_jobs": "test_edge_pack_jobs_hand_built_table",
    "eod_dropout": "test_edge_dropout_output_and_mask",
    "eod_add": "test_edge_add",
    "eod_adamw_step": "test_edge_adamw_step",
    "eod_adamw_step_guarded": "test_edge_adamw_guarded_call_patterns",
    "eod_ema_update": "test_edge_ema_update",
}
PINNED_ELSEWHERE = {  # launches outside the SPECS table of tests/test_gpu_train_kernels.py: (module, test)
    "eod_program_run": ("tests.test_gpu_conv_programs", "test_harvest_is_complete"),   # the executor: its op kinds have ledgers of their own,
    #   ... tests.test_gpu_glue_ops::test_edge_every_glue_op_kind_of_a_program_is_pinned_here and the attention ledger below
    "eod_rowdot": ("tests.test_gpu_attention", "test_edge_every_attention_launch_of_the_real_programs_is_pinned_here"),
    "eod_attention_bwd": ("tests.test_gpu_attention", "test_edge_every_attention_launch_of_the_real_programs_is_pinned_here"),
    "eod_softmax_bwd_rows": ("tests.test_gpu_attention", "test_edge_every_attention_launch_of_the_real_programs_is_pinned_here"),
    "eod_scale_f32": ("tests.test_gpu_attention", "test_edge_scale_f32"),
    "eod_mse_loss": ("tests.test_gpu_train_kernels", "test_edge_mse_loss"),
    "eod_gn_partial": ("tests.test_gpu_glue_ops", "test_edge_group_norm_slab_and_channel_block_edges"),
    "eod_conv_up4_weights": ("tests.test_gpu_conv_programs", "test_pack_dgrad_of_the_class_kernel_tensor_is_the_upsample4_weight"),
}
NO_LAUNCH = {"eod_last_error", "eod_version", "eod_struct_size", "eod_get_option", "eod_gn_bwd_apply_slabs"}   # host-side queries


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_edge_every_launch_of_a_training_step_is_pinned_somewhere(prec, monkeypatch):
    """a trainer with dropout, optim.AdamW and ExponentialMovingAverage: every C-ABI function that two full steps (forward -> mse_loss ->
    backward -> step -> update_parameters) call is pinned by this module, by the SPECS table of tests/test_gpu_train_kernels.py, or by
    the named test of another module"""
    import importlib
    import sys
    from eo_diffusion_amd import optim
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.training import UNetTrainer
    from tests import test_gpu_train_kernels as TK
    for name, test in PINNED_HERE.items():
        assert callable(getattr(sys.modules[__name__], test)), (name, test)
    for name, (mod, test) in PINNED_ELSEWHERE.items():
        assert callable(getattr(importlib.import_module(mod), test)), (name, mod, test)
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
    torch.manual_seed(7)
    cfg = dict(unet_cfgs()["u_a1_tiny"], dropout=0.1)
    S = cfg["image_size"]
    unet = UNetModel(**cfg).set_precision(prec).to(DEV).train()
    ema = optim.ExponentialMovingAverage(unet, decay=0.99, device=DEV)
    opt = optim.AdamW(unet.parameters(), lr=1e-3)
    tr = UNetTrainer(unet, 2, S, S, DEV, loss_scale=(256.0 if prec == "fp16" else 1.0), dropout_seed=99)
    called.clear()   # (construction asks the library about geometries and packs once: not part of a step)
    r = Rng(61)
    for _ in range(2):   # (the first update_parameters copies, the second one runs the kernel)
        x, noise, t = r.randn((2, 3, S, S)), r.randn((2, 3, S, S)), torch.tensor([7, 650], device=DEV)
        pred = tr.forward(x, t)
        loss, dpred = optim.mse_loss(pred, noise)
        tr.backward(dpred)
        opt.step()
        ema.update_parameters(unet)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    names = {n for n in called if n.startswith("eod_")} - NO_LAUNCH
    print(f"LEDGER step {prec}:", dict(sorted(called.items())))
    unpinned = sorted(n for n in names if n not in PINNED_HERE and n not in TK.SPECS and n not in PINNED_ELSEWHERE)
    assert not unpinned, f"launched by a training step and pinned nowhere: {unpinned}"
    for n in ("eod_pack_jobs", "eod_dropout", "eod_add", "eod_adamw_step_guarded", "eod_ema_update", "eod_program_run", "eod_mse_loss"):
        assert called[n] >= 1, f"the step does not call {n}: the ledger does not see it"
    del tr, opt, ema, unet
    gc.collect()
    torch.cuda.empty_cache()
