"""conv_plan() (csrc/igemm.hip) is the one place that decides which kernel a conv descriptor gets; the geometry queries and
eod_conv_kernel_name only read it.  tests/golden/conv_plan_table.npz records, for a fixed seeded set of (descriptor, option arm) pairs, what
the library answered BEFORE the decisions were gathered into the plan: the seven queries, and the kernel family its dispatcher launched
(taken from a launch trace of eod_conv2d_igemm; -1 where it rejected the descriptor).  The library must still give the same answers, and
eod_conv_kernel_name must name the family that was launched.

    python -m tests.test_conv_plan --record     regenerates the fixture against the library that is loaded (family = eod_conv_kernel_name)
"""
import ctypes as C
import os
import random
import sys

import numpy as np

from eo_diffusion_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.npz")
FAMILIES = ("conv3x3_halo_kernel", "conv3x3_halo_kernel<BN=32>", "conv_up4_halo_kernel", "conv_s2_halo_kernel", "conv_first_x3_kernel",
            "conv_head_kernel", "igemm_kernel")
QUERIES = ("eod_conv_workspace_size", "eod_conv_stats_slots", "eod_conv_gn_fusable", "eod_conv_skip_ok", "eod_conv_split_ok",
           "eod_conv_up4_ok", "eod_conv_up4_bwd_ok")
# the default options, then each of the eight options flipped in turn (the head's tile-run option at 1 and 4)
ARMS = ((None, 0), ("skip_fuse", 0), ("head", 0), ("halo_bn256", 0), ("gn_fuse_max_cout", 128), ("gn_fuse_max_cout", 1024), ("halo_splitk", 0),
        ("first", 0), ("head_tpw", 1), ("head_tpw", 4), ("s2_halo", 0))

# ---- the descriptor grid ----
STORAGE = ("fp16", "fp32x3", "fp32")
BATCH = (1, 2, 16)
MAPS = ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (16, 8), (24, 24), (40, 56))
COUT = (3, 16, 32, 64, 128, 192, 256, 384, 512, 640)
CIN = ((64, 0), (128, 0), (256, 128), (512, 0), (512, 512))
FORM = ((3, 1, 1, 0), (3, 2, 1, 0), (3, 2, 0, 1), (1, 1, 0, 0))  # (ksize, stride, pad, pad_tl)
UPSAMPLE = (0, 1, 2, 3, 4)
FLAGS = ("gn", "skip1", "skip2", "stats", "nchw", "tap4", "tap8", "tap16", "x_presplit", "y_presplit", "res", "cbias", "no_workspace")
N_RANDOM, SEED = 355, 20260


def _row(storage, n, hw, cout, cin, form=FORM[0], ups=0, flags=()):
    return dict(storage=storage, N=n, H=hw[0], W=hw[1], Cout=cout, C0=cin[0], C1=cin[1], form=form, ups=ups, flags=tuple(flags))


# one descriptor per family and per column width, both split-K paths, the 256 + 128 form, an 8-wide and a ragged map (the layers of the
# 256 x 256 and 64 x 64 UNets that take them), ahead of the seeded sample of the grid
NAMED = [
    _row("fp32x3", 16, (256, 256), 128, (128, 0), flags=("gn", "stats")),           # halo, 128 columns
    _row("fp32x3", 16, (64, 64), 256, (256, 0), flags=("gn",)),                      # halo, 256 columns
    _row("fp32x3", 16, (64, 64), 384, (256, 128), flags=("gn", "stats")),            # halo, 256 + 128
    _row("fp32x3", 16, (64, 64), 256, (128, 0), flags=("skip1",)),                   # halo, 256 columns, fused skip
    _row("fp16", 16, (64, 64), 256, (256, 0), flags=("gn", "skip2")),
    _row("fp16", 16, (64, 64), 256, (256, 0)),                                       # fp16 without GroupNorm: never 256 columns
    _row("fp32", 16, (64, 64), 256, (256, 0), flags=("gn",)),                        # exact fp32: 128 columns only
    _row("fp32x3", 16, (16, 16), 128, (64, 0), flags=("gn",)),                       # halo, 64 columns
    _row("fp32x3", 16, (16, 16), 384, (512, 0), flags=("gn", "stats")),              # halo, K slices
    _row("fp16", 2, (16, 8), 512, (512, 0), flags=("skip2", "stats")),               # 8-wide map, K slices + skip phase
    _row("fp32x3", 2, (8, 8), 512, (512, 0), flags=("gn",)),
    _row("fp16", 16, (32, 32), 256, (256, 128), ups=1),                              # halo, virtual nearest-2x
    _row("fp32x3", 16, (64, 64), 3, (128, 0), flags=("gn", "nchw")),                 # head kernel
    _row("fp32", 16, (64, 64), 3, (128, 0), flags=("gn", "nchw")),                   # exact fp32 head: 32-column halo instance
    _row("fp16", 16, (64, 64), 32, (64, 0), flags=("nchw",)),
    _row("fp32x3", 16, (256, 256), 128, (64, 0), flags=("tap8",)),                   # first conv
    _row("fp16", 16, (256, 256), 128, (64, 0), flags=("tap8",)),                     # ... fp16: generic kernel, tap-major
    _row("fp32x3", 16, (128, 128), 256, (256, 0), form=FORM[1], flags=("stats",)),   # stride-2 halo kernel
    _row("fp32x3", 16, (16, 16), 512, (512, 0), form=FORM[1]),                       # stride 2 on a small map: generic kernel, split K
    _row("fp16", 16, (32, 32), 256, (256, 0), ups=3, flags=("stats",)),              # parity-class upsample conv
    _row("fp16", 16, (64, 64), 256, (256, 0), ups=4),                                # ... and its backward-data
    _row("fp16", 2, (32, 32), 128, (128, 0), ups=2),                                 # zero insertion: four parity launches
    _row("fp32x3", 16, (64, 64), 512, (256, 0), form=FORM[3], flags=("y_presplit",)),  # qkv 1x1: 256 columns, direct
    _row("fp32x3", 16, (16, 16), 256, (256, 0), form=FORM[3], flags=("x_presplit",)),               # proj 1x1
    _row("fp32x3", 2, (24, 24), 192, (256, 128), flags=("res",)),                    # ragged map: generic kernel
    _row("fp16", 1, (40, 56), 64, (128, 0), form=FORM[2], flags=("res", "cbias")),
    _row("fp32", 2, (4, 4), 16, (512, 512), form=FORM[3]),
]


def rows():
    """the committed subset: the named descriptors, then N_RANDOM seeded draws"""
    rng = random.Random(SEED)
    return NAMED + [draw(rng, k) for k in range(N_RANDOM)]


def draw(rng, k):
    """draw k of a stream: a point of the product of the axes with 0 - 2 flags; every fourth one a 3x3 / stride 1 conv with a pair of the
    flags that choose among the halo instances (uniform draws almost never meet a fused GroupNorm AND a fused skip on a map that tiles)"""
    r = _row(rng.choice(STORAGE), rng.choice(BATCH), rng.choice(MAPS), rng.choice(COUT), rng.choice(CIN), rng.choice(FORM),
             rng.choice(UPSAMPLE), rng.sample(FLAGS, rng.choice((0, 1, 2, 2))))
    if k % 4 == 3:
        r.update(form=FORM[0], ups=0, flags=tuple(rng.sample(("gn", "skip1", "skip2", "nchw", "stats"), 2)))
    return r


def bind(L):
    for q in QUERIES:
        getattr(L, q).restype, getattr(L, q).argtypes = (C.c_int64 if q == "eod_conv_workspace_size" else C.c_int32), [C.POINTER(_lib.ConvDesc)]
    L.eod_set_option.restype, L.eod_set_option.argtypes = C.c_int32, [C.c_char_p, C.c_int32]
    if hasattr(L, "eod_conv_kernel_name"):
        L.eod_conv_kernel_name.restype, L.eod_conv_kernel_name.argtypes = C.c_char_p, [C.POINTER(_lib.ConvDesc)]
    return L


def make_desc(L, r):
    """the descriptor of a grid row, with fixed fake 16-byte-aligned pointers; stats_slots and the workspace as a caller sizes them, from
    the library's own queries under the current options"""
    ptr = lambda k: 0x10000000 + 0x1000000 * k
    f = set(r["flags"])
    d = _lib.ConvDesc()
    ks, stride, pad, pad_tl = r["form"]
    d.dtype = _lib.EOD_F16 if r["storage"] == "fp16" else _lib.EOD_F32
    d.N, d.H, d.W, d.C0, d.C1, d.Cout = r["N"], r["H"], r["W"], r["C0"], r["C1"], r["Cout"]
    d.ksize, d.stride, d.pad, d.pad_tl, d.upsample, d.alpha = ks, stride, pad, pad_tl, r["ups"], 1.0
    for t in (4, 8, 16):
        if f"tap{t}" in f:
            d.w_tapmajor, d.C0, d.C1 = 1, t, 0
    up = 2 if r["ups"] in (1, 2, 3) else 1
    if r["ups"] == 4:
        d.Ho, d.Wo = d.H // 2, d.W // 2
    else:
        d.Ho, d.Wo = ((d.H * up + pad_tl + 2 * pad - ks) // stride + 1, (d.W * up + pad_tl + 2 * pad - ks) // stride + 1)
    d.x, d.w, d.y, d.bias = ptr(1), ptr(2), ptr(3), ptr(4)
    if d.C1:
        d.x2 = ptr(5)
    if r["storage"] == "fp32x3":
        d.w_split, d.w_scale, d.a_bound = 1, ptr(6), ptr(7)
    if "gn" in f:
        d.gn_scale_shift, d.gn_silu = ptr(8), 1
    if "skip1" in f or "skip2" in f:
        d.skip_x, d.skip_w, d.skip_C0, d.skip_bound = ptr(9), ptr(10), 128, ptr(11)
        if "skip2" in f:
            d.skip_x2, d.skip_C0, d.skip_C1 = ptr(12), 256, 128
    if "nchw" in f:
        d.out_nchw_f32 = 1
    if "x_presplit" in f:
        d.x_presplit = 1
    if "y_presplit" in f:
        d.y_presplit_bound = ptr(13)
    if "res" in f:
        d.res = ptr(14)
    if "cbias" in f:
        d.cbias, d.cbias_stride = ptr(15), d.Cout
    if "stats" in f:
        d.stats, d.stats_slots = ptr(16), L.eod_conv_stats_slots(C.byref(d))
    if "no_workspace" not in f:
        d.workspace, d.workspace_bytes = ptr(17), L.eod_conv_workspace_size(C.byref(d))
    return d


class arm:
    """one option set to a value for the duration of a with block"""

    def __init__(self, L, a):
        self.L, self.name, self.value = L, a[0], a[1]

    def __enter__(self):
        if self.name:
            self.prev = self.L.eod_set_option(self.name.encode(), self.value)

    def __exit__(self, *exc):
        if self.name:
            self.L.eod_set_option(self.name.encode(), self.prev)


def answers(L, row_list, family_of):
    """(queries [pairs][7] int64, family [pairs] int8) over row_list x ARMS, arm-major"""
    q, fam = [], []
    for a in ARMS:
        with arm(L, a):
            for r in row_list:
                d = make_desc(L, r)
                q.append([int(getattr(L, name)(C.byref(d))) for name in QUERIES])
                fam.append(family_of(d))
    return np.asarray(q, np.int64), np.asarray(fam, np.int8)


def named_family(L):
    return lambda d: FAMILIES.index(L.eod_conv_kernel_name(C.byref(d)).decode())


def test_fixture_covers_the_grid():
    tab = np.load(GOLDEN)
    n = len(rows()) * len(ARMS)
    assert n >= 4200 and tab["queries"].shape == (n, len(QUERIES)) and tab["family"].shape == (n,)
    assert set(range(len(FAMILIES))) <= set(tab["family"].tolist())  # every family was launched at least once
    assert (tab["queries"][:, 0] > 0).any() and (tab["queries"][:, 1] > 0).any()
    for col in range(2, len(QUERIES)):
        assert set(tab["queries"][:, col].tolist()) == {0, 1}


def test_plan_gives_the_recorded_answers():
    L = bind(_lib.lib())
    tab = np.load(GOLDEN)
    q, fam = answers(L, rows(), named_family(L))
    for col, name in enumerate(QUERIES):
        bad = np.nonzero(q[:, col] != tab["queries"][:, col])[0]
        assert bad.size == 0, (name, bad[:10].tolist())
    launched = tab["family"] >= 0  # (a rejected descriptor launches nothing: no family to compare)
    bad = np.nonzero(launched & (fam != tab["family"]))[0]
    assert bad.size == 0, [(int(i), FAMILIES[fam[i]], FAMILIES[tab["family"][i]]) for i in bad[:10]]


def test_kernel_name_follows_the_options():
    L = bind(_lib.lib())
    name = lambda r: L.eod_conv_kernel_name(C.byref(make_desc(L, r))).decode()
    head, first, s2 = NAMED[12], NAMED[15], NAMED[17]
    assert (name(head), name(first), name(s2)) == ("conv_head_kernel", "conv_first_x3_kernel", "conv_s2_halo_kernel")
    for r, option, other in ((head, "head", "conv3x3_halo_kernel<BN=32>"), (first, "first", "igemm_kernel"), (s2, "s2_halo", "igemm_kernel")):
        with arm(L, (option, 0)):
            assert name(r) == other
        assert name(r) != other  # (and the option is back)


def test_the_removed_halo_tpw_option_is_an_unknown_name():
    """the streaming form of the 3x3 halo kernel and its option are gone: the name takes the unknown-option refusal, for set and for get"""
    L = bind(_lib.lib())
    L.eod_get_option.restype, L.eod_get_option.argtypes = C.c_int32, [C.c_char_p]
    EOD_EINVAL = -1  # (include/eodiff.h)
    assert L.eod_set_option(b"halo_tpw", 2) == EOD_EINVAL
    assert L.eod_get_option(b"halo_tpw") == EOD_EINVAL
    assert L.eod_get_option(b"head_tpw") == 0  # (a name that stays answers with its value)


if __name__ == "__main__":
    if "--record" in sys.argv:
        lib = bind(_lib.lib())
        queries, family = answers(lib, rows(), named_family(lib))
        np.savez_compressed(GOLDEN, queries=queries, family=family)
        print(f"{GOLDEN}: {len(family)} pairs")
