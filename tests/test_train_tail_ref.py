"""CPU: the numpy references of tests/train_tail_ref.py on their own -- Philox against the Random123 known answers, the pack layouts
against torch's permute / flip / pad, the AdamW restatement against oracle/train_ref.py, and the statistics of the dropout mask."""
import math

import numpy as np
import pytest
import torch

from oracle import train_ref as TR
from oracle.philox_ref import _philox
from tests import train_tail_ref as R


# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, result)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = _philox(*(np.array([c], np.uint32) for c in ctr), *key)
    assert tuple(int(g[0]) for g in got) == want


def test_dropout_draws_are_the_philox_words_in_order():
    """element e takes word e % 4 of the draw with counter (e // 4, 0, layer, step) and the seed halves as the key"""
    seed, layer, step = (0x299f31d0 << 32) | 0xa4093822, 0x13198a2e, 0x03707344
    d = R.dropout_draws(11, seed, layer, step)
    for e in range(11):
        w = _philox(np.array([e // 4], np.uint32), np.array([0], np.uint32), np.array([layer], np.uint32), np.array([step], np.uint32),
                    0xa4093822, 0x299f31d0)
        assert int(d[e]) == int(w[e % 4][0])


def _torch_pack(w, kind, ci0, nci, cpad):
    """the obvious expression: w [Cout][Cin][kh][kw]"""
    Cout, Cin = w.shape[:2]
    w3 = w.reshape(Cout, Cin, -1)
    if kind == 0:
        return torch.nn.functional.pad(w3.permute(2, 0, 1), (0, cpad - Cin))
    return torch.nn.functional.pad(w3[:, ci0:ci0 + nci].flip(2).permute(2, 1, 0), (0, cpad - Cout))


@pytest.mark.parametrize("Cout,Cin,ks,ci0,nci,cpad0,cpad1", [(5, 3, 3, 1, 2, 8, 8), (8, 13, 3, 4, 7, 16, 8), (6, 10, 1, 3, 5, 12, 9)])
def test_pack_job_against_permute_flip_pad(Cout, Cin, ks, ci0, nci, cpad0, cpad1):
    g = torch.Generator().manual_seed(Cout * 100 + Cin)
    w = torch.randn((Cout, Cin, ks, ks), generator=g)
    for dtype in (np.float32, np.float16):
        got0 = R.pack_job(w.numpy(), 0, Cout, Cin, ks * ks, 0, 0, cpad0, dtype)
        got1 = R.pack_job(w.numpy(), 1, Cout, Cin, ks * ks, ci0, nci, cpad1, dtype)
        assert got0.dtype == dtype and got0.shape == (ks * ks, Cout, cpad0) and got1.shape == (ks * ks, nci, cpad1)
        assert np.array_equal(got0, _torch_pack(w, 0, 0, 0, cpad0).numpy().astype(dtype))
        assert np.array_equal(got1, _torch_pack(w, 1, ci0, nci, cpad1).numpy().astype(dtype))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw_step_scalars_equals_train_ref_with_the_host_scalars(wd, step):
    r = np.random.default_rng(step)
    n = 4099
    p, g, m, v = (r.standard_normal(n).astype(np.float32) * s for s in (1.0, 0.05, 0.01, 1.0))
    v = np.abs(v) * np.float32(1e-3)
    g[:7] = 0.0
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    want = TR.adamw_step(p, g, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, step=step)
    bc2_sqrt, nss = R.host_scalars(lr, b1, b2, step)
    got = R.adamw_step_scalars(p, g, m, v, 1.0 - lr * wd, b1, b2, eps, bc2_sqrt, nss)
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a), _bits(b))


def test_ulps32():
    assert R.ulps32(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert R.ulps32(-0.5, -0.5) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_dropout_p0_is_the_identity(dtype):
    r = np.random.default_rng(3)
    x = r.standard_normal(4099).astype(dtype)
    x[:4] = [0.0, -0.0, np.inf, 6e-8]
    y = R.dropout(x, 0.0, 77, 3, 9)
    assert y.dtype == x.dtype and x.tobytes() == y.tobytes()
    assert R.keep_threshold(0.0) == (0xFFFFFFFF, 1.0)


def test_dropout_threshold_and_scale():
    thr, keep = R.keep_threshold(0.25)
    assert thr == 3 << 30 and keep == 0.75
    thr, keep = R.keep_threshold(0.1)  # p is a float32 on the C ABI: 0.1f = 0.100000001490116...
    assert keep == 1.0 - float(np.float32(0.1)) and thr == math.floor(keep * 2.0 ** 32)
    x = np.full(64, 3.0, np.float16)
    y = R.dropout(x, 0.25, 5, 0, 1)
    assert set(np.unique(y).tolist()) == {0.0, 4.0}


AGREE_N = 1 << 18


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_dropout_masks_of_different_keys_are_independent(p):
    """Two independent Bernoulli(keep) masks agree on an element with probability a = keep^2 + p^2, so over n elements the agreeing share
    is binomial with standard deviation sqrt(a (1 - a) / n) <= 0.5 / sqrt(n) = 9.8e-4 at n = 2^18; the band is 5 of those (a 6e-7 event
    per comparison for a true random source).  The keep rate itself has sqrt(keep p / n) and gets the same 5.
    Observed on the CPU reference (worst of the five comparisons per p, in standard deviations): p = 0.1: 1.61 (share within 0.0013 of
    0.82), p = 0.25: 1.55, p = 0.5: 1.33; keep rate: 0.75 / 0.16 / 0.64.  A key / counter mix-up that made two of these keys equal would
    give a share of 1."""
    base = (0x1234567 | (5 << 32), 3, 7)
    others = [((base[0] ^ 1), 3, 7), ((base[0] ^ (1 << 32)), 3, 7), (base[0], 4, 7), (base[0], 3, 8), (base[0], 7, 3)]
    m0 = R.dropout_keep(AGREE_N, p, *base)
    keep = 1.0 - float(np.float32(p))
    ksd = math.sqrt(keep * (1 - keep) / AGREE_N)
    print(f"dropout keep rate p={p}: {m0.mean():.5f}, {abs(m0.mean() - keep) / ksd:.2f} sd from {keep:.5f}")
    assert abs(m0.mean() - keep) < 5 * ksd
    a = keep * keep + (1 - keep) ** 2
    sd = math.sqrt(a * (1 - a) / AGREE_N)
    worst = 0.0
    for k in others:
        m1 = R.dropout_keep(AGREE_N, p, *k)
        share = float((m0 == m1).mean())
        worst = max(worst, abs(share - a) / sd)
        assert abs(share - a) < 5 * sd, (p, k, share, a, sd)
    print(f"dropout agreement p={p}: worst deviation {worst:.2f} sd (share a={a:.4f}, sd={sd:.2e})")
