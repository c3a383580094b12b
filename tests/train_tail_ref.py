"""TEST INFRASTRUCTURE: plain numpy references for the tail of the training step -- the one-launch weight re-pack (eod_pack_jobs), dropout
(eod_dropout), and the AdamW update with its two step-dependent scalars passed in (eod_adamw_step_guarded computes them on the device).
No GPU; checked on their own in tests/test_train_tail_ref.py, used by tests/test_gpu_train_tail.py.

Every function restates a documented layout or formula, not a kernel's index arithmetic:
  pack_job   the layout comments of csrc/train.hip: kind 0 [tap][Cout][cpad], kind 1 [taps-1-tap][ci - ci0][cpad]
  dropout    nn.Dropout with a Philox4x32-10 mask (oracle/philox_ref.py), one draw of four words per four elements
  adamw_step_scalars   oracle/train_ref.adamw_step with sqrt(1 - beta2^step) and -lr / (1 - beta1^step) given as float32"""
import math

import numpy as np

from oracle.philox_ref import _philox

f32 = np.float32


def pack_job(w, kind, Cout, Cin, taps, ci0, nci, cpad, dtype):
    """w: fp32 OIHW weight with Cout * Cin * taps values.  Returns the packed destination [taps][rows][cpad] in `dtype`:
    kind 0 (forward):        dst[t][co][c] = w[co][c][t]               for c < Cin,  else 0   (rows = Cout)
    kind 1 (backward-data):  dst[t][m][c]  = w[c][ci0 + m][taps-1-t]   for c < Cout, else 0   (rows = nci)"""
    w = np.asarray(w, f32).reshape(Cout, Cin, taps)
    rows = nci if kind else Cout
    dst = np.zeros((taps, rows, cpad), f32)
    for t in range(taps):
        for m in range(rows):
            if kind == 0:
                dst[t, m, :Cin] = w[m, :, t]
            else:
                dst[t, m, :Cout] = w[:, ci0 + m, taps - 1 - t]
    with np.errstate(over="ignore"):  # (a weight beyond the fp16 range becomes inf, as in the kernel's conversion)
        return dst.astype(dtype)


def keep_threshold(p):
    """(threshold on a 32-bit draw, keep probability): keep iff draw < threshold"""
    keep = 1.0 - float(f32(p))
    return (0xFFFFFFFF if keep >= 1.0 else int(math.floor(keep * 2.0 ** 32))), keep


def dropout_draws(n, seed, layer, step):
    """the 32-bit draw of each of n elements: word (e % 4) of Philox4x32-10 with counter (q & 0xffffffff, q >> 32, layer, step), q = e // 4,
    key = the two halves of the 64-bit seed"""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = _philox((q & np.uint64(0xFFFFFFFF)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32), np.uint32(layer), np.uint32(step),
                    seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([np.broadcast_to(c, q.shape) for c in words], 1).reshape(-1)[:n]


def dropout_keep(n, p, seed, layer, step):
    """boolean keep mask of n elements"""
    thr, _ = keep_threshold(p)
    return dropout_draws(n, seed, layer, step) < np.uint32(thr)


def dropout(x, p, seed, layer, step):
    """y = fl32(fl32(x) * fl32(1 / keep)) where kept, +0 elsewhere, rounded to x's storage type"""
    x = np.asarray(x)
    _, keep = keep_threshold(p)
    k = dropout_keep(x.size, p, seed, layer, step).reshape(x.shape)
    with np.errstate(over="ignore"):
        y = x.astype(f32) * f32(1.0 / keep)
        return np.where(k, y, f32(0.0)).astype(x.dtype)


def adamw_step_scalars(p, g, m, v, decay_mul, beta1, beta2, eps, bc2_sqrt, neg_step_size):
    """torch.optim.AdamW's single-tensor update (oracle/train_ref.adamw_step), every operation rounded to float32, with
    decay_mul = 1 - lr * weight_decay, bc2_sqrt = sqrt(1 - beta2^step) and neg_step_size = -lr / (1 - beta1^step) given by the caller
    (rounded to float32 here)"""
    p, g, m, v = (np.asarray(a).astype(f32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        p = p * f32(decay_mul)
        m = m * f32(beta1) + g * f32(1.0 - beta1)
        v = v * f32(beta2) + (f32(1.0 - beta2) * g) * g
        denom = np.sqrt(v) / f32(bc2_sqrt) + f32(eps)
        p = p + f32(neg_step_size) * (m / denom)
    return p.astype(f32), m.astype(f32), v.astype(f32)


def host_scalars(lr, beta1, beta2, applied):
    """(sqrt(1 - beta2^a), -lr / (1 - beta1^a)) in host double for a applied steps"""
    return math.sqrt(1.0 - beta2 ** applied), -(lr / (1.0 - beta1 ** applied))


def ulps32(a, b):
    """distance of two float32 values of the same sign in units of the last place"""
    ia, ib = (int(np.asarray(x, f32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)
