"""CPU suite: the RePaint resampling schedule (eo_diffusion_amd/diffusion/util.py make_resample_schedule; host, integer, exact) and the
fp32 coefficients of the forward move x_a -> x_b that eod_renoise applies, held to float64."""
import numpy as np
import pytest

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.util import make_resample_schedule
from tests import repaint_ref as RR

SWEEP = [(n, L, U) for n in range(1, 25) for L in range(1, 9) for U in range(1, 5)]


def n_points(n, L):
    return len(range(0, n - L, L))


def test_worked_cases():
    assert make_resample_schedule(6, 2, 2) == ([5, 4, 3, 4, 3, 2, 1, 2, 1, 0], [(3, 2, 4), (7, 0, 2)])
    assert make_resample_schedule(8, 2, 2) == ([7, 6, 5, 6, 5, 4, 3, 4, 3, 2, 1, 2, 1, 0], [(3, 4, 6), (7, 2, 4), (11, 0, 2)])
    assert make_resample_schedule(6, 5, 2)[0] == [5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 0]
    assert make_resample_schedule(5, 1, 3)[0] == [4, 4, 4, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0]
    assert make_resample_schedule(6, 6, 3) == ([5, 4, 3, 2, 1, 0], [])
    for n, L in ((6, 2), (8, 3), (20, 4), (1, 1)):
        assert make_resample_schedule(n, L, 1) == (list(range(n - 1, -1, -1)), [])


@pytest.mark.parametrize("n,L,U,count", [(250, 10, 10, 2410), (1000, 10, 10, 9910), (20, 4, 3, 52)])
def test_counts(n, L, U, count):
    visits, jumps = make_resample_schedule(n, L, U)
    assert len(visits) == count == n + (U - 1) * L * n_points(n, L)
    assert len(jumps) == (U - 1) * n_points(n, L)


def test_equals_the_independent_construction_on_the_sweep():
    for n, L, U in SWEEP:
        assert make_resample_schedule(n, L, U) == RR.resample_schedule(n, L, U), (n, L, U)


def test_invariants_on_the_sweep():
    for n, L, U in SWEEP:
        visits, jumps = make_resample_schedule(n, L, U)
        assert visits[0] == n - 1 and visits[-1] == 0 and visits.count(0) == 1, (n, L, U)
        assert len(visits) == n + (U - 1) * L * n_points(n, L)
        after = {k: (a, b) for k, a, b in jumps}
        assert len(after) == len(jumps)
        for k in range(1, len(visits)):                     # evaluation k (from 1) is visits[k - 1]; the next one is visits[k]
            d = visits[k] - visits[k - 1]
            if k in after:
                a, b = after[k]
                assert d == L - 1 and a == visits[k - 1] - 1 and b == a + L == visits[k], (n, L, U, k)
            else:
                assert d == -1, (n, L, U, k)
        left = {}
        for _, a, b in jumps:
            left[a] = left.get(a, 0) + 1
        assert left == ({j: U - 1 for j in range(0, n - L, L)} if U > 1 else {}), (n, L, U)


@pytest.mark.parametrize("args", [(6, 0, 2), (6, 2, 0), (6, -1, 2), (6, 2.0, 2), (6, 2, 1.5), (6, "2", 2), (6, 2, None), (0, 2, 2), (6, True, 2)])
def test_bad_arguments_are_refused(args):
    with pytest.raises(EodError):
        make_resample_schedule(*args)


@pytest.mark.parametrize("T,L", [(1000, 10), (250, 10), (1000, 1), (1000, 500)])
def test_renoise_coefficients_vs_float64(T, L):
    """x_b = ca x_a + cb z must carry the signal sqrt(acp_b) and the variance 1 - acp_b when x_a carries sqrt(acp_a) and 1 - acp_a:
        |ca sqrt(acp_a) - sqrt(acp_b)| <= 2 * 2^-24 * sqrt(acp_b)      three roundings enter ca (the quotient at half weight, the root): 1.5 ulp
        |ca^2 (1 - acp_a) + cb^2 - (1 - acp_b)| <= 8 * 2^-24           quotient once, ca's root twice, 1 - r once, cb's root twice: 6 * 2^-24
    over every jump (j, j + L) of the cosine schedule.  A wrong ratio (a product of betas, a level off by one) misses both by orders."""
    from oracle.schedule import eo_cosine_tables
    acp32 = eo_cosine_tables(T)["alphas_cumprod"].numpy()
    acp = acp32.astype(np.float64)
    u = 2.0 ** -24
    worst_s = worst_v = 0.0
    pairs = [(j, j + L) for j in range(0, T - L, L)]
    assert pairs
    for a, b in pairs:
        assert 0.0 < acp32[b] <= acp32[a]
        ca, cb = (float(v) for v in RR.renoise_coeffs(acp32[a], acp32[b]))
        es = abs(ca * np.sqrt(acp[a]) - np.sqrt(acp[b])) / np.sqrt(acp[b])
        ev = abs(ca * ca * (1.0 - acp[a]) + cb * cb - (1.0 - acp[b]))
        worst_s, worst_v = max(worst_s, es), max(worst_v, ev)
    print(f"T = {T}, L = {L}: {len(pairs)} jumps, worst signal error {worst_s / u:.2f} * 2^-24 relative, worst variance error {worst_v / u:.2f} * 2^-24")
    assert worst_s <= 2 * u and worst_v <= 8 * u
