"""GPU: the prediction-target kernels (eod_param_pred, eod_ddpm_param_pred, eod_q_sample_v; csrc/sampler.hip, csrc/param_body.h) on tensors
of more than 2^31 elements.  They are scene-sized like the rows of tests/test_gpu_big_index.py and go through that module's driver unchanged
(run_row: reference windows around 2^29, 2^30, 2^31 and the sample boundaries, the whole tensor against the same entry point on views of at
most 2^26 elements, NaN-prefilled outputs with guard bands, its shapes (i) and (ii), its vector and scalar paths, its memory accounting).
Their binding table is _lib.PARAM_SYMBOLS (include/eodiff_param.h); the ledger below places every name of it here, as that module's ledger
places every name of _lib.SYMBOLS."""
import sys

import pytest
import torch

from eo_diffusion_amd import _lib
from tests import param_ref as PRM
from tests import test_gpu_big_index as BI
from tests.test_gpu_big_index import _account, tabs  # noqa: F401  (that module's fixtures: memory / time accounting, the schedule tables)

pytestmark = pytest.mark.gpu

ROWS = [
    BI.Row("param_pred", "eod_param_pred", 2, 2, False, True,
           lambda L, st, A, I, O, N, chw, t, C, hw, m: L.eod_param_pred(I[0], I[1], 2, BI.A_T, BI.S1M, 1, O[0], O[1], N * chw, st),
           lambda A, ins, t, m: [v.numpy() for v in PRM.pred(BI._t1(ins[0]), BI._t1(ins[1]), PRM.V, BI.A_T, BI.S1M, True)]),
    BI.Row("param_pred_x0", "eod_param_pred", 2, 2, False, True,
           lambda L, st, A, I, O, N, chw, t, C, hw, m: L.eod_param_pred(I[0], I[1], 1, BI.A_T, BI.S1M, 0, O[0], O[1], N * chw, st),
           lambda A, ins, t, m: [v.numpy() for v in PRM.pred(BI._t1(ins[0]), BI._t1(ins[1]), PRM.X0, BI.A_T, BI.S1M, False)]),
    BI.Row("ddpm_param_pred", "eod_ddpm_param_pred", 2, 1, False, True,
           lambda L, st, A, I, O, N, chw, t, C, hw, m: L.eod_ddpm_param_pred(I[0], I[1], t, A.p(BI.SA), A.p(BI.SB), 2, 1, O[0], N, chw, BI.T, st),
           lambda A, ins, t, m: [PRM.ddpm_pred(A.tb, BI._t4(ins[0]), BI._t4(ins[1]), torch.tensor([t]), PRM.V, True).numpy()]),
    BI.Row("q_sample_v", "eod_q_sample_v", 2, 2, False, True,
           lambda L, st, A, I, O, N, chw, t, C, hw, m: L.eod_q_sample_v(I[0], I[1], t, A.p(BI.SA), A.p(BI.SB), O[0], O[1], N, chw, BI.T, st),
           lambda A, ins, t, m: [v.numpy() for v in PRM.q_sample_v(A.tb, BI._t4(ins[0]), BI._t4(ins[1]), torch.tensor([t]))]),
]
CASES = [(r, s, p) for r in ROWS for s in ("i", "ii") for p in ("vector", "scalar")]


@pytest.mark.parametrize("row,shape,path", CASES, ids=[f"{r.name}-{s}-{p}" for r, s, p in CASES])
def test_big_param_rows(row, shape, path, tabs):  # noqa: F811
    """(i) a sample of 2^31 + 2^16 + 4 (scalar: + 3) elements, whose loop index passes 2^31; (ii) three samples of 13 x 7424 x 7424, whose
    last base offset does"""
    N, chw, C, hw, _ = BI.geometry(shape, path)
    BI._need((row.n_in + row.n_out) * N * chw * 4 / BI.GIB + 1.0)
    BI.run_row(row, shape, path, tabs)


def test_big_every_prediction_target_entry_point_is_run_here():
    """every symbol of _lib.PARAM_SYMBOLS is launched by a row of this module, and none of them is hidden from the other ledger by being
    in both tables.  A new entry point of include/eodiff_param.h has to get a row"""
    assert {r.symbol for r in ROWS} == set(_lib.PARAM_SYMBOLS)
    assert not set(_lib.PARAM_SYMBOLS) & set(_lib.SYMBOLS)
    assert callable(getattr(sys.modules[__name__], "test_big_param_rows"))
