"""Host only: which form of conv_up4_halo_kernel conv_plan() (csrc/igemm.hip) gives an upsample = 3 descriptor, read through
eod_conv_halo_columns.  The split product of fp32 storage takes the 8-wave 256-column form where its launch still has a workgroup for
every CU, N * (H / 8) * ceil(W / 16) * 4 * (Cout / 256) >= 256 -- ((Cout - 128) / 256) for 256 + 128 columns -- unless halo_bn256 is
0; 128 columns have no such form; fp16 storage and the backward-data instance (upsample = 4) stay on the 4-wave form.  The kernel name
does not tell the forms apart, and none of the plan's other answers moves with the option."""
import ctypes as C

import pytest

from eo_diffusion_amd import _lib
from tests.test_conv_plan import QUERIES, _row, arm, bind, make_desc

# stored maps at batch 4: 32 x 64 has 16 tiles -> 4 * 16 * 4 = 256 workgroups of 256 columns (AT the rule), 32 x 32 half of that (below)
AT, BELOW = (32, 64), (32, 32)


def columns(L, storage, hw, cout, bn256, ups=3, n=4):
    with arm(L, ("halo_bn256", bn256)):
        d = make_desc(L, _row(storage, n, hw, cout, (256, 0), ups=ups, flags=("stats",) if ups == 3 else ()))
        assert L.eod_conv_kernel_name(C.byref(d)).decode() == "conv_up4_halo_kernel"
        return L.eod_conv_halo_columns(C.byref(d))


@pytest.fixture(scope="module")
def L():
    lib = bind(_lib.lib())
    lib.eod_conv_halo_columns.restype, lib.eod_conv_halo_columns.argtypes = C.c_int32, [C.POINTER(_lib.ConvDesc)]
    return lib


@pytest.mark.parametrize("cout", [128, 256, 384, 512])
def test_split_product_columns_follow_the_rule_and_the_option(L, cout):
    at = 128 if cout == 128 else 256
    assert columns(L, "fp32x3", AT, cout, 1) == at
    assert columns(L, "fp32x3", AT, cout, 0) == 128
    # below the rule: 128 workgroups per 256 columns; 512 columns are two column tiles per class, so that grid still has its 256
    assert columns(L, "fp32x3", BELOW, cout, 1) == (256 if cout == 512 else 128)
    assert columns(L, "fp32x3", BELOW, cout, 0) == 128
    assert columns(L, "fp32x3", (16, 32), cout, 1) == 128  # 4 tiles per image: below the rule at every width
    assert columns(L, "fp32x3", AT, cout, 1, n=3) == (256 if cout == 512 else 128)  # the rule counts the actual batch


@pytest.mark.parametrize("cout", [128, 256, 384, 512])
@pytest.mark.parametrize("bn256", [0, 1])
def test_fp16_storage_and_the_backward_instance_stay_on_the_4_wave_form(L, cout, bn256):
    assert columns(L, "fp16", AT, cout, bn256) == 128
    assert columns(L, "fp16", (64, 128), cout, bn256, ups=4) == 0  # (backward-data: not a forward form; the query names none)


@pytest.mark.parametrize("cout", [256, 384, 512])
@pytest.mark.parametrize("hw", [AT, BELOW])
def test_the_form_changes_no_other_answer(L, cout, hw):
    r = _row("fp32x3", 4, hw, cout, (256, 0), ups=3, flags=("stats",))
    got = []
    for v in (1, 0):
        with arm(L, ("halo_bn256", v)):
            d = make_desc(L, r)
            got.append([int(getattr(L, q)(C.byref(d))) for q in QUERIES])
    assert got[0] == got[1], got
