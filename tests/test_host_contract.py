"""CPU suite: host-side contract of the drop-in API -- state_dict key layout vs the reference's, module graph,
deep-copy / pickle safety, C-ABI library loads and exports every declared symbol, loud failure off-GPU."""
import copy
import ctypes
import os
import pickle
import re

import pytest
import torch

from tests.helpers import key_contracts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(key_contracts()))
def test_state_dict_keys_match_reference(name):
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    from eo_diffusion_amd.diffusion.model import EODiffusion
    kc = key_contracts()[name]
    shapes = unet_param_shapes(**kc["cfg"])
    assert list(shapes.keys()) == list(kc["unet"].keys())  # same keys in the same order
    assert {k: list(v) for k, v in shapes.items()} == kc["unet"]
    with torch.device("meta"):
        u = UNetModel(**kc["cfg"])
    m = EODiffusion(u, timesteps=1000, image_size=kc["cfg"]["image_size"], in_channels=3)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == kc["eodiffusion"]


def test_default_init_matches_reference_conventions():
    """zero_module convs are zero, GroupNorm affine is (1, 0) -- what a freshly constructed reference model has."""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    u = UNetModel(16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[2],
                  channel_mult=[1, 2])
    sd = u.state_dict()
    for k in ("out.2.weight", "out.2.bias", "conv_out.weight", "middle_block.1.proj_out.weight",
              "input_blocks.1.0.out_layers.3.weight"):
        assert float(sd[k].abs().max()) == 0.0, k
    assert torch.all(sd["out.0.weight"] == 1) and torch.all(sd["out.0.bias"] == 0)
    assert float(sd["input_blocks.1.0.in_layers.2.weight"].abs().max()) > 0


def test_modules_are_deepcopy_and_pickle_safe():
    """AveragedModel(model) deep-copies the whole EODiffusion (script_utils/utils.py:67, train.py:73)."""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.diffusion.model import EODiffusion
    u = UNetModel(16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[],
                  channel_mult=[1, 2])
    u.__dict__["_eod_cache"] = {"fake": ctypes.c_void_p(1)}  # what a live program cache looks like: not copyable
    m = EODiffusion(u, timesteps=10, image_size=16, in_channels=3)
    m2 = copy.deepcopy(m)
    assert "_eod_cache" not in m2.model.__dict__
    m3 = pickle.loads(pickle.dumps(m))
    assert list(m3.state_dict().keys()) == list(m.state_dict().keys())
    ema = torch.optim.swa_utils.AveragedModel(m, multi_avg_fn=None, use_buffers=True)
    assert any(k.startswith("module.model.") for k in ema.state_dict())


def test_library_exports_every_declared_symbol():
    from eo_diffusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eodiff.h")).read()
    declared = set(re.findall(r"\b(eod_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"eod_op", "eod_conv_desc", "eod_gemm_desc", "eod_temb_desc", "eod_small_desc"}
    L = _lib.lib()  # binds SYMBOLS and cross-checks struct sizes against the compiled library
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/eodiff.h but not exported"
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    assert L.eod_version() == _lib.ABI_VERSION


def test_conv_geometry_queries_are_pure_host_predicates():
    """the eod_conv_*_ok queries decide on the host which kernel form a conv descriptor gets (no device call): the rules of
    include/eodiff.h for the fused 1x1 skip conv, the parity-class upsample form and the fused input GroupNorm"""
    import ctypes as C
    from eo_diffusion_amd import _lib
    L = _lib.lib()

    def desc(**kw):
        d = _lib.ConvDesc()
        d.dtype, d.N, d.H, d.W, d.C0, d.C1, d.Cout = _lib.EOD_F32, 2, 32, 32, 128, 0, 128
        d.ksize, d.stride, d.pad, d.Ho, d.Wo, d.w_split = 3, 1, 1, 32, 32, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    ok = lambda fn, **kw: bool(fn(C.byref(desc(**kw))))
    # fused skip conv: 3x3 / stride 1 on maps that tile into 8 x 16 patches, > 64 output channels, whole 8-channel groups
    assert ok(L.eod_conv_skip_ok, skip_C0=256, skip_C1=128)
    assert ok(L.eod_conv_skip_ok, skip_C0=64, dtype=_lib.EOD_F16, w_split=0)
    assert not ok(L.eod_conv_skip_ok, skip_C0=0)
    assert not ok(L.eod_conv_skip_ok, skip_C0=60)                       # not a multiple of 8
    assert not ok(L.eod_conv_skip_ok, skip_C0=64, w_split=0)            # exact fp32 keeps the separate launch
    assert not ok(L.eod_conv_skip_ok, skip_C0=64, W=24, Wo=24)          # 24 columns do not tile
    assert not ok(L.eod_conv_skip_ok, skip_C0=64, Cout=64)
    assert not ok(L.eod_conv_skip_ok, skip_C0=64, stride=2, Ho=16, Wo=16)
    assert not ok(L.eod_conv_skip_ok, skip_C0=64, C1=32)                # the 3x3 input is a single source
    # parity-class upsample form: stored map tiles into 8 x 16 patches, fp16 or split fp32
    assert ok(L.eod_conv_up4_ok, upsample=3, Ho=64, Wo=64)
    assert not ok(L.eod_conv_up4_ok, upsample=3, Ho=64, Wo=64, w_split=0)
    assert not ok(L.eod_conv_up4_ok, upsample=1, Ho=64, Wo=64)
    assert not ok(L.eod_conv_up4_ok, upsample=3, H=20, Ho=40, Wo=64)
    # fused input GroupNorm: every width in split fp32, up to 256 output channels in fp16 storage
    assert ok(L.eod_conv_gn_fusable, Cout=512)
    assert ok(L.eod_conv_gn_fusable, Cout=256, dtype=_lib.EOD_F16, w_split=0)
    assert not ok(L.eod_conv_gn_fusable, Cout=512, dtype=_lib.EOD_F16, w_split=0)
    assert not ok(L.eod_conv_gn_fusable, stride=2, Ho=16, Wo=16)
    # the kernel family of the plan the launcher itself follows, under the names of bench.py's per-op tables
    name = lambda **kw: L.eod_conv_kernel_name(C.byref(desc(**kw))).decode()
    assert name() == "conv3x3_halo_kernel"
    assert name(upsample=3, Ho=64, Wo=64) == "conv_up4_halo_kernel"
    assert name(H=64, W=64, stride=2) == "conv_s2_halo_kernel"
    assert name(stride=2, Ho=16, Wo=16) == "igemm_kernel"              # 16 x 16 output map: split in K on the generic kernel
    assert name(ksize=1, pad=0) == "igemm_kernel"
    assert name(w_tapmajor=1, C0=8) == "conv_first_x3_kernel"
    assert name(w_tapmajor=1, C0=8, dtype=_lib.EOD_F16, w_split=0) == "igemm_kernel"
    assert name(Cout=3, out_nchw_f32=1, gn_scale_shift=1 << 20) == "conv_head_kernel"
    assert name(Cout=3, out_nchw_f32=1, gn_scale_shift=1 << 20, w_split=0) == "conv3x3_halo_kernel<BN=32>"   # exact fp32 has no head kernel
    assert name(W=24, Wo=24) == "igemm_kernel"                          # 24 columns do not tile


def test_product_fails_loudly_without_gpu():
    from eo_diffusion_amd import _lib
    from eo_diffusion_amd.backbones.unet_openai import ResBlock, UNetModel, normalization
    from eo_diffusion_amd.diffusion.model import EODiffusion
    u = UNetModel(16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[],
                  channel_mult=[1, 2])
    m = EODiffusion(u, timesteps=10, image_size=16, in_channels=3)
    with torch.no_grad():
        with pytest.raises(_lib.EodError):
            u(torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.long))
        with pytest.raises(_lib.EodError):
            m.sampling(1, device="cpu")
        with pytest.raises(_lib.EodError):
            m._forward_diffusion(torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.long), torch.zeros(1, 3, 16, 16))
        with pytest.raises(_lib.EodError):
            normalization(32)(torch.zeros(1, 32, 4, 4))  # parameter containers never run torch arithmetic
        with pytest.raises(_lib.EodError):
            ResBlock(32, 128, 0.0)(torch.zeros(1, 32, 4, 4), torch.zeros(1, 128))


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "eo_diffusion_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(dirpath, f)


def test_ddim_schedule_host_tables_match_golden():
    import numpy as np
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from tests.helpers import gload
    m = EODiffusion(torch.nn.Identity(), timesteps=1000, image_size=8, in_channels=3)
    for S in (50, 250, 600, 1000):
        for eta in (0.0, 0.5):
            s = DDIMSampler(m)
            s.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
            g = gload(f"ddim_S{S}_T1000_eta{eta}")
            assert np.array_equal(np.asarray(s.ddim_timesteps, np.int64), g["steps"])  # integer schedule: bit-exact
            assert np.array_equal(np.asarray(s.ddim_alphas), g["a"])
            assert np.array_equal(np.asarray(s.ddim_alphas_prev, np.float64), g["a_prev"])


def test_dropin_module_paths():
    import subprocess
    import sys
    code = ("from backbones.unet_openai import UNetModel, ResBlock, AttentionBlock; from diffusion.model import EODiffusion; "
            "from diffusion.ddim import DDIMSampler; from diffusion.util import make_ddim_timesteps; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "eo_diffusion_amd", "dropin") + os.pathsep + ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_checkpoint_wire_format_roundtrip(tmp_path):
    """train.py:137-138,155 / inference.py:81-86: torch.save({"model": sd, "model_ema": ema_sd}) and back."""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.diffusion.model import EODiffusion
    mk = lambda: EODiffusion(UNetModel(16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1,
                                       attention_resolutions=[2], channel_mult=[1, 2], num_heads=2),
                             timesteps=50, image_size=16, in_channels=3)
    m = mk()
    ema = torch.optim.swa_utils.AveragedModel(m, use_buffers=True)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01)
    ema.update_parameters(m)
    path = tmp_path / "ckpt.pt"
    torch.save({"model": m.state_dict(), "model_ema": ema.state_dict()}, path)
    ck = torch.load(path)
    assert set(ck) == {"model", "model_ema"} and "n_averaged" in ck["model_ema"]
    assert any(k.startswith("module.model.input_blocks.") for k in ck["model_ema"])
    m2 = mk()
    ema2 = torch.optim.swa_utils.AveragedModel(m2, use_buffers=True)
    m2.load_state_dict(ck["model"])
    ema2.load_state_dict(ck["model_ema"])
    for a, b in zip(m.state_dict().values(), m2.state_dict().values()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("sch,T", [("linear", 1000), ("cosine", 1000), ("linear", 20), ("sqrt_linear", 50)])
def test_ldm_register_schedule_buffers_vs_fixture(sch, T):
    """a21 (ddpm.py:122-162): the product's register_schedule buffers equal the harness-derived float64 tables bit for bit (the 11
    tables + betas; fixture = reference make_beta_schedule + the table formulas evaluated by tests/golden/make_golden.py)"""
    import torch
    from eo_diffusion_amd.diffusion.ddpm import DDPM
    from tests.helpers import bits_equal, gt
    g = gt(f"ldm_tables_{sch}_T{T}")
    m = DDPM(torch.nn.Identity(), timesteps=T, beta_schedule=sch)
    assert m.num_timesteps == T
    for k, v in g.items():
        assert bits_equal(getattr(m, k), v), (sch, T, k)


def test_make_label_matches_reference_semantics():
    """script_utils/utils.py:17-37: one rectangle of ones, side lengths between 10 % and 40 % of the image, fully inside it, and
    the same draw order from the same RandomState as the reference's four np.random.randint calls"""
    import numpy as np
    from eo_diffusion_amd.harness import make_label
    for seed in range(20):
        lab = make_label((64, 48), 10, 10, 40, 40, np.random.RandomState(seed))
        r = np.random.RandomState(seed)
        ws, hs = r.randint(6, 25, 1)[0], r.randint(4, 19, 1)[0]
        x, y = r.randint(ws, 64 - ws, 1)[0], r.randint(hs, 48 - hs, 1)[0]
        ref = np.zeros((64, 48))
        ref[x:x + ws, y:y + hs] = 1
        assert np.array_equal(lab, ref) and lab.sum() == ws * hs


def test_make_label_vs_reference_outputs():
    """the rectangles the reference's own make_label returned under np.random.seed(seed) (tests/golden/make_golden.py gen_make_label;
    make_label_boxes.npz): same seeds, same global numpy generator -> the same arrays"""
    import numpy as np
    from eo_diffusion_amd.harness import make_label
    from tests.helpers import gt
    g = gt("make_label_boxes")
    cases, boxes = g["cases"].numpy(), g["boxes"].numpy()
    for ci, seed, x, y, ws, hs, total in boxes:
        w, h, mnw, mnh, mxw, mxh = (int(v) for v in cases[ci])
        np.random.seed(1000 * int(ci) + int(seed))
        lab = make_label((w, h), mnw, mnh, mxw, mxh)
        ref = np.zeros((w, h))
        ref[x:x + ws, y:y + hs] = 1.0
        assert lab.sum() == total and np.array_equal(lab, ref), (ci, seed)


def test_dropin_modules_define_every_name_of_the_reference_modules():
    """`from backbones.unet_openai import X` / `from diffusion.{model,ddim,util} import X` works for every top-level class / function X of
    the reference's modules on the path, and every `Class.method` exists (fixture: names read from the reference's syntax trees by
    tests/golden/make_golden.py api_names).  The only names without a counterpart are the two private `_forward` bodies the reference's
    `checkpoint()` wrapper calls (ResBlock / AttentionBlock: here `forward` emits launch descriptors, there is no second body)."""
    import importlib
    import json
    root = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(root, "golden", "api_names.json")) as f:
        names = json.load(f)
    missing = []
    for rel, lst in names.items():
        for pkg in ("eo_diffusion_amd.", "eo_diffusion_amd.dropin."):
            mod = importlib.import_module(pkg + rel[:-3].replace("/", "."))
            for nm in lst:
                obj = mod
                try:
                    for part in nm.split("."):
                        obj = getattr(obj, part)
                except AttributeError:
                    missing.append(f"{pkg}{rel}:{nm}")
    allowed = {f"{pkg}backbones/unet_openai.py:{c}._forward" for pkg in ("eo_diffusion_amd.", "eo_diffusion_amd.dropin.")
               for c in ("ResBlock", "AttentionBlock")}
    assert set(missing) == allowed, sorted(set(missing) ^ allowed)
