"""CPU (-m "not gpu"): the shim packages resolve the import paths an unmodified test_demo.py uses (test_demo.py:8-10, 20,
26, 54, 152) to this repo's own classes, with the reference's ctor / load_state_dict / eval / to lifecycle and the
reference's complexity numbers; and `model(x)` is ONE registered torch.library operator with a fake (shape) implementation."""
import contextlib
import importlib
import io
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLD, REPO, load_sd_torch

SHIM = os.path.join(REPO, "shim")


def _run_in_shim(code):
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def test_shim_import_paths_lifecycle_and_counters():
    code = r'''
import contextlib, io, json, os, sys, torch
from safetensors.torch import load_file
from models.imdn_baseline import IMDN
from models.rfdn_baseline.RFDN import RFDN
from models.team04_rlfn import RLFN_cut
from models.team18_bsrn import BSRN
from utils.model_summary import get_model_activation, get_model_flops
from utils import utils_logger
from utils import utils_image as util
import ntire2022_esr_amd as E
assert IMDN is E.IMDN and RFDN is E.RFDN and RLFN_cut is E.RLFN_cut and BSRN is E.BSRN
W = os.environ["ESR_WEIGHTS"]
out = {}
with contextlib.redirect_stdout(io.StringIO()):
    nets = {"imdn_baseline": IMDN(in_nc=3, out_nc=3, nc=64, nb=8, upscale=4), "rfdn_baseline": RFDN(),
            "team04_rlfn": RLFN_cut(in_nc=3, out_nc=3),
            "team18_bsrn": BSRN(num_in_ch=3, num_feat=48, num_block=5, num_out_ch=3, upscale=4, conv='BSConvU', upsampler='pixelshuffledirect')}
for name, model in nets.items():
    model.load_state_dict(load_file(os.path.join(W, name + ".safetensors")), strict=True)      # test_demo.py:23
    model.eval()                                                                                  # :336
    for k, v in model.named_parameters():
        v.requires_grad = False                                                                   # :338-339
    model = model.to(torch.device("cpu"))                                                         # :340
    acts, nconv = get_model_activation(model, (3, 256, 256))                                      # :525
    flops = get_model_flops(model, (3, 256, 256), False)                                          # :530
    out[name] = {"activations": acts, "num_conv": nconv, "flops": flops,
                 "num_parameters": sum(map(lambda x: x.numel(), model.parameters()))}            # :534
utils_logger.logger_info("t", log_path=os.devnull)
assert util.uint2tensor4(__import__("numpy").zeros((4, 5, 3), "uint8"), 255.0).shape == (1, 3, 4, 5)
print(json.dumps(out))
'''
    os.environ["ESR_WEIGHTS"] = os.path.join(REPO, "weights")
    got = json.loads(_run_in_shim(code).strip().splitlines()[-1])
    want = json.load(open(os.path.join(GOLD, "summary.json")))
    assert got == want


def test_shim_rider_modules():
    out = _run_in_shim("from models.team06_v1 import v1; from models.team22_rep_rfdn import RFDN40; "
                       "m = RFDN40(); print(len(m.state_dict()), len(v1(in_nc=3, nf=50, num_modules=4, out_nc=3, upscale=4).state_dict()))")
    assert out.split() == ["128", "128"]


def test_forward_is_a_registered_custom_op_with_fake_impl():
    from ntire2022_esr_amd import IMDN, RFDN, _lib as L, engine
    assert hasattr(torch.ops.esr, "sr_forward")
    m = IMDN()
    with pytest.raises(L.EsrError, match="no CPU fallback"):
        m(torch.rand(1, 3, 16, 16))                                  # the real kernel refuses CPU tensors
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        y = m(torch.empty(2, 3, 40, 56))                              # shape function only, nothing runs
        assert tuple(y.shape) == (2, 3, 160, 224) and y.dtype == torch.float32
    y = torch.ops.esr.sr_forward(torch.empty(1, 3, 17, 15, device="meta"), m.handle)
    assert tuple(y.shape) == (1, 3, 68, 60)
    with pytest.raises(Exception):
        torch.ops.esr.sr_forward(torch.empty(1, 3, 17, 15, device="meta"), 12345)       # no live model with that handle
    # handles come from a counter: never recycled, gone from the registry with their module
    h = m.handle
    m2 = IMDN()
    assert m2.handle > h and engine._LIVE.get(h) is m
    del m, y
    import gc
    gc.collect()
    assert engine._LIVE.get(h) is None and IMDN().handle > m2.handle
    r = RFDN()
    with FakeTensorMode():
        assert tuple(r(torch.empty(1, 3, 33, 21)).shape) == (1, 3, 132, 84)


def test_every_name_test_demo_uses_resolves_in_the_shim():
    """What the reference's test_demo.py uses (tests/golden/demo_calls.json: ast-parsed by tools/gen_golden_demo_calls.py, names
    and call shapes only): every `util.<name>` / `utils_logger.<name>` attribute it touches, every name it imports from
    utils.model_summary, and the `from models... import ...` lines of ids -1 / 0 / 4 / 18 (+ riders 6, 8, 22, 26, 40) must
    resolve in shim/ with a compatible call signature (test_demo.py:8-10, 17-30, 52-58, 150-157, 411-465)."""
    import inspect
    demo = json.load(open(os.path.join(GOLD, "demo_calls.json")))
    aliases = demo["utils_aliases"]                      # local alias -> shim module
    from_summary = demo["summary_imports"]
    assert aliases == {"utils_logger": "utils.utils_logger", "util": "utils.utils_image"}, aliases
    used = {(a["alias"], a["attr"]): a["calls"] for a in demo["attributes"]}     # (alias, attr) -> call sites (positional count, keywords)
    assert ("util", "mkdir") in used and ("util", "imsave") in used and ("utils_logger", "logger_info") in used
    # registry entries this engine implements: model_id -> (module, class) from the select_model body
    model_imports = {int(mid): tuple(v) for mid, v in demo["select_model_imports"].items()}
    want_ids = [-1, 0, 4, 18, 6, 8, 22, 26, 40]
    assert all(i in model_imports for i in want_ids), sorted(model_imports)
    code = ["import importlib, inspect, json", "out = {}"]
    for (alias, attr), calls in sorted(used.items()):
        code.append(f"f = getattr(importlib.import_module({aliases[alias]!r}), {attr!r}); out[{alias + '.' + attr!r}] = str(inspect.signature(f))")
    for name in from_summary:
        code.append(f"f = getattr(importlib.import_module('utils.model_summary'), {name!r}); out['summary.{name}'] = str(inspect.signature(f))")
    for mid in want_ids:
        mod, names = model_imports[mid]
        for nm in names:
            code.append(f"getattr(importlib.import_module({mod!r}), {nm!r}); out['id{mid}'] = {mod + '.' + nm!r}")
    code.append("print(json.dumps(out))")
    got = json.loads(_run_in_shim("\n".join(code)).strip().splitlines()[-1])
    # every call site binds to the shim function's signature (positional count + keyword names)
    sys.path.insert(0, SHIM)
    try:
        for (alias, attr), calls in used.items():
            mod = importlib.import_module(aliases[alias])
            sig = inspect.signature(getattr(mod, attr))
            for c in calls:
                sig.bind(*[None] * c["nargs"], **{k: None for k in c["keywords"]})
    finally:
        sys.path.remove(SHIM)
        for m in [m for m in sys.modules if m == "utils" or m.startswith("utils.")]:
            del sys.modules[m]
    assert len(got) >= len(used) + len(from_summary) + len(want_ids)


def test_run_body_against_the_shim_with_a_stub_model(tmp_path):
    """The sequence of helper calls of the reference's run() (test_demo.py:411-465), executed against shim/utils with a stub
    model on the CPU: mkdir -> imread_uint -> uint2tensor4 -> forward -> tensor2uint -> modcrop -> calculate_psnr -> imsave."""
    code = r'''
import os, sys, numpy as np, torch
from utils import utils_image as util
from utils import utils_logger
import logging
d = sys.argv[1]
save_path = os.path.join(d, "out", "stub", "valid")
util.mkdir(save_path)                                            # test_demo.py:411
util.mkdir(save_path)                                            # idempotent
util.mkdirs([os.path.join(d, "a"), os.path.join(d, "b")])
rng = np.random.RandomState(0)
hr = rng.randint(0, 256, (40, 48, 3)).astype(np.uint8)
lr = hr[::4, ::4].copy()
util.imsave(hr, os.path.join(d, "0801.png")); util.imsave(lr, os.path.join(d, "0801x4.png"))
utils_logger.logger_info("stub", log_path=os.path.join(d, "log.txt"))
logger = logging.getLogger("stub")
img_lr = util.uint2tensor4(util.imread_uint(os.path.join(d, "0801x4.png"), n_channels=3), 1.0)
img_sr = torch.nn.functional.interpolate(img_lr, scale_factor=4, mode="nearest")     # the stub "model"
img_sr = util.tensor2uint(img_sr, 1.0)
img_hr = util.modcrop(util.imread_uint(os.path.join(d, "0801.png"), n_channels=3).squeeze(), 4)
psnr = util.calculate_psnr(img_sr, img_hr, border=4)
logger.info("{:s} - PSNR: {:.2f} dB".format("0801.png", psnr))
util.imsave(img_sr, os.path.join(save_path, "0801.png"))
assert os.path.exists(os.path.join(save_path, "0801.png")) and os.path.isdir(os.path.join(d, "b"))
print("ok", round(psnr, 2))
'''
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_kernel_level_custom_ops_are_registered_with_fake_impls():
    """BASELINE.json north star: "a thin PyTorch-ROCm custom-op layer exposes these [kernels]" -- esr::conv2d / esr::bsconv /
    esr::esa_apply / esr::channel_attention are registered operators whose fake implementations give the output shapes (FakeTensor
    tracing works without a GPU); the real ones refuse CPU tensors like every op of this engine."""
    from ntire2022_esr_amd import _lib as L, ops  # noqa: F401  (registers the operators)
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("conv2d", "bsconv", "esa_apply", "channel_attention", "sr_forward"):
        assert hasattr(torch.ops.esr, name), name
    with FakeTensorMode():
        x = torch.empty(2, 40, 56, 64)
        y = torch.ops.esr.conv2d(x, torch.empty(50, 64, 3, 3), torch.empty(50), 1, 0.05, None, 0, True)
        assert tuple(y.shape) == (2, 40, 56, 52)
        yb = torch.ops.esr.conv2d(x.to(torch.bfloat16), torch.empty(50, 64, 1, 1), None, 0, 0.05, None, 0, False)
        assert tuple(yb.shape) == (2, 40, 56, 56) and yb.dtype == torch.bfloat16
        z = torch.ops.esr.bsconv(torch.empty(1, 20, 20, 48), torch.empty(48, 48), None, torch.empty(48, 1, 3, 3), None, 3, 0.05, None, 0)
        assert tuple(z.shape) == (1, 20, 20, 48)
        e = torch.ops.esr.esa_apply(torch.empty(1, 30, 30, 56), torch.empty(1, 30, 30, 16), torch.empty(1, 4, 4, 16), torch.empty(12, 12),
                                    None, torch.empty(50, 12), None)
        assert tuple(e.shape) == (1, 30, 30, 56)
        c = torch.ops.esr.channel_attention(torch.empty(2, 64, 24, 24), torch.empty(4, 64), None, torch.empty(64, 4), None, True, True)
        assert tuple(c.shape) == (2, 64, 24, 24)
    with pytest.raises(Exception):
        torch.ops.esr.conv2d(torch.rand(1, 8, 8, 64), torch.rand(64, 64, 3, 3), None, 0, 0.05, None, 0, True)      # CPU tensor: no fallback
