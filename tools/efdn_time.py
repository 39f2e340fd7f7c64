"""EFDN timing (development helper, not the bench: bench.py has no EFDN entry): images/s of fp32 / bf16 / fp16 forwards at 32 x 256 x 256 and
ms at one 339 x 510 image, with fuse_esa_lowres on and off, then the per-kernel breakdown of each configuration (enable_profiling), with the
ESA low-resolution branch's time (the fused esa_pool7 pair of launches against esr_maxpool7s7_f32 + the three small convolutions it replaces).
Random weights are not used: the checkpoint fixture of tests/golden/.
usage: efdn_time.py [--steps N] [--json OUT]"""
import argparse, collections, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safetensors.torch import load_file
from ntire2022_esr_amd import PLAINRFDN, _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
m = PLAINRFDN()
m.load_state_dict(load_file(os.path.join(REPO, "tests", "golden", "team05_efdn.safetensors")), strict=True)
m = m.eval().to(dev)
rows = []
print(f"library source hash {L.lib().esr_source_hash().decode()[:12]}")
for comp in ("f32", "bf16", "f16"):
    m.set_compute(comp)
    for fuse in (True, False):
        m.fuse_esa_lowres = fuse
        for B, h, w in ((32, 256, 256), (1, 339, 510)):
            x = torch.rand(B, 3, h, w, device=dev) * 255
            with torch.no_grad():
                for _ in range(3):
                    m(x)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(args.steps):
                    m(x)
                e.record()
                torch.cuda.synchronize()
                ms = s.elapsed_time(e) / args.steps
                m.enable_profiling(3)
                for _ in range(3):
                    m(x)
                torch.cuda.synchronize()
                agg = collections.defaultdict(lambda: [0.0, 0])
                lowres_ms = 0.0
                for o in m.collect_profile():
                    a = agg[o["kernel"]]
                    a[0] += o["ms_sum"] / 3
                    a[1] += o["passes"] // 3
                    if "pool7" in o["kernel"] or ".esa.conv_2" in o["name"] or ".esa.conv_3" in o["name"] or ".esa.conv_23" in o["name"]:
                        lowres_ms += o["ms_sum"] / 3    # the low-resolution branch: the fused op, or the pooling + the three convolutions
                m.disable_profiling()
            row = dict(compute=comp, fuse_esa_lowres=fuse, batch=B, h=h, w=w, ms_per_forward=ms, images_per_s=B / ms * 1e3,
                       esa_lowres_ms=lowres_ms, kernels={k: round(v[0], 4) for k, v in agg.items()})
            rows.append(row)
            print(f"{comp:4s} fuse_esa_lowres={int(fuse)} {B:2d} x {h} x {w}: {ms:8.3f} ms/fwd {B / ms * 1e3:8.1f} img/s, "
                  f"ESA low-resolution branch {lowres_ms:.4f} ms/fwd")
            tot = sum(v[0] for v in agg.values())
            for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:12]:
                print(f"      {k:60s} {v[1]:3d} launches/fwd {v[0]:8.3f} ms/fwd {v[0] / tot * 100:5.1f}%")
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(rows, open(args.json, "w"), indent=1)
