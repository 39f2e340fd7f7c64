"""ESAN timing (development helper, not the bench: bench.py has no ESAN entry): ms per forward and images/s of fp32 / bf16 / fp16 forwards at
32 x 256 x 256 and one 339 x 510 image with fuse_head on and off -- both forms in ONE process, so that they meet the same GPU --, each
configuration timed `--repeats` times (the run-to-run spread of the visit), then the per-kernel breakdown (enable_profiling): the one-launch
residual-block head against the four launches it replaces, and its achieved bytes/s against the copy bandwidth esr_bw_probe measures.
Random weights are not used: the checkpoint fixture of tests/golden/.  Inputs are in [0, 255] (data_range 255).
usage: esan_time.py [--steps N] [--repeats R] [--json OUT]"""
import argparse, collections, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safetensors.torch import load_file
from ntire2022_esr_amd import ESAN, _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
m = ESAN()
m.load_state_dict(load_file(os.path.join(REPO, "tests", "golden", "team34_esan.safetensors")), strict=True)
m = m.eval().to(dev)
rows = []
print(f"library source hash {L.lib().esr_source_hash().decode()[:12]}")
# bench.py's hbm_copy_kernel_gbs: the read + write rate of a plain copy kernel at a 2 x 1 GiB working set (esr_bw_probe), second call
scratch = torch.empty(2 * (1 << 30), dtype=torch.uint8, device=dev)
gbs = ctypes.c_double(0.0)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for _ in range(2):
    L.check(L.lib().esr_bw_probe(ctypes.c_void_p(scratch.data_ptr()), 1 << 30, 1, stream, ctypes.byref(gbs)), "esr_bw_probe")
copy_gbs = gbs.value
print(f"hbm_copy_kernel_gbs (esr_bw_probe, 2 x 1 GiB) {copy_gbs:.0f} GB/s")
del scratch


def is_step(o):       # the ops of a block's head: the fused launch, or the identity add / conv1 / conv2 / ESA.conv1 of the per-op form
    return "resblock_head" in o["kernel"] or o["name"] == "ident" or o["name"].endswith((".conv1", ".conv2")) and ".ESA.conv2" not in o["name"]


for comp in ("f32", "bf16", "f16"):
    m.set_compute(comp)
    for fuse in ((False,) if comp == "f32" else (True, False)):
        m.fuse_head = fuse
        for B, h, w in ((32, 256, 256), (1, 339, 510)):
            x = torch.rand(B, 3, h, w, device=dev) * 255
            with torch.no_grad():
                for _ in range(3):
                    m(x)
                torch.cuda.synchronize()
                times = []
                for _ in range(args.repeats):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(args.steps):
                        m(x)
                    e.record()
                    torch.cuda.synchronize()
                    times.append(s.elapsed_time(e) / args.steps)
                ms = min(times)
                m.enable_profiling(3)
                for _ in range(3):
                    m(x)
                torch.cuda.synchronize()
                agg = collections.defaultdict(lambda: [0.0, 0])
                step_ms, step_bytes, n_launch = 0.0, 0.0, 0
                for o in m.collect_profile():
                    a = agg[o["kernel"]]
                    a[0] += o["ms_sum"] / 3
                    a[1] += o["passes"] // 3
                    if is_step(o):
                        step_ms += o["ms_sum"] / 3
                        step_bytes += o["stored_bytes"]
                    n_launch += 1
                m.disable_profiling()
            step_gbs = step_bytes / (step_ms * 1e-3) / 1e9 if step_ms else 0.0
            row = dict(compute=comp, fuse_head=fuse, batch=B, h=h, w=w, ms_per_forward=ms, ms_repeats=times, images_per_s=B / ms * 1e3,
                       ops=n_launch, steps_ms=step_ms, steps_gbs=step_gbs, hbm_copy_kernel_gbs=copy_gbs,
                       kernels={k: round(v[0], 4) for k, v in agg.items()})
            rows.append(row)
            print(f"{comp:4s} fuse_head={int(fuse)} {B:2d} x {h} x {w}: {ms:8.3f} ms/fwd (repeats {', '.join(f'{t:.3f}' for t in times)}) "
                  f"{B / ms * 1e3:8.1f} img/s, {n_launch} ops, the block heads {step_ms:.4f} ms/fwd at {step_gbs:.0f} GB/s stored", flush=True)
            tot = sum(v[0] for v in agg.values())
            for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:10]:
                print(f"      {k:60s} {v[1]:3d} launches/fwd {v[0]:8.3f} ms/fwd {v[0] / tot * 100:5.1f}%")
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(rows, open(args.json, "w"), indent=1)
