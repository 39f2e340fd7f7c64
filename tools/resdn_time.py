"""ResDN (team 43) timing (development helper, not the bench: bench.py has no ResDN entry): ms per forward and images/s of bf16 / fp16 / fp32
forwards at 32 x 256 x 256 and one 339 x 510 image with fuse_resdb on and off -- two instances of the model in ONE process, their repeats
INTERLEAVED (fused, per-layer, fused, per-layer, ...), so that both forms meet the same GPU in the same minute and the spread between
repeats is the yardstick for their difference --, fp32 throughput for the record, then the per-kernel breakdown (enable_profiling): the
twelve ResDB steps -- one esr_resdb_step launch, or five: esr_prelu, the expansion 1x1's two parts, esr_prelu, the 3x3 -- with their stored
bytes per pixel from cost() and their achieved bytes/s against the copy bandwidth esr_bw_probe measures, and the PReLU launches alone.
Random weights are not used: the checkpoint fixture of tests/golden/; the inputs are in 0 .. 1, the network's data_range.
usage: resdn_time.py [--steps N] [--repeats R] [--json OUT]"""
import argparse, collections, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safetensors.torch import load_file
from ntire2022_esr_amd import ResDN, _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
sd = load_file(os.path.join(REPO, "tests", "golden", "team43_resdn.safetensors"))
models = {}
for form, fuse in (("fused", True), ("per-layer", False)):
    m = ResDN()
    m.load_state_dict(sd, strict=True)
    m.fuse_resdb = fuse
    models[form] = m.eval().to(dev)
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


def is_step(o):       # the ops of the twelve steps: expansion{j}.0 / .1#res / .1#dist, compression{j}.0 / .1
    return o["name"].split(".")[1].startswith(("expansion", "compression")) if o["name"].startswith("body_unit") else False


def timed(m, x):
    steps = args.steps * (10 if x.shape[0] == 1 else 1)       # a single image: ten times the forwards, so that a timing is not a few milliseconds
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        m(x)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def breakdown(m, x):
    m.enable_profiling(3)
    for _ in range(3):
        m(x)
    torch.cuda.synchronize()
    agg = collections.defaultdict(lambda: [0.0, 0])
    c_ms, c_bytes, p_ms, p_bytes, n_launch = 0.0, 0.0, 0.0, 0.0, 0
    for o in m.collect_profile():
        a = agg[o["kernel"]]
        a[0] += o["ms_sum"] / 3
        a[1] += o["passes"] // 3
        if is_step(o):
            c_ms += o["ms_sum"] / 3
            c_bytes += o["stored_bytes"]
        if o["kernel"].startswith("prelu_kernel"):
            p_ms += o["ms_sum"] / 3
            p_bytes += o["stored_bytes"]
        n_launch += 1
    m.disable_profiling()
    return agg, c_ms, c_bytes, p_ms, p_bytes, n_launch


for comp in ("bf16", "f16", "f32"):
    forms = {f: m for f, m in models.items() if comp != "f32" or f == "per-layer"}      # (an fp32 plan has the per-layer form only)
    for m in forms.values():
        m.set_compute(comp)
    for B, h, w in ((32, 256, 256), (1, 339, 510)):
        x = torch.rand(B, 3, h, w, device=dev)
        with torch.no_grad():
            for m in forms.values():
                for _ in range(3):
                    m(x)
            torch.cuda.synchronize()
            times = {form: [] for form in forms}
            for _ in range(args.repeats):                  # interleaved: one repeat of every form, then the next repeat
                for form, m in forms.items():
                    times[form].append(timed(m, x))
            for form, m in forms.items():
                agg, c_ms, c_bytes, p_ms, p_bytes, n_launch = breakdown(m, x)
                ts = times[form]
                ms = min(ts)
                c_gbs = c_bytes / (c_ms * 1e-3) / 1e9 if c_ms else 0.0
                p_gbs = p_bytes / (p_ms * 1e-3) / 1e9 if p_ms else 0.0
                rows.append(dict(compute=comp, form=form, batch=B, h=h, w=w, ms_per_forward=ms, ms_repeats=ts, images_per_s=B / ms * 1e3,
                                 ops=n_launch, steps_ms=c_ms, steps_gbs=c_gbs, steps_stored_bytes_per_pixel=c_bytes / (1.0 * B * h * w),
                                 prelu_ms=p_ms, prelu_gbs=p_gbs, hbm_copy_kernel_gbs=copy_gbs, kernels={k: round(v[0], 4) for k, v in agg.items()}))
                print(f"{comp:4s} {form} {B:2d} x {h} x {w}: min {ms:8.3f} ms/fwd (repeats {', '.join(f'{t:.3f}' for t in ts)}; "
                      f"spread {(max(ts) - min(ts)) / min(ts) * 100:.1f} %) {B / ms * 1e3:8.1f} img/s, {n_launch} ops, the twelve steps "
                      f"{c_ms:.4f} ms/fwd at {c_gbs:.0f} GB/s stored, {c_bytes / (1.0 * B * h * w):.0f} B/pixel ({c_gbs / copy_gbs * 100:.0f} % of the copy bandwidth); "
                      f"the 28 PReLU launches {p_ms:.4f} ms/fwd at {p_gbs:.0f} GB/s", flush=True)
                tot = sum(v[0] for v in agg.values())
                for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:10]:
                    print(f"      {k:60s} {v[1]:3d} launches/fwd {v[0]:8.3f} ms/fwd {v[0] / tot * 100:5.1f}%")
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(rows, open(args.json, "w"), indent=1)
