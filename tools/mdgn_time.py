"""MDGN (team 24) timing (development helper, not the bench: bench.py has no MDGN entry): ms per forward and images/s of bf16 / fp16 forwards at
32 x 256 x 256 and one 339 x 510 image in the four combinations of fuse_conv_prelu and fuse_mdsa_gate, and fp32 -- four instances of the model
in ONE process, their repeats INTERLEAVED (every form once, then the next repeat), so that all forms meet the same GPU in the same minute and
the spread between repeats is the yardstick for their differences.  Each fused kernel is measured against the per-layer form, which runs only
kernels older than this network (conv_s16_kernel and its 64 -> 64 variants, prelu_kernel).  Then the per-launch report (enable_profiling):
every kernel's time per forward, and for the block's layers -- conv + prelu or esr_conv_prelu; fuse 1x1 + prelu + gate or esr_mdsa_gate --
the stored bytes per pixel from cost(), the achieved bytes/s against the copy bandwidth esr_bw_probe measures, and against the byte floors
(256 B per pixel for a 3x3 with its activation, 640 for the end of the block).
Random weights are not used: the checkpoint fixture of tests/golden/; the inputs are in 0 .. 255, the network's data_range.
usage: mdgn_time.py [--steps N] [--repeats R] [--json OUT]"""
import argparse, collections, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safetensors.torch import load_file
from ntire2022_esr_amd import MDGN, _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
gold = os.path.join(REPO, "tests", "golden")
sd = load_file(os.path.join(gold, "team24_mdgn.safetensors"))
sd.update(load_file(os.path.join(gold, "team24_mdgn.part2.safetensors")))
FORMS = {"per-layer": (False, False), "conv_prelu": (True, False), "mdsa_gate": (False, True), "both": (True, True)}
FLOOR = {"pair": 256.0, "tail": 640.0}                    # bytes per pixel in 16-bit storage that the layer cannot do without
models = {}
for form, (cp, mg) in FORMS.items():
    m = MDGN()
    m.load_state_dict(sd, strict=True)
    m.fuse_conv_prelu, m.fuse_mdsa_gate = cp, mg
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


def part(o):
    """which part of an MDSA block an op of the profile belongs to: 'pair' (f{j}.0 / f{j}.1), 'tail' (conv_fuse.*, sa.0), or None"""
    name = o["name"].split(".")
    if name[0] != "B":
        return None
    return "pair" if name[2] in ("f1", "f2", "f3") else "tail"


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
    parts = {"pair": [0.0, 0.0], "tail": [0.0, 0.0]}           # ms per forward, stored bytes per forward
    n_launch = 0
    for o in m.collect_profile():
        a = agg[o["kernel"]]
        a[0] += o["ms_sum"] / 3
        a[1] += o["passes"] // 3
        k = part(o)
        if k is not None:
            parts[k][0] += o["ms_sum"] / 3
            parts[k][1] += o["stored_bytes"]
        n_launch += 1
    m.disable_profiling()
    return agg, parts, n_launch


for comp in ("bf16", "f16", "f32"):
    forms = {f: m for f, m in models.items() if comp != "f32" or f == "per-layer"}      # (an fp32 plan has the per-layer form only)
    for m in forms.values():
        m.set_compute(comp)
    for B, h, w in ((32, 256, 256), (1, 339, 510)):
        x = torch.rand(B, 3, h, w, device=dev) * 255.0
        npix = float(B * h * w)
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
                agg, parts, n_launch = breakdown(m, x)
                ts = times[form]
                ms = min(ts)
                row = dict(compute=comp, form=form, batch=B, h=h, w=w, ms_per_forward=ms, ms_repeats=ts, images_per_s=B / ms * 1e3, ops=n_launch,
                           hbm_copy_kernel_gbs=copy_gbs, kernels={k: round(v[0], 4) for k, v in agg.items()})
                text = []
                for k, (p_ms, p_bytes) in parts.items():
                    n_layers = 12 if k == "pair" else 4
                    p_gbs = p_bytes / (p_ms * 1e-3) / 1e9 if p_ms else 0.0
                    floor_gbs = FLOOR[k] * n_layers * npix / (p_ms * 1e-3) / 1e9 if (p_ms and comp != "f32") else 0.0
                    row[k] = dict(ms=p_ms, stored_bytes_per_pixel=p_bytes / npix / n_layers, gbs=p_gbs, floor_gbs=floor_gbs)
                    text.append(f"{k} {p_ms:.4f} ms/fwd, {p_bytes / npix / n_layers:.0f} B/pixel stored at {p_gbs:.0f} GB/s ({p_gbs / copy_gbs * 100:.0f} % of the copy "
                                f"bandwidth), the byte floor at {floor_gbs:.0f} GB/s")
                rows.append(row)
                print(f"{comp:4s} {form:10s} {B:2d} x {h} x {w}: min {ms:8.3f} ms/fwd (repeats {', '.join(f'{t:.3f}' for t in ts)}; "
                      f"spread {(max(ts) - min(ts)) / min(ts) * 100:.1f} %) {B / ms * 1e3:8.1f} img/s, {n_launch} ops; " + "; ".join(text), flush=True)
                tot = sum(v[0] for v in agg.values())
                for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])[:8]:
                    print(f"      {k:60s} {v[1]:3d} launches/fwd {v[0]:8.3f} ms/fwd {v[0] / tot * 100:5.1f}%")
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(rows, open(args.json, "w"), indent=1)
