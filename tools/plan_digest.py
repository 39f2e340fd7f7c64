"""Digest of every plan the networks build (no GPU): one line per (model, storage, flags, N x H x W) with len(plan.ops), plan.total,
plan.total_lo and a SHA-256 over the finalized Op array and the buffer table, and per (model, storage, flags) one line with a SHA-256 over the
packed weight blobs and one (`costs`) with a SHA-256 over the cost entries of the ops of all those plans (HipSRModel.op_costs: names, kernel
strings, flops and bytes of the benchmark's roofline leg) and their complexity terms (the model summary's counters).  Weights are the constructor's under torch.manual_seed(0); plans are finalized against the fixed base
(0x10000000, plan.total) and blob addresses 4096 * (1 + rank of the name in sorted(model._packed)); a blob name that _packed does not hold
raises.  Two trees whose outputs are equal launch the same descriptors: run it before and after a change to the plan builders and diff
(tests/golden/plan_digests_14_networks.txt holds the output, of all the networks by now; tests/test_plan_digest.py compares).
usage: plan_digest.py [--models NAME,...] > digest.txt"""
import argparse, contextlib, hashlib, io, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ntire2022_esr_amd as pkg
from ntire2022_esr_amd import _lib as L
from ntire2022_esr_amd.engine import Plan

R, M = pkg.RFDN, pkg.IMDN


def _resdn():
    """ResDN with the 3x3 identity in both MeanShift weights, which its packing insists on; the biases keep their seeded values"""
    m = pkg.ResDN()
    with torch.no_grad():
        for name in ("sub_mean", "add_mean"):
            m._leaf(name).weight.copy_(torch.eye(3)[:, :, None, None])
    return m


MODELS = {          # name -> (constructor, the flags its plans read besides hilo_skip (bf16 plans) and winograd (fp32 plans))
    "IMDN": (M, ()), "IMDN_nb7": (lambda: M(nb=7, act_mode='L'), ()), "IMDN_nc32": (lambda: M(nc=32), ()),
    "RFDN": (R, ("fuse_esa_lowres", "tight_pitch", "fuse_tail")), "RFDN_nf40": (lambda: R(nf=40), ("fuse_esa_lowres", "tight_pitch", "fuse_tail")),
    "RFDN_sfdn": (lambda: R(block_residual=False, esa_conv_f=False), ("fuse_esa_lowres", "tight_pitch", "fuse_tail")),
    "RFDN_pruned": (lambda: R(nf=40, block_residual=False, esa_f=12), ("fuse_esa_lowres", "tight_pitch", "fuse_tail")),
    "RLFN_cut": (pkg.RLFN_cut, ("fuse_esa_lowres", "fuse_chain")), "BSRN": (lambda: pkg.BSRN(num_feat=48, num_block=5), ("fuse_esa_lowres", "fuse_tail")),
    "FMEN": (pkg.FMEN, ("tight_pitch", "fuse_hfab")), "PLAINRFDN": (pkg.PLAINRFDN, ("fuse_esa_lowres",)),
    "BMDN": (pkg.BMDN, ("fuse_esa_lowres", "tight_pitch", "fuse_step")), "ESAN": (pkg.ESAN, ("fuse_esa_lowres", "fuse_head")),
    "FasterRFDN": (pkg.FasterRFDN, ("fuse_esa_lowres", "fuse_cascade")), "RFDNeXt": (pkg.RFDNeXt, ("tight_pitch", "fuse_cx")),
    "DWRFDN": (pkg.DWRFDN, ("tight_pitch", "fuse_pair")), "RePAFDN": (pkg.RePAFDN, ("fuse_esa_lowres", "fuse_pa_tail")),
    "ARFDN": (pkg.ARFDN, ("fuse_esa_lowres", "tight_pitch", "fuse_asym")),
    "ResDN": (_resdn, ("fuse_esa_lowres", "fuse_resdb")), "MDGN": (pkg.MDGN, ("fuse_conv_prelu", "fuse_mdsa_gate")),
}
# 32 x 256 x 256 crosses the 256-tile threshold of the fused tails; at 3400 x 3400 (nothing is allocated) some fused kernels refuse the shape
# and the plan keeps the per-op form (MDGN's 16-bit plans: 32 ops instead of 20), so the blobs of a fallback form are read too
SHAPES = ((1, 15, 16), (2, 45, 70), (1, 339, 510), (32, 256, 256), (1, 3400, 3400))


class Blob:
    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


class Blobs:
    """stands in for model._packed in Plan.finalize: every name of it at a fixed address, any other name raises"""
    def __init__(self, names):
        self.at = {n: Blob(4096 * (1 + i)) for i, n in enumerate(sorted(names))}

    def __getitem__(self, name):
        return self.at[name]

    def __contains__(self, name):
        return name in self.at

    def get(self, name, default=None):
        return self.at.get(name, default)


def build(name, store, flip=None):
    """the model `name` with the constructor's weights, packed for `store` on the CPU, with the flag `flip` inverted"""
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):     # (BSRN prints its conv type, as the reference does)
        m = MODELS[name][0]()
    m.compute = store
    if flip:
        setattr(m, flip, not getattr(m, flip))
    m._repack("cpu")
    return m


def plan_digest(m, shape, names=None, costs=None):
    """(len(ops), total, total_lo, sha256) of the plan of `m` for shape = (N, H, W); names: the blob names (default: m._packed's); costs: a
    hashlib object that takes the plan's cost entries and complexity terms"""
    plan = Plan(*shape, m._store())
    m._build_plan(plan, m.in_nc)
    arr, _, _ = plan.finalize((0x10000000, plan.total), Blobs(m._packed if names is None else names))
    h = hashlib.sha256(bytes(arr))
    h.update(repr([(b.pitch, b.offset, b.h, b.w, b.esize, b.arena, b.blocked) for b in plan.buffers]).encode())
    if costs is not None:
        costs.update(repr(m.op_costs(plan, arr)).encode() + repr([m._complexity_terms(plan, o) for o in plan.ops]).encode())
    return len(plan.ops), plan.total, plan.total_lo, h.hexdigest()


def packed_digest(m):
    h = hashlib.sha256()
    for n in sorted(m._packed):
        t = m._packed[n].contiguous()
        h.update(repr((n, tuple(t.shape), str(t.dtype))).encode() + t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def cells(models=None):
    """(model name, storage, flipped flag or None) of every cell: the defaults and each flag the plans of that storage read, inverted"""
    for name in models or MODELS:
        for store in ("f32", "bf16", "f16"):
            # (of the models' own flags only fuse_esa_lowres shapes an fp32 plan)
            flags = [None] + [f for f in MODELS[name][1] if store != "f32" or f == "fuse_esa_lowres"]
            flags += ["hilo_skip"] * (name != "ESAN" and store == "bf16") + ["winograd"] * (store == "f32")
            for flip in flags:
                yield name, store, flip


def cell_lines(name, store, flip, names=None):
    """(the built model or None, the output lines) of one cell; names: see plan_digest"""
    cell = f"{name} {store} {flip or 'defaults'}"
    try:
        m = build(name, store, flip)
    except L.EsrError as e:                             # (FMEN refuses fp16 storage)
        return None, [f"{cell} refused: {e}"]
    lines, costs = [f"{cell} packed {len(m._packed)} {packed_digest(m)}"], hashlib.sha256()
    for shape in SHAPES:
        try:
            lines.append(" ".join([f"{cell} {'x'.join(map(str, shape))}"] + [str(v) for v in plan_digest(m, shape, names, costs)]))
        except L.EsrError as e:
            lines.append(f"{cell} {'x'.join(map(str, shape))} refused: {e}")
    return m, lines + [f"{cell} costs {costs.hexdigest()}"]


def arrange(per_cell):
    """The tool's output from the cells' lines: first every cell's `packed` line and first four shapes, in the places they have had since the
    fixture was first recorded, then every cell's later additions -- the largest shape and `costs` (a cell that refused has its one line)"""
    cut = lambda lines: max(len(lines) - 2, 1)
    return [l for lines in per_cell for l in lines[:cut(lines)]] + [l for lines in per_cell for l in lines[cut(lines):]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(MODELS))
    print("\n".join(arrange([cell_lines(*cell)[1] for cell in cells(ap.parse_args().models.split(","))])))


if __name__ == "__main__":
    main()
