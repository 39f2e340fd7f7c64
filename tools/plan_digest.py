"""Digest of every plan the networks build (no GPU): one line per (model, storage, flags, N x H x W) with len(plan.ops), plan.total,
plan.total_lo and a SHA-256 over the finalized Op array and the buffer table, and one line per (model, storage, flags) with a SHA-256 over
the packed weight blobs.  Weights are the constructor's under torch.manual_seed(0); plans are finalized against the fixed base
(0x10000000, plan.total) and blob addresses 4096 * (1 + rank of the name in sorted(model._packed)); a blob name that _packed does not hold
raises.  Two trees whose outputs are equal launch the same descriptors: run it before and after a change to the plan builders and diff.
usage: plan_digest.py [--models NAME,...] > digest.txt"""
import argparse, contextlib, hashlib, io, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ntire2022_esr_amd as pkg
from ntire2022_esr_amd import _lib as L
from ntire2022_esr_amd.engine import Plan

R, M = pkg.RFDN, pkg.IMDN
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
    "ResDN": (pkg.ResDN, ("fuse_esa_lowres", "fuse_resdb")),
}
SHAPES = ((1, 15, 16), (2, 45, 70), (1, 339, 510), (32, 256, 256))      # the last one crosses the 256-tile threshold of the fused tails


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


def plan_digest(m, shape, names=None):
    """(len(ops), total, total_lo, sha256) of the plan of `m` for shape = (N, H, W); names: the blob names (default: m._packed's)"""
    plan = Plan(*shape, m._store())
    m._build_plan(plan, m.in_nc)
    arr, _, _ = plan.finalize((0x10000000, plan.total), Blobs(m._packed if names is None else names))
    h = hashlib.sha256(bytes(arr))
    h.update(repr([(b.pitch, b.offset, b.h, b.w, b.esize, b.arena, b.blocked) for b in plan.buffers]).encode())
    return len(plan.ops), plan.total, plan.total_lo, h.hexdigest()


def packed_digest(m):
    h = hashlib.sha256()
    for n in sorted(m._packed):
        t = m._packed[n].contiguous()
        h.update(repr((n, tuple(t.shape), str(t.dtype))).encode() + t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(MODELS))
    for name in ap.parse_args().models.split(","):
        for store in ("f32", "bf16", "f16"):
            # (of the models' own flags only fuse_esa_lowres shapes an fp32 plan)
            flags = [None] + [f for f in MODELS[name][1] if store != "f32" or f == "fuse_esa_lowres"]
            flags += ["hilo_skip"] * (name != "ESAN" and store == "bf16") + ["winograd"] * (store == "f32")
            for flip in flags:
                cell = f"{name} {store} {flip or 'defaults'}"
                try:
                    m = build(name, store, flip)
                except L.EsrError as e:                 # (FMEN refuses fp16 storage)
                    print(f"{cell} refused: {e}")
                    continue
                print(f"{cell} packed {len(m._packed)} {packed_digest(m)}")
                for shape in SHAPES:
                    try:
                        print(f"{cell} {'x'.join(map(str, shape))}", *plan_digest(m, shape))
                    except L.EsrError as e:
                        print(f"{cell} {'x'.join(map(str, shape))} refused: {e}")


if __name__ == "__main__":
    main()
