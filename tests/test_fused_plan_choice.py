"""CPU: a plan fuses a run of convolutions into one op (engine.Chain / Distill / ResHead) exactly where the kernel's own predicate takes the
descriptor the plan will launch -- asked by Plan._fuse when the plan is built, never mirrored by hand in a model.  Where the predicate
refuses, the plan keeps the per-op form instead of raising at finalize.  No GPU: plans are finalized against a fake workspace address."""
import ctypes

import pytest

# op kind -> (the C ABI's predicate, the esr_op member it reads)
PREDICATE = {"chain": ("esr_conv_chain_supported", "chain"), "distill": ("esr_distill_step_supported", "chain"),
             "reshead": ("esr_resblock_head_supported", "conv")}


def _models():
    from ntire2022_esr_amd import BMDN, ESAN, FMEN, RLFN_cut
    fmen = FMEN()
    fmen.fuse_hfab = True                         # (off by default: DESIGN.md, FMEN)
    return {"rlfn": (RLFN_cut(), "chain", 4), "fmen": (fmen, "chain", 4), "bmdn": (BMDN(), "distill", 12), "esan": (ESAN(), "reshead", 16)}


@pytest.fixture(scope="module")
def packed():
    """name -> (bf16 model with its blobs packed on the host, kind of its fused op, how many a plan has)"""
    ms = _models()
    for m, _, _ in ms.values():
        m.set_compute("bf16")
        m._repack("cpu")
    return ms


def _finalized(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    return plan, arr


@pytest.mark.parametrize("name", ["rlfn", "fmen", "bmdn", "esan"])
def test_every_fused_op_satisfies_its_own_predicate(packed, name):
    from ntire2022_esr_amd import _lib as L
    m, kind, count = packed[name]
    plan, arr = _finalized(m, 2, 45, 70)
    fused = [(o, arr[i]) for i, o in enumerate(plan.ops) if o.kind in PREDICATE]
    assert [o.kind for o, _ in fused] == [kind] * count
    for o, op in fused:
        fn, field = PREDICATE[o.kind]
        assert getattr(op, field).n == 2
        assert getattr(L.lib(), fn)(ctypes.byref(getattr(op, field))) == 1, (name, o.replaces[0].w)
    # the batch plays no part in the choice
    kinds = [[o.kind for o in _finalized(m, n, 45, 70)[0].ops] for n in (1, 8)]
    assert kinds[0] == kinds[1] == [o.kind for o in plan.ops]


def test_rlfn_keeps_the_per_op_form_where_the_chain_kernel_refuses(packed):
    """1 x 3400 x 3400 in bf16: the largest tensor of an image is 3400 * 3400 * 48 * 2 bytes, over the 1 GiB the chain kernel addresses.  The
    hand-written condition this replaces said yes and the plan raised at finalize; nothing is allocated here."""
    m = packed["rlfn"][0]
    assert 3400 * 3400 * 48 * 2 > 1 << 30
    plan, arr = _finalized(m, 1, 3400, 3400)
    assert not any(o.kind == "chain" for o in plan.ops)
    c3 = [o for o in plan.ops if o.kind == "conv" and o.w.endswith(".c3_r")]
    assert [o.w for o in c3] == [f"B{k}.c3_r" for k in range(1, 5)]
    for k, o in enumerate(c3, 1):                 # c5 and esa.conv1 still ride in c3_r's epilogue
        assert o.dst is None and (o.post.w, o.post.post2.w) == (f"B{k}.c5", f"B{k}.esa.conv1")
    ws = [o.w for o in plan.ops if o.kind == "conv"]
    assert all(ws.index(f"B{k}.c1_r") + 2 == ws.index(f"B{k}.c2_r") + 1 == ws.index(f"B{k}.c3_r") for k in range(1, 5))
    # the same model at a DIV2K shape fuses all four blocks
    plan, _ = _finalized(m, 1, 339, 510)
    chains = [o for o in plan.ops if o.kind == "chain"]
    assert len(chains) == 4 and [[c.w for c in o.replaces] for o in chains] == [[f"B{k}.c{j}_r" for j in (1, 2, 3)] for k in range(1, 5)]
    assert not any(o.kind == "conv" and o.w.endswith(("c1_r", "c2_r", "c3_r")) for o in plan.ops)


@pytest.mark.parametrize("esdb", [False, True])
def test_the_tail_predicate_refuses_a_3x3_of_one_output_tile(esdb):
    """rfdb_tail_kernel reads the 3x3's weights from the 32x32x16 image behind the blob's bias, which esr_pack_conv_s16 emits for two output tiles
    (17 .. 32 outputs) at three and four chunks and not for one: the descriptor of tests/test_gpu_c64m.py's tail cases (4 x 128 x 144, nf = 50 |
    48, f = 16; no pointer is read) is taken with 17, 25 and 32 outputs and refused with 16 and 1 -- as with 33."""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    nf, cp = (48, 48) if esdb else (50, 64)
    a = 0x10000000                                # (any non-null 16-byte-aligned addresses)

    def desc(dc):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.ksize = 4, 128, 144, nf, dc, 3
        d.in_layout = d.out_layout = L.NHWC
        d.storage = d.compute = L.STORE["bf16"]
        d.act, d.slope = L.ACT_NONE, 0.05
        d.inp = L.View(ctypes.c_void_p(a), cp, 0)
        d.out0 = L.View(ctypes.c_void_p(a + (1 << 24)), cp, 0)
        d.wpacked, d.tail_wpacked, d.post_wpacked = (ctypes.c_void_p(a + (k << 26)) for k in (1, 2, 3))
        d.tail_cat = L.View(ctypes.c_void_p(a + (2 << 24)), 32, 0)
        d.tail_cat_c, d.tail_cout, d.tail_mid_act = 96, nf, (L.ACT_GELU if esdb else L.ACT_LRELU)
        d.tail_seg_stride16 = 4 * 128 * 144 * 32 * 2 // 16
        d.post_out = L.View(ctypes.c_void_p(a + (3 << 24)), 16, 0)
        d.post_cout, d.post_act = 16, L.ACT_NONE
        if esdb:
            d.border_bias = ctypes.c_void_p(a + (4 << 26))
        return d

    assert [lib.esr_conv_tail_supported(ctypes.byref(desc(dc))) for dc in (1, 16, 17, 25, 32, 33)] == [0, 0, 1, 1, 1, 0]
    # the packer's side of the same fact: the blob of a one-tile 3x3 is the tap-pair image and the bias, nothing behind them
    for dc, image in ((16, 0), (17, (3 if esdb else 4) * 9 * 1024), (32, (3 if esdb else 4) * 9 * 1024)):
        assert lib.esr_packed_conv_s16_bytes(cp, dc, 3) == (cp // 16) * 5 * ((dc + 15) // 16) * 1024 + ((dc + 15) // 16) * 64 + image
