"""CPU-only: the rules that the fused launchers share, pinned at their edges for every one of them, as one table.

Four rules, each stated once in csrc/esr_internal.h and asked by many predicates and launchers:
    storage / compute   16-bit storage with the operand type equal to it (esr_s16_pair); esr_pa_gate and esr_prelu take fp32 / fp32 as well
    1 GiB               one image of a tiled view stays below 2^30 bytes (esr_image_below_1g)
    count               the 16 x 16 tiles (esr_tiles), the pixels or the jobs of a launch stay below 2^31 - 1
    overlap             what a launch writes shares no byte with what it reads: whole tensors (esr_bytes_overlap) or views (esr_views_meet)
A row is a descriptor, what the predicate answers and what the launcher answers.  The baselines are the other test files' own builders.

Nothing is allocated and nothing is launched on a GPU: the addresses are stand-ins.  A descriptor that the launcher refuses (-1 / -2) is
passed to it everywhere; one that it would accept only where there is no device, where it passes every check and fails in the launch
(ESR_ERR_LAUNCH), as check_refusals of tests/_arfdn.py does.  With a device those rows ask the predicate alone."""
import ctypes

import pytest
import torch

import _arfdn
import test_bmdn
import test_dwrfdn
import test_esan
import test_frfdn
import test_mdgn
import test_repafdn
import test_resdn
import test_rfdnext
import test_view_validation
from ntire2022_esr_amd import _lib as L

BAD_ARG, UNSUPPORTED, LAUNCH = -1, -2, -3
OK = "ok"                                    # the launcher accepts: asked only without a device, where it answers LAUNCH
GIB, INDEX_LIMIT = 1 << 30, (1 << 31) - 1
F32, BF16, F16 = L.STORE["f32"], L.STORE["bf16"], L.STORE["f16"]
_BUF = (ctypes.c_float * 8192)()
A = ctypes.addressof(_BUF)
S = 1 << 20
VIEWS = ("inp", "res", "out0", "out1", "tail_cat", "post_out", "post2_out")
FAR = 1 << 54                                # between the stand-in tensors of a row with a huge image or batch: more than any of them holds


def _resdb():
    """a ResDB step with one distilled output and no extra input (tests/test_resdn.py holds the predicate to its shapes; it has no pointers)"""
    d = L.ConvDesc()
    d.n, d.h, d.w, d.ksize, d.cin, d.cout, d.post_cout = 1, 4, 4, 3, 48, 48, 16
    d.in_layout = d.out_layout = L.NHWC
    d.storage = d.compute = BF16
    d.inp, d.out0, d.post_out = L.View(A, 48, 0), L.View(A + S, 48, 0), L.View(A + 2 * S, 16, 0)
    d.wpacked = d.post_wpacked = d.tail_wpacked = A
    return d


# name -> predicate, launcher, baseline, and what the launcher's rules are:
#   f32      fp32 / fp32 is accepted too
#   gib      the views the predicate holds below 1 GiB per image (a view behind the first is widened 8 x, so that it alone decides)
#   count    (what is counted, who refuses): "tiles" of 16 x 16, "pixels", or esr_conv_chain's "jobs" (n at 4 x 1); "sup": the predicate says 0
#            and the launcher UNSUPPORTED, "run": the predicate does not look and the launcher answers UNSUPPORTED
#   overlap  ("bytes", output, inputs): whole tensors; ("views", output, input, channels read from the input, element size): esr_views_meet
#   hmin     the smallest h the predicate takes
ENTRIES = {
    "pa_gate": dict(sup="esr_pa_gate_supported", run="esr_pa_gate", base=lambda: test_repafdn._gate_desc(L, A), f32=True,
                    count=("pixels", "sup"), overlap=("bytes", "out0", ("inp", "res"))),
    "pa_tail": dict(sup="esr_pa_tail_supported", run="esr_pa_tail", base=lambda: test_repafdn._gate_desc(L, A, ksize=3, tail_wpacked=A),
                    gib=("inp",), count=("tiles", "sup"), overlap=("bytes", "out0", ("inp", "res"))),
    "conv_prelu": dict(sup="esr_conv_prelu_supported", run="esr_conv_prelu", base=lambda: test_mdgn._conv_desc(L), gib=("inp",),
                       count=("tiles", "sup"), overlap=("views", "out0", "inp", 64, 2)),
    "mdsa_gate": dict(sup="esr_mdsa_gate_supported", run="esr_mdsa_gate", base=lambda: test_mdgn._gate_desc(L, planar=False),
                      count=("pixels", "sup"), overlap=("bytes", "out0", ("inp", "res"))),
    "mdsa_gate_planar": dict(sup="esr_mdsa_gate_supported", run="esr_mdsa_gate", base=lambda: test_mdgn._gate_desc(L, planar=True),
                             count=("pixels", "sup")),
    "asym_step": dict(sup="esr_asym_step_supported", run="esr_asym_step", base=lambda: _arfdn.step_desc(L, A), gib=("inp",),
                      count=("tiles", "sup"), overlap=("views", "out0", "inp", 32, 2)),
    "prelu": dict(sup="esr_prelu_supported", run="esr_prelu", base=lambda: test_resdn._desc(L, "bf16", (41,)), f32=True,
                  overlap=("views", "out0", "inp", 41, 2)),
    "prelu_f32": dict(sup="esr_prelu_supported", run="esr_prelu", base=lambda: test_resdn._desc(L, "f32", (41,)), f32=True,
                      overlap=("views", "out0", "inp", 41, 4)),
    "resdb_step": dict(sup="esr_resdb_step_supported", run="esr_resdb_step", base=_resdb, count=("tiles", "sup"),
                       overlap=("views", "out0", "inp", 48, 2)),
    "cx_block": dict(sup="esr_cx_block_supported", run="esr_cx_block_s16", base=lambda: test_rfdnext._cx_desc(L, A), gib=("inp",),
                     count=("tiles", "sup")),
    "dwpw_pair": dict(sup="esr_dwpw_pair_supported", run="esr_dwpw_pair_s16", base=lambda: test_dwrfdn._pair_desc(L, A), gib=("inp",),
                      count=("tiles", "sup")),
    "refine_cascade": dict(sup="esr_refine_cascade_supported", run="esr_refine_cascade_s16", base=lambda: test_frfdn._casc_desc(L, A),
                           gib=("inp",), count=("tiles", "sup")),
    "distill_step": dict(sup="esr_distill_step_supported", run="esr_distill_step_s16", base=lambda: test_bmdn._step_desc(L, A), gib=("inp",),
                         count=("tiles", "run")),
    "resblock_head": dict(sup="esr_resblock_head_supported", run="esr_resblock_head_s16", base=lambda: test_esan._head_desc(L, A),
                          gib=("inp", "res"), count=("tiles", "sup")),
    "hfab": dict(sup="esr_conv_chain_supported", run="esr_conv_chain_s16", base=lambda: test_view_validation._chain(True), gib=("inp",),
                 count=("tiles", "run")),
    "chain": dict(sup="esr_conv_chain_supported", run="esr_conv_chain_s16", base=lambda: test_view_validation._chain(False),
                  gib=("inp", "post_out", "post2_out"), count=("jobs", "run"), hmin=4),
}


def _spread(d):
    """every tensor of the descriptor FAR from every other, so that a huge image or batch makes no two of them meet"""
    for k, name in enumerate(VIEWS):
        v = getattr(d, name, None)
        if v is not None and v.ptr:
            v.ptr = FAR * (k + 1)
    return d


def _edit(e, **kw):
    d = _spread(e["base"]())
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _storage_rows(e):
    for st in (BF16, F16) + ((F32,) if e.get("f32") else ()):
        yield f"storage:{st}/{st}", lambda st=st: _edit(e, storage=st, compute=st), 1, OK
    mixed = [(BF16, F16), (F16, BF16), (F32, BF16), (BF16, F32), (F32, F16), (F16, F32), (3, 3), (-1, -1), (3, BF16), (BF16, 3)]
    for st, co in mixed + ([] if e.get("f32") else [(F32, F32)]):
        yield f"storage:{st}/{co}", lambda st=st, co=co: _edit(e, storage=st, compute=co), 0, UNSUPPORTED


def _gib_rows(e):
    """n = 1 and one row of pixels (hmin rows): the largest w whose image of this view stays below 2^30 bytes, and the next"""
    h = e.get("hmin", 1)
    for i, name in enumerate(e.get("gib", ())):
        def make(extra, name=name, i=i):
            d = _edit(e, n=1, h=h)
            v = getattr(d, name)
            if i:
                v.pitch *= 8
            d.w = (GIB - 1) // (2 * v.pitch * h) + extra
            assert (d.h * d.w * v.pitch * 2 < GIB) == (extra == 0) and d.h * (d.w - extra) * v.pitch * 2 + 2 * v.pitch * h >= GIB
            return d
        yield f"gib:{name}:below", lambda make=make: make(0), 1, OK
        yield f"gib:{name}:reached", lambda make=make: make(1), 0, UNSUPPORTED


def _count_rows(e):
    """small images and a large batch: the last count below 2^31 - 1 and the first one at or above it"""
    if "count" not in e:
        return
    what, who = e["count"]
    # (h, w, the units of one image): a single unit, where n is the count, and an image whose edges are no multiple of the tile
    shapes = {"tiles": [(1, 16, 1), (17, 33, 6)], "pixels": [(1, 1, 1), (3, 5, 15)], "jobs": [(4, 1, 1)]}[what]
    for h, w, per in shapes:
        n = (INDEX_LIMIT - 1) // per
        assert n * per < INDEX_LIMIT <= (n + 1) * per
        yield f"count:{h}x{w}:below", lambda n=n, h=h, w=w: _edit(e, n=n, h=h, w=w), 1, OK
        yield f"count:{h}x{w}:reached", lambda n=n, h=h, w=w: _edit(e, n=n + 1, h=h, w=w), 0 if who == "sup" else 1, UNSUPPORTED


def _overlap_rows(e):
    if "overlap" not in e:
        return
    kind, out = e["overlap"][:2]
    es = e["overlap"][4] if kind == "views" else 2
    for name in (e["overlap"][2] if kind == "bytes" else (e["overlap"][2],)):
        def edge(short, name=name):
            """the output behind the input's tensor, or `short` pixels of the input's before its end"""
            d = _edit(e)
            i, o = getattr(d, name), getattr(d, out)
            o.ptr = i.ptr + (d.n * d.h * d.w - short) * i.pitch * es
            return d
        yield f"overlap:{name}:last-pixel", lambda edge=edge: edge(1), 1, BAD_ARG
        yield f"overlap:{name}:behind", lambda edge=edge: edge(0), 1, OK
    if kind != "views":
        return
    name, ic = e["overlap"][2:4]
    g = 16 // es
    adjacent = -(-ic // g) * g                          # the first granule behind the channels read

    def concat(coff, offset):
        """input and output as slices of one pitch-128 tensor: the input's channels from 0, the output's from coff"""
        d = _edit(e)
        i, o = getattr(d, name), getattr(d, out)
        i.pitch, i.coff = 128, 0
        o.ptr, o.pitch, o.coff = i.ptr + offset, 128, coff
        return d
    yield "overlap:concat:adjacent", lambda: concat(adjacent, 0), 1, OK
    # one granule lower: the output takes the input's last granule -- for esr_prelu, which reads 41 channels, exactly one channel of it
    yield "overlap:concat:shared", lambda: concat(adjacent - g, 0), 1, BAD_ARG
    yield "overlap:concat:not-a-whole-pixel", lambda: concat(adjacent, 16), 1, BAD_ARG


def _rows():
    for name, e in ENTRIES.items():
        yield f"{name}:baseline", e, e["base"], 1, OK
        for rows in (_storage_rows, _gib_rows, _count_rows, _overlap_rows):
            for rid, make, sup, run in rows(e):
                yield f"{name}:{rid}", e, make, sup, run


ROWS = list(_rows())


def test_every_launcher_and_rule_is_in_the_table():
    ids = [r[0] for r in ROWS]
    assert len(ids) == len(set(ids))
    for name, e in ENTRIES.items():
        assert {e["sup"], e["run"]} <= set(L.EXPORTS), name
        mine = [i for i in ids if i.startswith(name + ":")]
        assert sum(":storage:" in i for i in mine) >= 12
        assert sum(":gib:" in i for i in mine) == 2 * len(e.get("gib", ()))
        assert any(":count:" in i for i in mine) == ("count" in e) and any(":overlap:" in i for i in mine) == ("overlap" in e)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_rule_at_its_edge(row):
    rid, e, make, want_sup, want_run = row
    lib = L.lib()
    d = make()
    assert getattr(lib, e["sup"])(ctypes.byref(d)) == want_sup, rid
    if want_run != OK:
        assert getattr(lib, e["run"])(ctypes.byref(d), None) == want_run, rid
    elif torch.cuda.device_count() == 0:
        assert getattr(lib, e["run"])(ctypes.byref(d), None) == LAUNCH, rid
