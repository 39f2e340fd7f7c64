"""The walk table of tests/_walk_cases.py, checked without a GPU: every batch is more than four rounds of its kernel's grid (two for
the group walkers) and no whole number of them, every chunk of the walk == no walk check is at most one round, and along every block's
walk no two consecutive work items are the same tile of the same base image -- a tile computed from the previous tile's staged data would
otherwise show the right values.  The work-item counts restate the launchers' arithmetic (_walk_cases.items); a later edit of the table
cannot silently shrink a batch below the walk it is there for."""
import pytest

import _persist_cases as P
import _walk_cases as W

ROWS = [pytest.param(f, hw, n, id=f"{f['id']}-{hw[0]}x{hw[1]}") for f, c, hw, n in W.rows() if c == "bf16"]      # (the storage changes no count)


def test_table_covers_every_kernel_and_storage():
    assert {f["kernel"] for f in W.FORMS} == set(W.KERNELS) and len(W.KERNELS) == 13
    ids = [f["id"] for f in W.FORMS]
    assert len(ids) == len(set(ids))
    symbols = [W.symbol(f, c) for f in W.FORMS for c in f["storages"]]
    assert len(symbols) == len(set(symbols))                                   # one form per instantiation
    for f in W.FORMS:
        assert f["storages"] == ("bf16", "f16")
        assert all(W.symbol(f, c).startswith(f["kernel"] + "<") for c in f["storages"])
    # every kernel has exactly one main instantiation (all its shapes); the others run the first shape only
    for k in W.KERNELS:
        forms = [f for f in W.FORMS if f["kernel"] == k]
        mains = [f for f in forms if len(f["shapes"]) == 3 or f["unit"] == "g16"]
        assert len(mains) == (2 if k == "rlfb_chain_kernel" else 1), k         # (both strip widths are RLFN's own)
        assert all(f["shapes"] == W.SHAPES[:1] for f in forms if f not in mains)
    # the shapes: two of test_network_on_300_thin_images' and the largest of the thin-batch table -- one to four tiles across, one to three
    # down, a single live row (17, 33) or column (33, 49) in the last tile, a change of image at least every 12 tiles
    assert W.SHAPES == [(17, 15), (16, 33), (33, 49)] and W.SHAPES[2] in P.SHAPES
    assert {(w + 15) // 16 for _, w in W.SHAPES} == {1, 3, 4} and {(h + 15) // 16 for h, _ in W.SHAPES} == {1, 2, 3}
    assert {h % 16 for h, _ in W.SHAPES} >= {0, 1} and {w % 16 for _, w in W.SHAPES} >= {1, 15}
    assert max(P.tiles_per_image(hw, "t16") for hw in W.SHAPES) == 12
    # the template arguments that change the staging, each value in some form
    assert {W.symbol(f, "bf16") for f in W.FORMS} >= {
        "rlfb_chain_kernel<true, 2>", "rlfb_chain_kernel<true, 3>", "hfab_kernel<true, 3>", "hfab_kernel<true, 4>",
        "distill_step_kernel<true, 3, false>", "distill_step_kernel<true, 2, true>", "distill_step_kernel<true, 2, false>",
        "resblock_head_kernel<true, true>", "resblock_head_kernel<true, false>", "pa_tail_kernel<true, 3>", "pa_tail_kernel<true, 4>",
        "asym_step_kernel<true, 2, false>", "asym_step_kernel<true, 1, true>", "asym_step_kernel<true, 1, false>",
        *[f"resdb_step_kernel<true, {nx}, {nd}>" for nx in (0, 1, 2) for nd in (1, 2, 3)]}


def test_tile_walkers_have_the_issues_batches():
    sizes = {hw: n for f, c, hw, n in W.rows() if f["unit"] == "t16"}
    assert sizes == {(17, 15): 514, (16, 33): 343, (33, 49): 87}
    assert sorted(n * P.tiles_per_image(hw, "t16") for hw, n in sizes.items()) == [1028, 1029, 1044]


@pytest.mark.parametrize("form,hw,n", ROWS)
def test_batch_walks_and_every_chunk_does_not(form, hw, n):
    total, rnd = W.items(form, hw, n), form["round"]
    assert total > form["rounds"] * rnd and total % rnd != 0
    assert W.items(form, hw, n - 2) <= form["rounds"] * rnd                    # the smallest such batch, plus one image
    assert n >= 2 * form["period"]                                            # images 0 .. 2 and the last three are six images
    if form["unit"] == "g16":
        assert n * hw[0] * hw[1] % 16 != 0                                     # the last group is a partial one
    bounds = W.chunks(form, hw, n)
    assert bounds[0][0] == 0 and bounds[-1][1] == n and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    assert all(0 < W.items(form, hw, hi - lo) <= rnd for lo, hi in bounds)
    # the walks: together every item once; each as long as the rounds; no two consecutive items alike
    lanes = min(total, rnd)
    walks = [W.walk_of(form, hw, n, lane) for lane in range(lanes)]
    assert sorted(i for w in walks for i in w) == list(range(total))
    assert min(len(w) for w in walks) == form["rounds"] and max(len(w) for w in walks) == form["rounds"] + 1
    for w in walks:
        keys = [W.item_key(form, hw, n, i) for i in w]
        assert all(a != b for a, b in zip(keys, keys[1:])), (w, keys)


def test_chain_geometry_restates_the_launchers_choice():
    """a strip is 16 G - 4 columns wide; one row segment is the cheapest on a batch this large (every further segment adds six halo rows to
    every job), so a job is one strip of one image"""
    for g, ws in ((2, 28), (3, 44)):
        for h, w in W.SHAPES:
            assert W.chain_geometry(2000, h, w, g) == ((w + ws - 1) // ws, 1)
    assert W.chain_geometry(1, 96, 61, 2)[1] > 1                               # (a single image is cut into segments)
