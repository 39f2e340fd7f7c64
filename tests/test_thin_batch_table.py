"""The thin-batch table of tests/_persist_cases.py, checked without a GPU: the library's own shape query (esr_conv_block_waves, host-only) must
put every batch of the table on its form's kernel and every chunk of the bit-identity check on another one, and the sixteen shapes must cover
the row residues, widths and tile counts they are there for -- a later edit of the table cannot silently drop one."""
import ctypes

import pytest

import _persist_cases as P


def test_shapes_cover_heights_widths_and_tile_counts():
    assert len(P.SHAPES) == 16 and len(set(P.SHAPES)) == 16
    hs, ws = {h for h, _ in P.SHAPES}, {w for _, w in P.SHAPES}
    assert hs == {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33}
    assert ws == {1, 2, 15, 16, 17, 31, 32, 33, 48, 49}
    assert {(w + 15) // 16 for w in ws} == {1, 2, 3, 4}                      # tiles_x (3: the multiply-shift division is not a shift)
    assert {(h + 15) // 16 for h in hs} == {1, 2, 3}                         # tiles_y on 16-row tiles
    assert {(h + 31) // 32 for h in hs} == {1, 2}                            # ... on 32-row tiles
    assert {h % 4 for h in hs} == {0, 1, 2, 3}                               # wino8's strips of 4 rows
    # a wave owns 4 or 8 rows and works on row pairs: one live row in the only pair, in the last pair of a wave, in the last tile
    assert {1, 3, 5, 7, 9, 17, 33} <= hs
    # border-table rows with opposite edges set need W == 1 or H == 1
    assert 1 in hs and 1 in ws
    # tiles_x == 3 and tiles_y == 3 occur on shapes of their own and together
    assert any((w + 15) // 16 == 3 for _, w in P.SHAPES) and any((h + 15) // 16 == 3 for h, _ in P.SHAPES)
    assert any((w + 15) // 16 == 4 and (h + 15) // 16 == 3 for h, w in P.SHAPES)


def test_every_form_has_every_shape():
    ids = [f["id"] for f in P.FORMS]
    assert len(ids) == len(set(ids))
    rows = list(P.rows())
    assert len(rows) == 16 * sum(len(f["storages"]) for f in P.FORMS)
    for form, compute, hw, n in rows:
        tpi = P.tiles_per_image(hw, form["unit"])
        assert n * tpi >= form["threshold"] and (n - 2) * tpi < form["threshold"]          # the smallest batch that reaches it, plus one image
        assert n >= 4                                                                       # three distinct images and a repeat
    assert max(n for *_, n in rows) == 8193                                                 # 1 x 1 images, 8192 strips


ROWS = [pytest.param(f, c, hw, n, id=f"{f['id']}-{c}-{hw[0]}x{hw[1]}") for f, c, hw, n in P.rows() if f["waves"] is not None]


@pytest.mark.parametrize("form,compute,hw,n", ROWS)
def test_batch_is_above_the_threshold_and_every_chunk_below(form, compute, hw, n):
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    d = P.descriptor(form, compute, n, hw)
    assert lib.esr_conv_block_waves(ctypes.byref(d)) == form["waves"]
    if form["id"] == "hilo-4w":
        assert n * P.tiles_per_image(hw, "t16") < 4096
    for lo, hi in P.chunk_bounds(n, form["chunks"]) if form["chunks"] > 0 else []:
        d = P.descriptor(form, compute, hi - lo, hw)
        assert lib.esr_conv_block_waves(ctypes.byref(d)) != form["waves"], (lo, hi)
    if form["chunks"] > 0:
        bounds = P.chunk_bounds(n, form["chunks"])
        assert len(bounds) == form["chunks"] and bounds[0][0] == 0 and bounds[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    # conv48r_kernel: 4 rows per wave below 1024 tiles of 16 x 32, 8 from there on
    if form["id"].startswith("conv48r-") and form["id"].endswith("rw4"):
        assert n * P.tiles_per_image(hw, "t32") < 1024
