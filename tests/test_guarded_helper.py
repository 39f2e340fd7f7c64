"""CPU: the guarded arena of tests/_guarded.py reports what it must and nothing else (the GPU bounds tests rest on it)."""
import pytest
import torch

from _guarded import ALIGN, GUARD_MIN_BYTES, GUARD_ROWS, SENTINEL, Arena, Untouched


def _arena(fill="nan", seed=0):
    a = Arena("cpu", fill=fill, seed=seed)
    g = torch.Generator().manual_seed(3)
    a.add_input("x", torch.randn(2, 5, 7, 24, generator=g).to(torch.bfloat16))
    a.add_input("r", torch.randn(2, 5, 7, 8, generator=g))
    a.add_output("y", (2, 5, 7, 32), torch.bfloat16, writable=(-1, 8, 16))          # coff 8, 16 channels of pitch 32
    a.add_output("z", (2, 5, 7, 8), torch.float32, writable=None)                  # a buffer the launch says it does not store
    a.add_output("img", (2, 3, 20, 28), torch.float32)                             # NCHW, written whole
    return a.build()


def _bytes(t):
    return t.reshape(-1).view(torch.uint8)


def test_views_have_the_requested_shape_alignment_and_neighbours():
    a = _arena()
    for name, shape, dt in (("x", (2, 5, 7, 24), torch.bfloat16), ("r", (2, 5, 7, 8), torch.float32), ("y", (2, 5, 7, 32), torch.bfloat16),
                            ("z", (2, 5, 7, 8), torch.float32), ("img", (2, 3, 20, 28), torch.float32)):
        t = a[name]
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.data_ptr() % ALIGN == 0
    # one flat allocation per dtype: x and y share one, r / z / img the other, and neither pair overlaps
    assert a["x"].untyped_storage().data_ptr() == a["y"].untyped_storage().data_ptr()
    assert a["r"].untyped_storage().data_ptr() == a["z"].untyped_storage().data_ptr() == a["img"].untyped_storage().data_ptr()
    assert a["x"].untyped_storage().data_ptr() != a["r"].untyped_storage().data_ptr()
    # a slice of pitch 32 at coff 8 as the kernels see it
    v = a["y"][..., 8:24]
    assert v.stride() == (5 * 7 * 32, 7 * 32, 32, 1) and v.data_ptr() == a["y"].data_ptr() + 16
    # guards: at least 18 rows and at least 64 KiB on both sides of every tensor
    for s in a.slots:
        assert s.guard >= max(GUARD_ROWS * s.shape[-2] * s.shape[-1] * s.es, GUARD_MIN_BYTES) and s.guard % ALIGN == 0
    by = {s.name: s for s in a.slots}
    assert by["y"].start - (by["x"].start + by["x"].nbytes) >= by["x"].guard + by["y"].guard
    a.check_untouched()


@pytest.mark.parametrize("fill", ["nan", "big", "noise"])
def test_input_guards_hold_the_fill_and_output_bytes_the_sentinel(fill):
    a = _arena(fill)
    _, buf, _, _, _ = a._bufs[torch.bfloat16]
    s = next(s for s in a.slots if s.name == "x")
    before = buf[s.start - s.guard:s.start].view(torch.bfloat16).float()
    behind = buf[s.start + s.nbytes:s.end_guard].view(torch.bfloat16).float()
    for gd in (before, behind):
        if fill == "nan":
            assert bool(torch.isnan(gd).all())
        elif fill == "big":
            assert bool((gd == 29952.0).all())                   # 3e4 in bf16: finite
        else:
            assert bool(torch.isfinite(gd).all()) and float(gd.std()) > 1.0
    assert float(torch.tensor(3.0e4).to(torch.float16)) == 30000.0                   # and exact in f16
    s = next(s for s in a.slots if s.name == "y")
    assert bool((buf[s.start - s.guard:s.end_guard] == SENTINEL).all())
    assert bool(torch.isfinite(a["y"].float()).all()) and bool(torch.isfinite(a["z"]).all())
    # two seeds of the noise fill differ, the same seed repeats
    if fill == "noise":
        b, c = _arena(fill, seed=1), _arena(fill, seed=0)
        assert not torch.equal(b._bufs[torch.bfloat16][2], a._bufs[torch.bfloat16][2])
        assert torch.equal(c._bufs[torch.bfloat16][2], a._bufs[torch.bfloat16][2])


def test_a_write_inside_the_view_is_not_reported():
    a = _arena()
    a["y"][..., 8:24] = 1.5
    a["img"][...] = float("nan")
    a.check_untouched()
    assert torch.equal(a.written("y"), torch.full((2, 5, 7, 16), 1.5, dtype=torch.bfloat16))
    with pytest.raises(KeyError):
        a.written("z")


@pytest.mark.parametrize("name,byte,where,region", [
    ("y", 2 * 5 * 7 * 32 * 2, ("y", 2, 0, 0, 0), "guard behind"),                      # the first byte behind the last image
    ("y", 2 * 5 * 7 * 32 * 2 + 2 * (3 * 32 + 9) + 1, ("y", 2, 0, 3, 9), "guard behind"),
    ("y", -1, ("y", -1, 4, 6, 31), "guard before"),                                  # the last byte in front of the tensor
    ("x", 2 * 5 * 7 * 24 * 2 + 2 * (7 * 24 + 5), ("x", 2, 1, 0, 5), "guard behind"),   # an INPUT's guard is watched too
    ("img", -4 * 28, ("img", -1, 2, 19, 0), "guard before")])      # NCHW: the last three dims are (plane, row, column)
def test_one_changed_guard_byte_is_reported_with_its_coordinates(name, byte, where, region):
    a = _arena()
    s = next(s for s in a.slots if s.name == name)
    _, buf, _, _, _ = a._bufs[s.dtype]
    buf[s.start + byte] ^= 1
    with pytest.raises(Untouched) as e:
        a.check_untouched()
    assert e.value.where == where and e.value.region == region
    assert f"image {where[1]}, row {where[2]}, column {where[3]}, channel {where[4]}" in str(e.value)


@pytest.mark.parametrize("name,index,region", [
    ("y", (1, 3, 2, 24), "outside the declared view"),          # the first channel behind [8, 24)
    ("y", (0, 0, 0, 7), "outside the declared view"),           # the last channel in front of it
    ("z", (1, 4, 6, 7), "outside the declared view"),           # a buffer declared as not stored
    ("x", (1, 2, 3, 4), "input")])                              # an input is not written either
def test_a_change_outside_the_declared_view_is_reported_with_its_coordinates(name, index, region):
    a = _arena()
    t = a[name]
    _bytes(t[index])[0] ^= 0x80
    with pytest.raises(Untouched) as e:
        a.check_untouched()
    assert e.value.where == (name,) + index and e.value.region == region


def test_the_first_offence_is_the_one_reported_and_nan_bits_compare_as_bits():
    a = _arena()
    a["z"][0, 1, 2, 3] = 0.0
    a["z"][1, 0, 0, 0] = 0.0
    with pytest.raises(Untouched) as e:
        a.check_untouched()
    assert e.value.where == ("z", 0, 1, 2, 3)
    # a NaN guard that is rewritten with another NaN payload changed; an untouched NaN guard did not
    a = _arena("nan")
    a.check_untouched()
    s = next(s for s in a.slots if s.name == "r")
    _, buf, _, _, _ = a._bufs[torch.float32]
    buf[s.start + s.nbytes:s.start + s.nbytes + 4].view(torch.int32)[0] = 0x7fc00001
    with pytest.raises(Untouched) as e:
        a.check_untouched()
    assert e.value.where == ("r", 2, 0, 0, 0)


def test_declarations_are_checked():
    a = Arena("cpu")
    a.add_output("y", (1, 4, 4, 16), torch.float16, writable=(-1, 8, 8))
    with pytest.raises(ValueError):
        a.add_output("y", (1, 4, 4, 16), torch.float16)
    with pytest.raises(ValueError):
        a.add_output("w", (1, 4, 4, 16), torch.float16, writable=(-1, 12, 8))
    with pytest.raises(ValueError):
        Arena("cpu", fill="zero")
    a.build()
    with pytest.raises(RuntimeError):
        a.add_output("late", (1,), torch.float32)


def test_a_blocked_tensor_gets_its_guard_from_the_row_it_is_given():
    """[N, C/8, H, W, 8]: the last two dims are (w, 8), one image row is w * C elements -- the guard must hold 18 of THOSE"""
    a = Arena("cpu")
    w, planes = 700, 7
    a.add_output("blk", (1, planes, 3, w, 8), torch.float32, writable=(1, 1, 5), row=w * planes * 8)
    a.add_output("plain", (1, planes, 3, w, 8), torch.float32)
    a.build()
    by = {s.name: s for s in a.slots}
    assert by["blk"].guard >= GUARD_ROWS * w * planes * 8 * 4 > GUARD_MIN_BYTES
    assert by["plain"].guard < by["blk"].guard
    a.check_untouched()
