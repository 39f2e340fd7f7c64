"""CPU: the byte patterns of tests/_poison.py are what they claim -- finite in every element type, typed by arena, reproducible from the
seed -- and buffer_ranges names the bytes the engine resolves (the GPU stale-workspace tests rest on them)."""
import pytest
import torch

import _poison as P


@pytest.mark.parametrize("byte,f16,bf16", [(0x3C, 1.05859375, 2.0 ** -7 * (1 + 60 / 128)), (0x77, 30576.0, 2.0 ** 111 * (1 + 119 / 128)),
                                           (0xF7, -32624.0, -2.0 ** 112 * (1 + 119 / 128))])
def test_constant_bytes_are_finite_in_every_type(byte, f16, bf16):
    d = P.constant_bytes(4096 + 2, byte)
    assert d.dtype == torch.uint8 and d.numel() == 4098 and bool((d == byte).all())
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        v = d[:4096].view(dt)
        assert bool(torch.isfinite(v).all()) and float(v.float().abs().min()) > 0.0
    assert float(d[:2].view(torch.float16)) == f16
    assert float(d[:2].view(torch.bfloat16)) == bf16            # sign, 8 exponent bits, 7 mantissa bits of the repeated byte
    # fp32 shares bf16's exponent: the same magnitude to bf16's precision
    assert float(d[:4].view(torch.float32)) == pytest.approx(bf16, rel=1e-2)


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
def test_typed_noise_is_finite_typed_and_reproducible(store):
    nbytes, lo_cap = 256 * 40 + 3, 256 * 9
    d = P.typed_noise(nbytes, lo_cap, store, seed=7)
    assert d.dtype == torch.uint8 and d.numel() == nbytes
    lo, hi = P.typed_views(d, lo_cap, store)
    assert lo.dtype == torch.float32 and lo.numel() == lo_cap // 4 and hi.dtype == P.DTYPES[store]
    assert hi.numel() == (nbytes - lo_cap) // hi.element_size()
    for v in (lo, hi):
        f = v.float()
        assert bool(torch.isfinite(v).all())
        # randn * 100: far from zero on the whole, far below every type's largest value (fp16: 65504)
        assert 80.0 < float(f.std()) < 120.0 and float(f.abs().max()) < 1000.0 and abs(float(f.mean())) < 10.0
    # the typed part is exactly representable in its type (it was rounded to it), the tail is the first constant byte
    assert torch.equal(hi.float().to(P.DTYPES[store]), hi)
    assert bool((d[lo_cap + hi.numel() * hi.element_size():] == P.BYTES[0]).all())
    assert torch.equal(P.typed_noise(nbytes, lo_cap, store, seed=7), d)
    assert not torch.equal(P.typed_noise(nbytes, lo_cap, store, seed=8), d)


def test_typed_noise_without_a_lowres_arena_and_with_one_that_fills_the_workspace():
    d = P.typed_noise(512, 0, "bf16")
    lo, hi = P.typed_views(d, 0, "bf16")
    assert lo.numel() == 0 and hi.numel() == 256 and bool(torch.isfinite(hi).all())
    d = P.typed_noise(512, 1024, "f16")                        # (a workspace of the 256-byte minimum size under a grown lo_cap)
    lo, hi = P.typed_views(d, 1024, "f16")
    assert lo.numel() == 128 and hi.numel() == 0 and bool(torch.isfinite(lo).all())


def test_pattern_dispatch():
    assert P.PATTERNS == ("0x3C", "0x77", "0xF7", "noise")
    for name, byte in zip(P.PATTERNS, P.BYTES):
        assert torch.equal(P.pattern(name, 300, 256, "f16"), P.constant_bytes(300, byte))
    assert torch.equal(P.pattern("noise", 1024, 256, "f16", seed=3), P.typed_noise(1024, 256, "f16", seed=3))


@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_buffer_ranges_tile_the_two_arenas(store):
    """against engine._addr: a Plan's buffers, in the order they were made, fill [0, total_lo) and [lo_cap, lo_cap + total) without gaps"""
    from ntire2022_esr_amd.engine import Plan, _addr
    plan = Plan(2, 24, 31, store)
    plan.buffer("a", 48)
    plan.buffer("lo1", 16, 5, 7)
    plan.buffer("b", 16)
    plan.buffer("lo2", 32, 3, 4)
    lo_cap = plan.total_lo + 512                                # (grown by a larger shape)
    r = P.buffer_ranges(plan, lo_cap)
    assert [n for n, _, _ in r] == ["a", "lo1", "b", "lo2"]
    for (name, start, size), b in zip(r, plan.buffers):
        assert start == _addr(b, (0, lo_cap)) and size % 256 == 0 and size >= plan.n * b.h * b.w * b.pitch * b.esize
    by = {n: (s, z) for n, s, z in r}
    assert by["lo1"][0] == 0 and by["lo2"][0] == by["lo1"][1] and sum(by["lo2"]) == plan.total_lo
    assert by["a"][0] == lo_cap and by["b"][0] == lo_cap + by["a"][1] and sum(by["b"]) == lo_cap + plan.total


def test_poison_range_touches_only_its_bytes():
    ws = torch.zeros(1024, dtype=torch.uint8)
    P.poison_range(ws, P.constant_bytes(1024, 0x77), 256, 512)
    assert bool((ws[:256] == 0).all()) and bool((ws[256:768] == 0x77).all()) and bool((ws[768:] == 0).all())
