"""tests/_esa_apply_ref.py checked without a GPU, in both directions: the fp32 emulation of esa_apply_mfma_kernel's documented arithmetic is
inside bound (a) and cap (b) -- and, summed another way, inside cap (c) -- on every case of the GPU matrix (tests/test_gpu_esa_apply.py;
the large case excepted), and each way that arithmetic can be subtly wrong misses (a) or (b), and (c), on a named case -- so the GPU
test can fail for each of them."""
import pytest
import torch
import torch.nn.functional as F

import _esa_apply_ref as R

CASES = R.combos()
IDS = [R.case_id(g, wd) for g, wd in CASES]


def test_matrix_is_the_documented_one():
    """every width on three geometries, every geometry on two widths: 3 * 7 + 8 * 2 cases, not the full product"""
    assert len(CASES) == 37 and len(set(IDS)) == 37
    assert all(w >= 8 for (_, _, w, _), _ in CASES) and R.BIG[2] >= 8
    # NP = 1 and NP = 2 of esa_apply_mfma_kernel are both there, with the smallest NP = 2
    assert {(c + 3) // 4 * 4 > 32 for _, (c, _) in CASES} == {False, True} and (33, 16) in R.WIDTHS
    # the large case needs several passes of the 4096-block grid: more than 4096 * 4 waves * 2 groups
    n, h, w, _ = R.BIG
    assert (n * h * w + 15) // 16 == 67500 > 4096 * 4 * 2


@pytest.mark.parametrize("W,wrong,total", [(7, 2, 266), (6, 10, 228), (5, 31, 190), (4, 36, 152)] + [(w, 0, 38 * w) for w in range(8, 17)])
def test_two_wrap_carry_needs_w8(W, wrong, total):
    """the apply kernels' (n, oy, ox) -- one division per 16-pixel group, a carry over at most two rows -- replayed for H = 19, N = 2: right
    for W >= 8 and wrong below, which is why esr_esa_apply_f32 refuses W < 8"""
    n, oy, ox = R.carry_coords(2, 19, W)
    en, ey, ex = R.exact_coords(2, 19, W)
    assert n.numel() == total
    assert int(((n != en) | (oy != ey) | (ox != ex)).sum()) == wrong


@pytest.mark.parametrize("geom", R.GEOMS, ids=[R.case_id(g, (0, 0))[:-5] for g in R.GEOMS])
def test_carry_is_exact_on_every_geometry(geom):
    N, H, W, _ = geom
    for got, want in zip(R.carry_coords(N, H, W), R.exact_coords(N, H, W)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("geom", R.GEOMS, ids=[R.case_id(g, (0, 0))[:-5] for g in R.GEOMS])
def test_ref64_is_atens_operation(geom):
    """ref64's own bilinear rule and layout against F.interpolate(align_corners=False) and F.conv2d in fp64"""
    inp = R.make_inputs(geom, (50, 12), "bf16")
    r = R.ref64(**inp, storage="bf16")
    d = {k: v.double() for k, v in inp.items()}
    up = F.interpolate(d["c3"].permute(0, 3, 1, 2), geom[1:3], mode="bilinear", align_corners=False)
    s = up + F.conv2d(d["c1"].permute(0, 3, 1, 2), d["wf"][:, :, None, None], d["bf"])
    want = d["x"].permute(0, 3, 1, 2) * torch.sigmoid(F.conv2d(s, d["w4"][:, :, None, None], d["b4"]))
    assert float((r.ref.permute(0, 3, 1, 2) - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    # the bound has its parts: half a step at least, the arithmetic part positive and below half a step on almost every element
    assert bool((r.bound >= 0.5 * r.step * 0.99).all()) and bool((r.arith > 0).all())


@pytest.mark.parametrize("storage", ["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_is_inside(storage, case):
    """emulate32 meets (a) and (b); the same arithmetic with another summation (fp64 sums, rounded once) meets them too and stays within
    (c) of it -- what a correct kernel whose matrix instructions add in another order would give"""
    inp = R.make_inputs(*case, storage)
    r = R.ref64(**inp, storage=storage)
    emu = R.emulate32(**inp, storage=storage)
    R.compare(emu, r, f"emulate32 {storage} {R.case_id(*case)}")
    R.compare(R.emulate32(**inp, storage=storage, exact_sums=True), r, f"emulate32 with exact sums {storage} {R.case_id(*case)}", emu=emu)


def test_fp32_evaluation_is_inside_the_fp32_bound():
    """fp32 storage: ATen's fp32 evaluation stays inside 2e-5 * max(1, max|ref|) + the coordinate term, on the geometry with the largest source"""
    geom, wd = R.GEOMS[10], (50, 12)
    inp = R.make_inputs(geom, wd, "f32")
    r = R.ref64(**inp, storage="f32")
    up = F.interpolate(inp["c3"].permute(0, 3, 1, 2), geom[1:3], mode="bilinear", align_corners=False)
    s = up + F.conv2d(inp["c1"].permute(0, 3, 1, 2), inp["wf"][:, :, None, None], inp["bf"])
    y = inp["x"].permute(0, 3, 1, 2) * torch.sigmoid(F.conv2d(s, inp["w4"][:, :, None, None], inp["b4"]))
    fig = R.compare(y.permute(0, 2, 3, 1), r, "ATen fp32")
    assert "mism" not in fig                       # (b) is about 16-bit stores


# the case that catches each mutant (in both storage types).  one_wrap: at W = 8 a group starts at column 0 of a row (16 = 2 W), so ONE wrap
# is all it ever needs and dropping the second changes nothing there; W = 9 is the smallest width whose groups wrap twice.
CAUGHT_ON = {
    "wf_rounded": (R.GEOMS[0], (50, 12)),
    "w4_rounded": (R.GEOMS[0], (32, 16)),
    "s_rounded": (R.GEOMS[0], (50, 12)),
    "align_corners": (R.GEOMS[4], (50, 12)),
    "no_half_pixel": (R.GEOMS[4], (50, 12)),
    "no_clamp0": (R.GEOMS[9], (50, 12)),
    "no_clamp_edge": (R.GEOMS[9], (32, 16)),
    "swap_lx_ly": (R.GEOMS[4], (32, 16)),
    "quarter_lx_zero": (R.GEOMS[4], (50, 12)),
    "tiles_swapped": (R.GEOMS[0], (33, 16)),
    "one_wrap": (R.GEOMS[3], (50, 12)),
}


def test_every_mutant_is_listed():
    assert set(CAUGHT_ON) == set(R.MUTANTS) and all(c in CASES for c in CAUGHT_ON.values())


@pytest.mark.parametrize("storage", ["bf16", "f16"])
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_caught(storage, mutant):
    case = CAUGHT_ON[mutant]
    inp = R.make_inputs(*case, storage)
    r = R.ref64(**inp, storage=storage)
    got = R.emulate32(**inp, storage=storage, mutant=mutant)
    fig = R.measure(got, r)
    print(R.describe(f"{mutant} {storage} {R.case_id(*case)}", fig), "-> misses", sorted(R.failures(fig)))
    assert R.failures(fig) & {"a", "b"}, R.describe(mutant, fig)
    with pytest.raises(AssertionError):
        R.compare(got, r, mutant)
    # and (c), the comparison with the emulation, sees it on its own
    assert "c" in R.failures(R.measure(got, r, R.emulate32(**inp, storage=storage)))


def test_one_wrap_is_no_mutant_at_w8():
    """(see CAUGHT_ON) the carry with one wrap equals the exact coordinates at W = 8 and differs at W = 9"""
    for got, want in zip(R.carry_coords(2, 19, 8, wraps=1), R.exact_coords(2, 19, 8)):
        assert torch.equal(got, want)
    assert not torch.equal(R.carry_coords(2, 12, 9, wraps=1)[2], R.exact_coords(2, 12, 9)[2])
