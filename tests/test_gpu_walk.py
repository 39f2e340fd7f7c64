"""-m gpu: the one-launch kernels' VALUES where a block walks many tiles ("The walk table").

The persistent fused kernels start at most 256 blocks (pa_gate_kernel / mdsa_gate_kernel: 2048 / 768 blocks of four waves over groups of 16
pixels) and loop over the rest of their work.  What only matters from a block's second item on -- the barriers at the end of a tile, the
weight images a block copies into LDS once, conv_prelu_kernel's three-stage ring (a stage is reused on the fourth tile), s16_tile_index's
un-swizzled last round, rlfb_chain_kernel's hand-over from job to job -- ran in no value test: the kernels' own suites stop at two dozen
tiles.  tests/_walk_cases.py holds the forms and the table (four rounds and a partial fifth on batches of thin images; two for the group
walkers); each case asserts

  1. the kernel that ran: exactly one launch, the form's kernel with its template arguments;
  2. images 0 .. 2 and the last three against the fp64 restatement and the bound of the kernel's OWN suite (the same function objects), and bit
     for bit against the launches that suite holds it equal to (the chain, the HFAB, the cascade);
  3. walk == no walk: the same batch as consecutive chunks of at most one round through the same wrapper -- the same kernel (these kernels
     have no tile threshold), every stored channel, the pad granule and the sentinel behind it bit-identical.  This one needs no number;
  4. no dependence on the position in the batch: the batch is base[i % 3], so output i is output i % 3, bit for bit;
  5. pad channels zero up to the 16-byte granule, the sentinel behind it untouched."""
import importlib

import pytest
import torch

import _walk_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("form,compute,hw,n", [pytest.param(f, c, hw, n, id=f"{f['id']}-{c}-{hw[0]}x{hw[1]}") for f, c, hw, n in W.rows()])
def test_walk(form, compute, hw, n):
    period = form["period"]
    case = form["run"](compute, hw, n)
    case.outs, case.names = case.launch(0, n)
    torch.cuda.synchronize()
    # 1. the kernel that ran
    want = W.symbol(form, compute)
    assert len(case.names) == 1 and case.names[0].startswith(want), (case.names, want)
    assert all(y.shape[0] == n for y in case.outs)
    # 2. values: images 0 .. 2 and the last three (brought into base order), against the own suite's restatement and bound
    worst = 0.0
    last = sorted(range(n - period, n), key=lambda i: i % period)
    for idx in (list(range(period)), last):
        outs = [y[idx].cpu() for y in case.outs]
        for name, got, ref, tol in case.values(outs):
            assert got.shape == ref.shape and got.shape[0] == period, name
            ratio = float(((got - ref).abs() / tol).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, idx, ratio)
        for name, got, ref in case.exact(outs):
            assert got.shape == ref.shape and torch.equal(got, ref), (name, idx, int((got != ref).sum()))
    print(f"walk {form['id']} {compute} {n} x {hw}: worst |got - ref| / tol = {worst:.3f}" + (f" {case.extra}" if case.extra else ""))
    # 3. walk == no walk: chunks of at most one round, the same kernel, bit-identical
    for lo, hi in W.chunks(form, hw, n):
        outs1, names1 = case.launch(lo, hi)
        assert names1 == case.names, (names1, lo, hi)
        for k, (y, y1) in enumerate(zip(case.outs, outs1)):
            assert torch.equal(y[lo:hi], y1), (k, lo, hi, int((y[lo:hi] != y1).sum()))
    # 4. output i is output i % period
    idx = (torch.arange(n) % period).to(DEV)
    for k, y in enumerate(case.outs):
        assert torch.equal(y, y[:period][idx]), (k, int((y != y[:period][idx]).sum()))
    # 5. pad channels of the granule; nothing behind what is stored
    for y, (c, stored) in zip(case.outs, case.pads):
        assert stored < y.shape[-1] and torch.all(y[..., c:stored] == 0) and torch.all(y[..., stored:] == W.SENTINEL)


# ---- one network-level test per newer network with a fused form: 3 distinct images repeated to 520 (1040 tiles: four rounds and a fifth)
# (module of the network's own suite, its loader there, the loader's arguments with every fused switch on, data range, fused kernels)
NETWORKS = [("bmdn", "test_gpu_bmdn", "_bmdn", ("bf16", True), 1.0, ("distill_step_kernel",)),
            ("esan", "test_gpu_esan", "_esan", ("bf16", True), 255.0, ("resblock_head_kernel",)),
            ("frfdn", "test_gpu_frfdn", "_frfdn", ("bf16", True), 1.0, ("refine_cascade_kernel",)),
            ("rfdnext", "test_gpu_rfdnext", "_rfdnext", ("bf16", True), 1.0, ("cx_block_kernel",)),
            ("dwrfdn", "test_gpu_dwrfdn", "_dwrfdn", ("bf16", True), 255.0, ("dwpw_pair_kernel",)),
            ("repafdn", "test_gpu_repafdn", "_repafdn", ("bf16", True), 1.0, ("pa_tail_kernel",)),
            ("arfdn", "test_gpu_arfdn", "_arfdn", ("bf16", True), 1.0, ("asym_step_kernel",)),
            ("resdn", "test_gpu_resdn", "_resdn", ("bf16", False, True), 1.0, ("resdb_step_kernel",)),
            ("mdgn", "test_gpu_mdgn", "_mdgn", ("bf16", True, True), 255.0, ("conv_prelu_kernel", "mdsa_gate_kernel")),
            ("fmen", "test_gpu_fmen", "_fmen", ("bf16",), 255.0, ("hfab_kernel",))]


@pytest.mark.parametrize("name,module,loader,args,dr,kernels", NETWORKS, ids=[v[0] for v in NETWORKS])
def test_network_on_520_thin_images(name, module, loader, args, dr, kernels):
    m = getattr(importlib.import_module(module), loader)(*args)
    hw, n, period = (17, 15), 520, W.PERIOD
    base = torch.rand(period, 3, *hw, generator=torch.Generator().manual_seed(len(name) + hw[0])) * dr
    idx = torch.arange(n) % period
    x = base[idx].contiguous().to(DEV)
    with torch.no_grad():
        for graphs in (False, True):
            m.use_graphs = graphs
            for _ in range(2):                      # (graphs on: the second forward of a shape replays the captured graph)
                y = m(x).clone()
                assert tuple(y.shape) == (n, 3, 4 * hw[0], 4 * hw[1])
                assert torch.equal(y, y[:period][idx.to(DEV)]), (name, graphs)
        m.enable_profiling(1)
        m(x)
        torch.cuda.synchronize()
        names = sorted({o["kernel"] for o in m.collect_profile()})
        m.disable_profiling()
    fused = [k for k in names if k.startswith(kernels)]
    print(f"{name} bf16 {n} x {hw}: fused kernels of the forward: {fused}")
    assert {k.split("<")[0] for k in fused} == set(kernels), names
