"""The walk table: the one-launch kernels on batches in which every block walks four work items and a few walk five.

The fused kernels written since BMDN are persistent: their launchers start min(work items, GRID) blocks and every block strides over the
tiles (rlfb_chain_kernel: over its jobs, in s16_tile_index's order); pa_gate_kernel and mdsa_gate_kernel stride over groups of 16 pixels,
four waves per block, under a cap of their own.  The kernels' own suites stop at a few dozen tiles, one per block.  Each function below is one
form: it takes the inputs of PERIOD images from the kernel's own suite (the same `_case` / `random_case` / `conv_case` it tests with), repeats
them to the batch base[i % PERIOD] and returns a Walk -- how to launch images [lo, hi) of that batch through the kernel's ops wrapper, and
the fp64 restatement and bound of that suite for the outputs of PERIOD images.  The callers hold the assertions; nothing here compares.

FORMS is the table; rows() gives every (form, storage, shape) with its batch size and the chunks of the walk == no walk check.  The module
imports without a GPU (tests/test_walk_table.py)."""
import os

import torch
import torch.nn.functional as F

from _persist_cases import Case, _rep, batch_for, chunk_bounds, tiles_per_image

DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
TF = {True: "true", False: "false"}
PERIOD, CHAIN_PERIOD = 3, 7
SENTINEL = 7.0

GRID = 256                      # ESR_BLOCKS_1_PER_CU (csrc/esr_internal.h): the blocks esr_persistent_grid starts at most
PA_ROUND = 2048 * 4             # PA_GRID_CAP blocks of PA_NW = 4 waves (csrc/esr_pa.hip): groups of 16 pixels per round
MG_ROUND = 768 * 4              # MG_GRID_CAP blocks of MG_NW = 4 waves (csrc/esr_mdsa.hip)
CH_HALO, CH_LAGP = 3, 8         # csrc/esr_chain.hip: what chain_geometry_g prices a job with

# three of the thin-batch suite's shapes (test_network_on_300_thin_images' two and the largest of _persist_cases.SHAPES): one to four tiles
# across, one to three down, a single live row or column in the last tile, a change of image at least every 12 tiles.  No predicate of these
# kernels refuses one of them (the chain needs h >= 4, the networks' ESA branches 15 x 15)
SHAPES = [(17, 15), (16, 33), (33, 49)]
KERNELS = ["rlfb_chain_kernel", "hfab_kernel", "distill_step_kernel", "resblock_head_kernel", "refine_cascade_kernel", "cx_block_kernel",
           "dwpw_pair_kernel", "pa_tail_kernel", "asym_step_kernel", "resdb_step_kernel", "conv_prelu_kernel", "pa_gate_kernel", "mdsa_gate_kernel"]


def r8(c):
    return (c + 7) // 8 * 8


class Walk(Case):
    """one form at one (storage, shape, batch): a Case whose names and outs the caller fills from launch(0, n).  launch(lo, hi) -> (outs, names):
    images [lo, hi) of the batch through the ops wrapper (Case.chunk), every output in a SENTINEL-filled tensor wider than what the launch
    stores; pads: per output (logical channels, stored channels); values(outs) -> [(name, got, ref, tol)] and exact(outs) ->
    [(name, got, want)]: the own suite's fp64 restatement with its bound, and what that suite holds the kernel to bit for bit, for the
    outputs (on the CPU) of the form's `period` images in base order"""

    def __init__(self, launch, pads, values=None, exact=None, **extra):
        super().__init__(None, None, None, launch, pads=pads, **extra)
        self.launch, self.values, self.exact = launch, values or (lambda outs: []), exact or (lambda outs: [])


def _sent(like, m, hw, pitch):
    return torch.full((m, hw[0], hw[1], pitch), SENTINEL, dtype=like.dtype, device=DEV)


def _padded(t, pitch):
    return F.pad(t, (0, pitch - t.shape[-1])).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


# ---- the forms --------------------------------------------------------------------------------------------------------------------------------
def rlfb_chain(compute, hw, n, g, period):
    """ops.conv_chain at RLFN's widths with the strip width forced (ESR_CHAIN_G, as tests/test_gpu_chain.py's strip_groups); the batch is
    base[i % period] of `period` images (CHAIN_PERIOD below)"""
    import test_gpu_chain as T
    from ntire2022_esr_amd import ops
    nf, mf, f = T.RLFN_WIDTHS
    wts = T._weights(1000 * period + hw[0] + hw[1], nf, mf, f)
    x = torch.zeros(period, hw[0], hw[1], 48)
    x[..., :nf] = torch.randn(period, hw[0], hw[1], nf, generator=torch.Generator().manual_seed(hw[0] * hw[1]))
    xb = x.to(DT[compute]).to(DEV)
    xin = _rep(xb, n, period)

    def forced(fn):
        old = os.environ.get("ESR_CHAIN_G")
        os.environ["ESR_CHAIN_G"] = str(g)
        try:
            return fn()
        finally:
            if old is None:
                del os.environ["ESR_CHAIN_G"]
            else:
                os.environ["ESR_CHAIN_G"] = old

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, 64), _sent(xin, hi - lo, hw, 24)]
        with ops.kernel_trace() as names:
            forced(lambda: ops.conv_chain(xin[lo:hi], *wts, cin=nf, v_out=outs[0], c1_out=outs[1]))
        return outs, names

    def exact(outs):
        rv, rc1 = T._separate(xb, *wts, nf)
        return [("v", outs[0][..., :nf], rv.cpu()[..., :nf]), ("c1", outs[1][..., :r8(f)], rc1.cpu())]

    return Walk(launch, [(nf, 48), (f, r8(f))], exact=exact)


def hfab(compute, hw, n, cin, cmid):
    """FMEN's HFAB (ops.conv_chain with ESR_RES_GATE -> ops._hfab) against the four per-layer launches, as tests/test_gpu_fmen.py"""
    import test_gpu_fmen as T
    from ntire2022_esr_amd import _lib as L, ops
    pitch, slope = r8(cin), 0.05
    ws, bs = T._hfab_weights(PERIOD * 100 + hw[0] + cin, cin, cmid)
    g = torch.Generator().manual_seed(hw[0] * hw[1] + cin)
    xb = _padded(torch.randn(PERIOD, hw[0], hw[1], cin, generator=g) * 2, pitch).to(DT[compute]).to(DEV)
    xin = _rep(xb, n, PERIOD)
    stored = (cin + 15) // 16 * 16                # the last chunk's pad channels are stored too, as zeros (ops._hfab)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, stored + 8)]
        with ops.kernel_trace() as names:
            ops.conv_chain(xin[lo:hi], ws, bs, slope=slope, res_mode=L.RES_GATE, cin=cin, out=outs[0])
        return outs, names

    def exact(outs):
        return [("y", outs[0][..., :pitch], T._hfab_per_layer(xb, ws, bs, slope, cin, pitch).cpu())]

    return Walk(launch, [(cin, stored)], exact=exact)


def distill(compute, hw, n, cin, cmid, cout, res):
    import test_gpu_bmdn as T
    from ntire2022_esr_amd import ops
    c, dt = T._case(compute, cin, hw, n=PERIOD, cmid=cmid, cout=cout), DT[compute]
    xin = _rep(_padded(c["x"], r8(cin)).to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, r8(cmid) + 8), _sent(xin, hi - lo, hw, r8(cout) + 8)]
        with ops.kernel_trace() as names:
            ops.distill_step(xin[lo:hi], *c["w"], res=res, cin=cin, d_out=outs[0], out=outs[1])
        return outs, names

    def values(outs):
        ds = outs[0][..., :cmid].permute(0, 3, 1, 2)
        ref_d, ref_y = T._ref_d(c), T._ref_out(c, ds, res)                       # out from the d THE KERNEL STORED
        return [("d", ds.double(), ref_d, T._tol(ref_d, dt)), ("out", _nchw(outs[1][..., :cout]), ref_y, T._tol(ref_y, dt))]

    return Walk(launch, [(cmid, r8(cmid)), (cout, r8(cout))], values)


def resblock_head(compute, hw, n, with_g):
    import test_gpu_esan as T
    from ntire2022_esr_amd import ops
    c = T._case(compute, (PERIOD,) + hw)
    xin, gin = _rep(c["x"].to(DEV), n, PERIOD), _rep(c["g"].to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = ([_sent(xin, hi - lo, hw, 40)] if with_g else []) + [_sent(xin, hi - lo, hw, 40), _sent(xin, hi - lo, hw, 24)]
        kw = dict(g=gin[lo:hi], x_out=outs[0]) if with_g else {}
        with ops.kernel_trace() as names:
            ops.resblock_head(xin[lo:hi], *c["w"], u_out=outs[-2], c1_out=outs[-1], **kw)
        return outs, names

    def values(outs):
        res = []
        if with_g:
            ref_x = T._nchw(c["x"]) + T._nchw(c["g"])
            res.append(("x", T._nchw(outs[0][..., :T.C]), ref_x, T._tol(ref_x, compute)))
        u, c1 = outs[-2][..., :T.C], outs[-1]
        t, ref_u = T._ref_u(c, T._nchw(outs[0][..., :T.C] if with_g else c["x"]), compute)
        res.append(("u", T._nchw(u), ref_u, T._tol_u(c, t, ref_u, compute)))
        wc, bc = c["ec"]
        ref_c = F.conv2d(T._nchw(u), wc.double(), bc.double())
        res.append(("c1", T._nchw(c1[..., :T.FE]), ref_c, T._tol(ref_c, compute)))
        return res

    return Walk(launch, ([(32, 32)] if with_g else []) + [(32, 32), (8, 8)], values)


def refine_cascade(compute, hw, n):
    import test_gpu_frfdn as T
    from ntire2022_esr_amd import ops
    c, dt = T._case(compute, hw, n=PERIOD), DT[compute]
    xin = _rep(c["x"].to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, 24), _sent(xin, hi - lo, hw, 24)]
        with ops.kernel_trace() as names:
            ops.refine_cascade(xin[lo:hi], *c["w"], slope=T.SLOPE, d3_out=outs[0], r4_out=outs[1])
        return outs, names

    def values(outs):
        refs = T._stage_refs(c)                                                  # each stage on what the previous launch stored
        return [("d3", T._nchw(outs[0][..., :16]), refs[1], T._tol(refs[1], dt)), ("r4", T._nchw(outs[1][..., :16]), refs[3], T._tol(refs[3], dt))]

    def exact(outs):
        return [("d3", outs[0][..., :16], c["per_op"][1]), ("r4", outs[1][..., :16], c["per_op"][3])]

    return Walk(launch, [(16, 16), (16, 16)], values, exact)


def _cx_fp32_orders(T, cs, dt, ts, orders=8):
    """The ConvNeXt block from t as stored (NCHW fp64), the hidden tensor summed in FP32 on the CPU in `orders` channel orders, rounded where
    the kernel stores, the result rounded once: how far fp32 evaluations of the chain land from the fp64 restatement, in units of ITS bound"""
    _, _, _, b1, _, b2 = cs["w"]
    ref = T._cx_ref(cs, dt, t_stored=ts)
    g = torch.Generator().manual_seed(ts.shape[2] * 64 + ts.shape[3])
    worst = 0.0
    for k in range(orders):
        perm = torch.arange(ts.shape[1]) if k == 0 else torch.randperm(ts.shape[1], generator=g)
        pre = torch.zeros(ts.shape[0], cs["w1e"].shape[0], *ts.shape[2:])
        for j in perm.tolist():                                                  # one input channel at a time: the order is the sum's order
            pre = pre + ts[:, j:j + 1].float() * cs["w1e"][:, j].float().view(1, -1, 1, 1)
        h = F.leaky_relu(pre + b1.float().view(1, -1, 1, 1), T.SLOPE).to(dt).double()
        out = (F.conv2d(h, cs["w2e"], b2.double()) + T._nchw(cs["x"])).to(dt).double()
        worst = max(worst, float(((out - ref).abs() / T._tol(ref, dt)).max()))
    return worst


def cx_block(compute, hw, n, c, m):
    """The own suite's restatement rounds the hidden tensor, which no launch stores, from an fp64 sum; the kernel rounds an fp32 sum.  Where a
    hidden value lies closer to a rounding boundary than fp32 resolves, the two may round it to neighbouring storage values, and one 16-bit
    step of it times a weight of the second 1x1 can exceed the one-store bound, which has no term for it (test_gpu_rfdnext._case says so for
    large t).  Seed 0 at bf16 (16, 33) has one: h = 1.464843651 of hidden channel 182, 1.3e-5 of a step from the boundary between 1.4609375
    and 1.46875; that step times w2 is 6.3e-4 and 3.8e-4 at two outputs of the pixel whose bounds are 2.6e-4 (measured 2.23 of the bound, the
    same bits with and without a walk).  So the data are screened ON THE CPU, before any result is looked at: the first seed at which eight fp32
    evaluations of the chain in different summation orders all stay inside that bound of the fp64 restatement."""
    import test_gpu_rfdnext as T
    from ntire2022_esr_amd import ops
    dt = DT[compute]
    for seed in range(16):
        cs = T._case(compute, (PERIOD,) + hw, c=c, m=m, seed=seed)
        xb = _padded(cs["x"], r8(c)).to(DEV)
        ts = T._nchw(ops.dwconv7x7(xb, *cs["w"][:2]).cpu()[..., :c])              # t as esr_dwconv7x7 stores it: the suite's asserted reference
        if _cx_fp32_orders(T, cs, dt, ts) <= 1.0:
            break
    else:
        raise AssertionError("no seed at which the restatement bounds an fp32 evaluation of the chain")
    xin = _rep(xb, n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, r8(c) + 8)]
        with ops.kernel_trace() as names:
            ops.cx_block(xin[lo:hi], *cs["w"], slope=T.SLOPE, out=outs[0])
        return outs, names

    def values(outs):
        ref = T._cx_ref(cs, dt, t_stored=ts)
        return [("out", T._nchw(outs[0][..., :c]), ref, T._tol(ref, dt))]

    return Walk(launch, [(c, r8(c))], values, seed=seed)


def dwpw_pair(compute, hw, n, c):
    import test_gpu_dwrfdn as T
    from ntire2022_esr_amd import ops
    cs, dt = T._case(compute, (PERIOD,) + hw, c=c), DT[compute]
    xin = _rep(_padded(cs["x"], r8(c)).to(DEV), n, PERIOD)
    seen = {}

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, r8(c) + 8)]
        with ops.kernel_trace() as names:
            ops.dwpw_pair(xin[lo:hi], *cs["w"], slope=T.SLOPE, out=outs[0])
        return outs, names

    def values(outs):
        if not seen:                                                             # the hidden tensors as the kernel holds them (T._observe), once
            seen.update({k: T._observe(cs, k) for k in ("u1", "h", "u2")})
        got = dict(seen, out=T._nchw(outs[0][..., :c]))
        return [(name, got[name], ref, T._tol(ref, dt)) for name, ref in T._stage_refs(cs, T._nchw(cs["x"]), got["u1"], got["h"], got["u2"], cs["wae"], cs["wbe"])]

    return Walk(launch, [(c, r8(c))], values)


def pa_tail(compute, hw, n, c):
    import test_gpu_repafdn as T
    from ntire2022_esr_amd import ops
    cs, dt = T._tail_case(compute, (PERIOD,) + hw, c), DT[compute]
    s, s64 = T._s_of(cs, "single")
    xin, sin = _rep(_padded(cs["x"], r8(c)).to(DEV), n, PERIOD), _rep(_padded(s, r8(c)).to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, r8(c) + 8)]
        with ops.kernel_trace() as names:
            ops.pa_tail(xin[lo:hi], cs["w3"], cs["b3"], cs["w"], cs["b"], s=sin[lo:hi], out=outs[0])
        return outs, names

    def values(outs):
        hi_, lo_ = T._hidden_t(cs)                                               # t, which no launch stores, handed out exactly
        t = hi_.double() + lo_.double()
        ref = t * T._sigmoid(hi_.double() @ cs["we"].t() + cs["be"]) + s64
        return [("y", outs[0][..., :c].double(), ref, T._tol(ref, dt))]

    return Walk(launch, [(c, r8(c))], values)


def pa_gate(compute, hw, n, c):
    import test_gpu_repafdn as T
    from ntire2022_esr_amd import ops
    cs, dt = T._case(compute, (PERIOD,) + hw, c), DT[compute]
    s, s64 = T._s_of(cs, "single")
    tin, sin = _rep(_padded(cs["t"], r8(c)).to(DEV), n, PERIOD), _rep(_padded(s, r8(c)).to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(tin, hi - lo, hw, r8(c) + 8)]
        with ops.kernel_trace() as names:
            ops.pa_gate(tin[lo:hi], cs["w"], cs["b"], s=sin[lo:hi], out=outs[0])
        return outs, names

    def values(outs):
        ref, _ = T._ref(cs, s64)
        return [("y", outs[0][..., :c].double(), ref, T._tol(ref, dt))]

    return Walk(launch, [(c, r8(c))], values)


def asym_step(compute, hw, n, cin, c, res, np_):
    import _arfdn as A
    import test_gpu_arfdn as T
    from ntire2022_esr_amd import _lib as L, ops
    case = T._case("random", compute, hw, cin, c, res, np_, n=PERIOD)
    W, dt = case.W, case.dt
    xin = _rep(_padded(case.x, r8(cin)).to(DEV), n, PERIOD)
    pin = [_rep(_padded(p, r8(c)).to(DEV), n, PERIOD) for p in case.ps]

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, r8(c) + 8), _sent(xin, hi - lo, hw, r8(c) + 8)]
        pk = dict(zip(("p1", "p2"), [p[lo:hi] for p in pin]))
        with ops.kernel_trace() as names:
            ops.asym_step(xin[lo:hi], W["w_d"], W["b_d"], W["w_l1"], W["b_l1"], W["w_l2"], W["b_l2"], W["w_m1"], W["b_m1"], W["w_m2"], W["b_m2"],
                          res=res, act=L.ACT_LRELU, slope=case.slope, cin=cin, d_out=outs[0], out=outs[1], **pk)
        return outs, names

    def values(outs):
        d_stored = A.nchw(outs[0][..., :c])
        ref = A.step_ref(case.xs, case.w, case.slope, res, case.pss, dt, d_used=d_stored)      # out from the d THE KERNEL STORED
        return [("d", d_stored.double(), ref.d, T._tol(ref.d, dt)), ("out", A.nchw(outs[1][..., :c]).double(), ref.out, T._tol(ref.out, dt) + ref.extra)]

    return Walk(launch, [(c, r8(c)), (c, r8(c))], values)


def resdb_step(compute, hw, n, nx, nd):
    import _resdn as R
    from ntire2022_esr_amd import ops
    case = R.step_case("random", compute, hw, nx, nd, n=PERIOD)
    xin = _rep(case["x"].to(DEV), n, PERIOD)
    ein = [_rep(e.to(DEV), n, PERIOD) for e in case["extras"]]

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, 16 * nd + 8), _sent(xin, hi - lo, hw, 56)]
        with ops.kernel_trace() as names:
            ops.resdb_step(xin[lo:hi], case["a_e"], case["w_e"], case["b_e"], case["a_c"], case["w_c"], case["b_c"],
                           extras=[(e[lo:hi], 0) for e in ein], d_out=outs[0], out=outs[1])
        return outs, names

    def values(outs):
        ref = R.case_ref(case)
        bd, by = R.step_bounds(case, ref)
        return [("dists", outs[0][..., :16 * nd].double(), ref["dists_raw"], bd), ("y", outs[1][..., :48].double(), ref["y_raw"], by)]

    return Walk(launch, [(16 * nd, 16 * nd), (48, 48)], values)


def conv_prelu(compute, hw, n):
    import _mdgn as M
    from ntire2022_esr_amd import ops
    case = M.conv_case("random", compute, hw, n=PERIOD)
    xin = _rep(case["x"].to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, 72)]
        with ops.kernel_trace() as names:
            ops.conv_prelu(xin[lo:hi], case["w"], case["b"], case["a"], out=outs[0])
        return outs, names

    def values(outs):
        ref = M.conv_case_ref(case)
        return [("y", outs[0][..., :64].double(), ref["f_raw"], M.one_store_bound(ref["f_raw"], case["dt"]))]

    return Walk(launch, [(64, 64)], values)


def mdsa_gate(compute, hw, n):
    import _mdgn as M
    from ntire2022_esr_amd import ops
    case = M.gate_case("random", compute, (PERIOD,) + hw)
    fin, xin = _rep(case["f"].to(DEV), n, PERIOD), _rep(case["x"].to(DEV), n, PERIOD)

    def launch(lo, hi):
        outs = [_sent(xin, hi - lo, hw, 72)]
        with ops.kernel_trace() as names:
            ops.mdsa_gate(fin[lo:hi], xin[lo:hi], case["w_f"], case["b_f"], case["a_f"], case["w_s"], case["b_s"], out=outs[0])
        return outs, names

    def values(outs):
        ref = M.gate_case_ref(case)
        return [("y", outs[0][..., :64].double(), ref["y_raw"], M.one_store_bound(ref["y_raw"], case["dt"]))]

    return Walk(launch, [(64, 64)], values)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
# One form per kernel instantiation its own suite reaches.  Widths come from that suite's own list: the network's (the main instantiation, all
# three shapes) and, where a template argument changes the staging, one more width per value of it ((17, 15) only).
#   unit    "t16": tiles of 16 x 16; "chain2" / "chain3": rlfb_chain_kernel's jobs at strip width G; "g16": groups of 16 pixels
#   round   work items of one round of the grid;  rounds: the batch is the smallest with more than this many rounds, plus one image
#   period  the batch is base[i % period].  3, as the thin-batch suite, where no block then meets the same tile of the same base image twice in a
#           row (tests/test_walk_table.py); the chain's last, un-swizzled round is 225 jobs behind block 1's fourth job, a multiple of 3 (and
#           of 5; a full round of 256 is one of 4), and at (17, 15) a job is a whole image: its batches repeat 7 images
def _f(id, kernel, args, run, main=True, unit="t16", round=GRID, rounds=4, period=PERIOD):
    return dict(id=id, kernel=kernel, args=args, run=run, shapes=SHAPES if main else SHAPES[:1], unit=unit, round=round, rounds=rounds,
                storages=("bf16", "f16"), period=period)


def _bf(compute):
    return TF[compute == "bf16"]


FORMS = [
    # both strip widths: G = 2 (single images) and G = 3 (batches) are both what RLFN launches, the launcher prices them per shape
    *[_f(f"chain-g{g}", "rlfb_chain_kernel", (lambda c, g=g: f"{_bf(c)}, {g}"), (lambda c, hw, n, g=g: rlfb_chain(c, hw, n, g, CHAIN_PERIOD)), unit=f"chain{g}",
         period=CHAIN_PERIOD)
      for g in (2, 3)],
    # hfab_kernel<.., NCH>: FMEN's (50, 16) has four chunks of x, HFAB_WIDTHS' (44, 16) three
    *[_f(f"hfab-{cin}-{cmid}", "hfab_kernel", (lambda c, cin=cin: f"{_bf(c)}, {(cin + 15) // 16}"),
         (lambda c, hw, n, a=(cin, cmid): hfab(c, hw, n, *a)), main) for cin, cmid, main in [(50, 16, True), (44, 16, False)]],
    # distill_step_kernel<.., NCH, RES>: BMDN_WIDTHS' two steps, and NEW_WIDTHS' (18, 24, 31) for two chunks without `+ in`
    *[_f("distill-" + "-".join(str(int(v)) for v in wd), "distill_step_kernel", (lambda c, wd=wd: f"{_bf(c)}, {(wd[0] + 15) // 16}, {TF[wd[3]]}"),
         (lambda c, hw, n, wd=wd: distill(c, hw, n, *wd)), main)
      for wd, main in [((40, 20, 20, False), True), ((20, 20, 20, True), False), ((18, 24, 31, False), False)]],
    # resblock_head_kernel<.., G>: with the `+ g` in front (every block but the first) and without
    *[_f(f"head-g{int(g)}", "resblock_head_kernel", (lambda c, g=g: f"{_bf(c)}, {TF[g]}"), (lambda c, hw, n, g=g: resblock_head(c, hw, n, g)), g)
      for g in (True, False)],
    _f("cascade", "refine_cascade_kernel", _bf, refine_cascade),
    _f("cx-50-200", "cx_block_kernel", _bf, (lambda c, hw, n: cx_block(c, hw, n, 50, 200))),
    _f("dwpw-50", "dwpw_pair_kernel", _bf, (lambda c, hw, n: dwpw_pair(c, hw, n, 50))),
    # pa_tail_kernel<.., NCH>: RePAFDN's 48 channels are three chunks, WIDTHS' 64 four
    *[_f(f"pa-tail-{ch}", "pa_tail_kernel", (lambda c, ch=ch: f"{_bf(c)}, {(ch + 15) // 16}"), (lambda c, hw, n, ch=ch: pa_tail(c, hw, n, ch)), main)
      for ch, main in [(48, True), (64, False)]],
    # asym_step_kernel<.., NKP, RES>: ARFDN_WIDTHS' first step (two K pairs) and third (one, `+ in`, both earlier maps); NEW_WIDTHS' (18, 24) for
    # one K pair without `+ in`
    *[_f("asym-" + "-".join(str(int(v)) for v in wd), "asym_step_kernel", (lambda c, wd=wd: f"{_bf(c)}, {2 if wd[0] > 32 else 1}, {TF[wd[2]]}"),
         (lambda c, hw, n, wd=wd: asym_step(c, hw, n, *wd)), main)
      for wd, main in [((50, 25, False, 0), True), ((25, 25, True, 2), False), ((18, 24, False, 1), False)]],
    # resdb_step_kernel<.., NX, ND>: RESDN_STEPS' first step, then its other two and OTHER_STEPS
    *[_f(f"resdb-{nx}-{nd}", "resdb_step_kernel", (lambda c, a=(nx, nd): f"{_bf(c)}, {a[0]}, {a[1]}"),
         (lambda c, hw, n, a=(nx, nd): resdb_step(c, hw, n, *a)), (nx, nd) == (0, 3))
      for nx, nd in [(0, 3), (1, 2), (2, 1), (0, 1), (0, 2), (1, 1), (1, 3), (2, 2), (2, 3)]],
    _f("conv-prelu", "conv_prelu_kernel", _bf, conv_prelu),
    # the group walkers: (33, 49) only, just over two rounds
    dict(_f("pa-gate-48", "pa_gate_kernel", (lambda c: {"bf16": "1", "f16": "2"}[c]), (lambda c, hw, n: pa_gate(c, hw, n, 48)),
            unit="g16", round=PA_ROUND, rounds=2), shapes=SHAPES[2:]),
    dict(_f("mdsa-gate", "mdsa_gate_kernel", _bf, mdsa_gate, unit="g16", round=MG_ROUND, rounds=2), shapes=SHAPES[2:]),
]


def symbol(form, compute):
    """what ops.kernel_trace() must report: the kernel with its template arguments"""
    return f"{form['kernel']}<{form['args'](compute)}>"


# ---- the launchers' arithmetic, restated -------------------------------------------------------------------------------------------------------
def chain_geometry(n, h, w, g):
    """chain_geometry_g (csrc/esr_chain.hip) at the forced strip width: (SX, SY) -- SX from the width, then the cheapest SY"""
    ws = 16 * g - 4
    sx, best, best_sy = (w + ws - 1) // ws, -1, 1
    for sy in range(1, min(max(h // 4, 1), 4096) + 1):
        rs = (h + sy - 1) // sy
        if (h + rs - 1) // rs != sy:
            continue
        cost = (n * sx * sy + 255) // 256 * (rs + 2 * CH_HALO) + CH_LAGP + 1
        if best < 0 or cost < best:
            best, best_sy = cost, sy
    return sx, best_sy


def items(form, hw, m):
    """the work items of a launch on m images: ceil(h / 16) ceil(w / 16) n tiles, n SX SY jobs, ceil(n h w / 16) groups"""
    if form["unit"] == "t16":
        return m * tiles_per_image(hw, "t16")
    if form["unit"] == "g16":
        return (m * hw[0] * hw[1] + 15) // 16
    sx, sy = chain_geometry(m, hw[0], hw[1], int(form["unit"][-1]))
    return m * sx * sy


def batch(form, hw):
    """tile walkers: _persist_cases.batch_for; the others the same rule on their own items: the smallest batch with more than `rounds` rounds,
    plus one image"""
    want = form["rounds"] * form["round"]
    if form["unit"] == "t16":
        return batch_for(hw, "t16", want + 1)
    n = 1
    while items(form, hw, n) <= want:
        n += 1
    return n + 1


def chunks(form, hw, n):
    """the fewest (nearly) equal consecutive chunks of at most one round of items each"""
    k = 1
    while any(items(form, hw, hi - lo) > form["round"] for lo, hi in chunk_bounds(n, k)):
        k += 1
    return chunk_bounds(n, k)


def walk_of(form, hw, n, lane):
    """the items one block (one wave of a block, for the group walkers) works on, in its order.  Tiles: t = b, b + G, ..; groups:
    g = b NW + wave, + grid NW, ..; the chain: s16_tile_index (csrc/esr_s16_dev.h) -- the XCD swizzle on full rounds, plain order on the last"""
    total = items(form, hw, n)
    grid = min(total, form["round"])
    if not form["unit"].startswith("chain"):
        return list(range(lane, total, grid))
    out = []
    for k in range((total + grid - 1) // grid):
        off = lane
        if grid % 8 == 0 and (k + 1) * grid <= total:
            off = (lane & 7) * (grid >> 3) + (lane >> 3)
        if k * grid + off < total:
            out.append(k * grid + off)
    return out


def item_key(form, hw, n, item):
    """(base image, position within the image) of a work item"""
    if form["unit"] == "g16":
        px = item * 16
        return px // (hw[0] * hw[1]) % form["period"], px % (hw[0] * hw[1])
    per = tiles_per_image(hw, "t16")
    if form["unit"].startswith("chain"):
        sx, sy = chain_geometry(n, hw[0], hw[1], int(form["unit"][-1]))
        per = sx * sy
    return item // per % form["period"], item % per


def rows():
    """every (form, storage, shape) of the table with its batch size"""
    for form in FORMS:
        for compute in form["storages"]:
            for hw in form["shapes"]:
                yield form, compute, hw, batch(form, hw)
