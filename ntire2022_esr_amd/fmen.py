"""FMEN (x4) on the HIP engine -- drop-in for `models.team03_fmen.FMEN` (team03_fmen.py:76-134; NTIRE 2022 ESR team 03, the runtime track's
runner-up).

Same constructor (no arguments) and the same 68 state_dict keys (`head`, `warmup.{0,1}`, `basic_blocks.{i}.conv{1,2}.rep_conv`,
`hfabs.{i}.{squeeze,convs.0.conv{1,2}.rep_conv,excitate}`, `lr_conv`, `tail.0`).  nf = 50 lives in NHWC buffers of pitch 56 (16-bit: the
tight pitch, as RFDN); the HFABs' 12 / 16-channel maps in buffers of pitch 16.  LeakyReLU slope 0.1 everywhere (team03_fmen.py:6-7).
Per HFAB (team03_fmen.py:60-73): squeeze + lrelu, the BasicBlocks' convs (conv1 + lrelu, conv2; the last one gets the outer lrelu), excitate,
sigmoid(.) * x as the conv's gate epilogue (L.RES_GATE).  16-bit plans with fuse_hfab: the four layers of a body HFAB as ONE launch
(Plan.hfab -> hfab_kernel); the warmup HFAB (mid 12, two BasicBlocks, one layer without activation) stays on per-layer launches.
The long skip (x = head(in), lr_conv(h) + x; team03_fmen.py:122-134) is the shared frame's (frame.py).
"""
from . import _lib as L
from .engine import HipSRModel
from .frame import LongSkip, _pad8, check_input, set_scale

SLOPE = 0.1


class FMEN(HipSRModel):
    def __init__(self):
        super().__init__()
        self.down_blocks = 4
        self.in_nc, self.out_nc, self.nf, self.upscale = 3, 3, 50, 4
        self.mid_feats = 16
        self.up_blocks = [2, 1, 1, 1, 1]
        self.scale_idx = 0
        # 16-bit plans: a body HFAB as one esr_conv_chain_s16 launch (hfab_kernel, res_mode L.RES_GATE).  OFF by default: at 32 x 256 x 256
        # bf16 the fused launch takes 0.59 ms per HFAB against 0.46 ms for the four launches it replaces (one 4-wave block per CU with its
        # staging latency exposed, 2x halo recompute); on one 339 x 510 image it is faster (FMEN)
        self._fuse_hfab = False
        nf = self.nf
        self._add_conv('head', self.in_nc, nf, 3)
        self._add_conv('warmup.0', nf, nf, 3)
        self._add_hfab('warmup.1', self.up_blocks[0], self.mid_feats - 4)
        for i in range(self.down_blocks):
            self._add_conv(f'basic_blocks.{i}.conv1.rep_conv', nf, nf, 3)
            self._add_conv(f'basic_blocks.{i}.conv2.rep_conv', nf, nf, 3)
        for i in range(self.down_blocks):
            self._add_hfab(f'hfabs.{i}', self.up_blocks[i + 1], self.mid_feats)
        self._add_conv('lr_conv', nf, nf, 3)
        self._add_conv('tail.0', nf, self.out_nc * self.upscale ** 2, 3)

    def _add_hfab(self, path, up_blocks, mid):
        self._add_conv(path + '.squeeze', self.nf, mid, 3)
        for j in range(up_blocks):
            self._add_conv(f'{path}.convs.{j}.conv1.rep_conv', mid, mid, 3)
            self._add_conv(f'{path}.convs.{j}.conv2.rep_conv', mid, mid, 3)
        self._add_conv(path + '.excitate', mid, self.nf, 3)

    fuse_hfab = property(lambda self: self._fuse_hfab, lambda self, v: self._set_flag("_fuse_hfab", v))

    set_scale = set_scale

    def _hfab(self, plan, path, up_blocks, x, y, ta, tb, mid, fuse):
        """HFAB(x) -> y (team03_fmen.py:67-73): lrelu(squeeze), [conv1 + lrelu, conv2] x up_blocks with the outer lrelu on the last conv2,
        sigmoid(excitate) * x"""
        act = dict(act=L.ACT_LRELU, slope=SLOPE)
        mark = len(plan.ops)
        plan.conv(path + '.squeeze', x, ta, self.nf, mid, **act)
        cur, nxt = ta, tb
        for j in range(up_blocks):
            plan.conv(f'{path}.convs.{j}.conv1.rep_conv', cur, nxt, mid, mid, **act)
            last = j == up_blocks - 1
            plan.conv(f'{path}.convs.{j}.conv2.rep_conv', nxt, cur, mid, mid, **(act if last else dict(slope=SLOPE)))
        plan.conv(path + '.excitate', cur, y, mid, self.nf, res=x, res_mode=L.RES_GATE)
        if fuse:
            plan.hfab(mark)

    def _build_plan(self, plan, c):
        check_input('FMEN', plan, c, self.in_nc, esa=False)
        if plan.store == "f16":
            # the checkpoint's HFAB intermediates reach ~2e7 on natural images (warmup.1.convs.1.conv2; the sigmoid saturates them): beyond
            # fp16's 65504, the forward would overflow to Inf / NaN.  bf16 has fp32's exponent range
            raise L.EsrError("FMEN: fp16 storage cannot hold the HFAB activations (|v| up to ~2e7 > 65504); use compute 'bf16' or 'f32'")
        nf = self.nf
        # 16-bit storage: nf-wide tensors at the tight pitch round_up(nf, 8) = 56 (esr_conv2d_s16: tight pitch; hfab_kernel reads cin channels)
        P = _pad8(nf) if (plan.esize == 2 and self.tight_pitch) else plan.cpad(nf)
        M = plan.cpad(self.mid_feats)
        skip = LongSkip(plan, self, nf, P, name='x')
        ha, hb = plan.buffer('ha', P), plan.buffer('hb', P)
        ta, tb = plan.buffer('ta', M), plan.buffer('tb', M)
        act = dict(act=L.ACT_LRELU, slope=SLOPE)
        fuse = self.fuse_hfab and plan.esize == 2
        skip.head('head', self.in_nc)
        plan.conv('warmup.0', skip.fea, ha, nf, nf)
        self._hfab(plan, 'warmup.1', self.up_blocks[0], ha, hb, ta, tb, self.mid_feats - 4, False)
        h, u = hb, ha
        for i in range(self.down_blocks):
            # BasicBlock (team03_fmen.py:36-42): h -> u -> h (h is consumed by conv1), then HFAB(h) -> u
            plan.conv(f'basic_blocks.{i}.conv1.rep_conv', h, u, nf, nf, **act)
            plan.conv(f'basic_blocks.{i}.conv2.rep_conv', u, h, nf, nf)
            self._hfab(plan, f'hfabs.{i}', self.up_blocks[i + 1], h, u, ta, tb, self.mid_feats, fuse and self.up_blocks[i + 1] == 1)
            h, u = u, h
        skip.close('lr_conv', 'tail.0', h, u, self.out_nc * 16)

    def _counted_convs(self, plan, o):
        """FMEN's LeakyReLU is one module-level object (team03_fmen.py:6-7), not a submodule: utils/model_summary.py's hooks never see it, so the
        reference's FLOPs are the conv MACs alone"""
        return [(ci, co, k, npix, L.ACT_NONE) for (ci, co, k, npix, _) in super()._counted_convs(plan, o)]
