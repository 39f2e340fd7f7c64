"""ARFDN (x4) on the HIP engine -- drop-in for `models.team14_arfdn.ARFDN.ARFDN` (ARFDN.py:6-37 + block.py; NTIRE 2022 ESR team 14,
test_demo.py id 14, data_range 1.0).

Same constructor keywords and the same 200 state_dict keys (`fea_conv`, `B{k}.{c0_d,c1_d,c2_d}`, `B{k}.c{j}_{l1,l2,m1,m2}`, `B{k}.{c4,c5}`,
`B{k}.mpa.{conv1,conv_f,conv_max,conv2,conv3,conv3_,conv4}`, `c.0`, `LR_conv`, `upsampler.0`).  It is RFDN's frame (frame.py) at nf = 50
with LeakyReLU(0.05), ReLU and sigmoid only; `c.1` is LeakyReLU(0.1) (block.py:67: conv_block passes no slope).  Its block, ARFDB
(block.py:195-262), replaces every 3x3 of RFDB's refinement path by two ASYMMETRIC PAIRS over dc = 25 channels; step j = 1, 2, 3 on r_0 = the
block input (50 channels), r_1, r_2 (25 channels):

    d_j = act(c{j-1}_d(r))                                        1x1
    a_l = act(c{j}_l1(r))   3x1        a_m = act(c{j}_m1(r))      1x3
    r_j = act(c{j}_l2(a_l) + c{j}_m2(a_m) [+ r, j >= 2] + d_j + .. + d_1)          1x3 / 3x1

then r4 = act(c4(r_3)), c5 over cat(d1, d2, d3, r4) and the baseline ESA with f = 12 (named `mpa`).

A step has two forms (model.fuse_asym):
  per-layer  three launches on the existing kernels; the only form of an fp32 plan.  A 3x1 or 1x3 is a 3x3 with six zero taps:
             d_j = act(1x1(r));  [a_l | a_m] = act(P (*) r), ONE 3x3 r -> 50 channels whose weight is plus-shaped (c{j}_l1 in the middle
             column, c{j}_m1 in the middle row);  r_j = act(Q (*) [d_j .. d_1 | a_l | a_m] [+ r]), ONE 3x3 over a channel range of the
             block's concat buffer with c{j}_l2 in the middle row, c{j}_m2 in the middle column and identity centre taps for every
             distilled map (fold_a / fold_b below); r is that launch's residual.  16-bit plans round a_l and a_m to the storage type, as
             every stored tensor.  Executed MACs per pixel: 9 cin 50 + 9 K 25 with K = 96 / 128 / 160 physical slots (a 16-bit plan's third
             step: 128, after an identity 1x1), against the 3 (2 cin 25 + 2 25 25) the reference counts: 3.9x / 5.3x / 6.3x in steps
             1 / 2 / 3.
  fused      ONE esr_asym_step launch (Plan.asym_step, asym_step_kernel; 16-bit plans): r is read once, d_j and r_j are written once,
             a_l and a_m stay in LDS, the MFMA K dimension is three taps.  Not bit-identical to the per-layer form (another summation
             order; the 3-tap weights are rounded once where pack_conv_s16 diffuses the error over a 3x3's taps).
Which form a plan takes depends on the flag, the per-image shape and esr_asym_step_supported only, never on the batch size.

The layouts: nf = 50 as in rfdn.py (pitch 56 / 64); r_1 .. r_3 ping-pong between two buffers of their own (a step never stores into its
input's tensor: the neighbouring tiles read the halo); the block's other maps are channel slices of ONE 224-wide buffer,
[r4 | d2 | d1 | a_l a_m (64) | d3 | q], ordered so that every step's second convolution reads ONE contiguous channel range that holds only
tensors already written in this block -- [d_1 | a], [d_2 d_1 | a], [d_2 d_1 | a | d_3] (a 16-bit plan: [a | d_3 | q] with q = d_2 + d_1, see
_step) -- and c5 reads the first 192 slots through its cin_map.  Slices and not dense tensors in 16-bit plans too: the existing 16-bit
kernels run a 3x3 over one tensor only.  `+ r` is the second convolution's pre-activation residual.  torch.cat never runs.
"""
import torch
import torch.nn as nn

from . import _lib as L
from .engine import S16, HipSRModel, Post, Conv, pack_conv, pack_conv_s16
from .frame import FP, Concat, EsaBranch, LongSkip, _pad8, _slice_map, block_cin_map, check_input, set_scale

SEG = 32                                                   # slice width of the block's maps
R4, D2, D1, A, D3, Q = 0, 32, 64, 96, 160, 192             # first slot of each slice of the block buffer; a_l | a_m: 64 slots
SPITCH = 224
KMAX = 144                                                 # physical input channels of a 3x3 on conv_s16_kernel: nine K chunks' weights stay resident
FOLD_Q = "#q"                                              # the identity 1x1 of a 16-bit plan's d_2 + d_1, under the name of c3_l2
FOLD_A, FOLD_B = "#a", "#b"                                # the folded 3x3s of the per-layer form, under the names of c{j}_l1 / c{j}_l2


def fold_a(w_l1, b_l1, w_m1, b_m1):
    """c_l1 [dc, cin, 3, 1] and c_m1 [dc, cin, 1, 3] over the same input as ONE 3x3 -> [a_l | a_m]: a plus-shaped weight [2 dc, cin, 3, 3]"""
    dc, cin = w_l1.shape[:2]
    w = torch.zeros(2 * dc, cin, 3, 3, dtype=w_l1.dtype)
    w[:dc, :, :, 1] = w_l1[:, :, :, 0]
    w[dc:, :, 1, :] = w_m1[:, :, 0, :]
    return w, torch.cat([b_l1, b_m1])


def fold_b(w_l2, b_l2, w_m2, b_m2, slots, a0, ident):
    """c_l2 [dc, dc, 1, 3] over a_l and c_m2 [dc, dc, 3, 1] over a_m plus the residuals as ONE 3x3 over `slots` physical channels: a_l at slots
    a0 .. a0 + dc - 1 (middle row), a_m behind it (middle column), an identity centre tap for the dc-channel tensor at every slot of `ident`"""
    dc = w_l2.shape[0]
    w = torch.zeros(dc, slots, 3, 3, dtype=w_l2.dtype)
    w[:, a0:a0 + dc, 1, :] = w_l2[:, :, 0, :]
    w[:, a0 + dc:a0 + 2 * dc, :, 1] = w_m2[:, :, :, 0]
    for s in ident:
        w[torch.arange(dc), s + torch.arange(dc), 1, 1] = 1.0
    return w, b_l2 + b_m2


class ARFDN(HipSRModel):
    def __init__(self, in_nc=3, out_nc=3, nf=50, num_modules=4):
        super().__init__()
        if nf != 50 or num_modules != 4 or in_nc > 4 or out_nc > 4:
            raise NotImplementedError('HIP ARFDN supports nf=50, num_modules=4, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, 4
        self.dc = nf // 2                                  # block.py:198
        self.f = nf // 4                                   # block.py:139
        self.scale_idx = 0
        dc, f = self.dc, self.f
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            for j in (1, 2, 3):
                cin = nf if j == 1 else dc
                self._add_conv(b + f'c{j - 1}_d', cin, dc, 1)
                # the asymmetric pairs: parameter holders with the reference's shapes, folded by _extra_pack; as they are: Plan.asym_step
                self._add_leaf(b + f'c{j}_l1', nn.Conv2d(cin, dc, (3, 1), 1, (1, 0)))
                self._add_leaf(b + f'c{j}_l2', nn.Conv2d(dc, dc, (1, 3), 1, (0, 1)))
                self._add_leaf(b + f'c{j}_m1', nn.Conv2d(cin, dc, (1, 3), 1, (0, 1)))
                self._add_leaf(b + f'c{j}_m2', nn.Conv2d(dc, dc, (3, 1), 1, (1, 0)))
            self._add_conv(b + 'c4', dc, dc, 3)
            c5_map = [-1] * (D3 + SEG)                     # slots [r4 | d2 | d1 | a_l a_m | d3] -> cat(d1, d2, d3, r4), block.py:259
            for s0, seg in ((R4, 3), (D3, 2), (D2, 1), (D1, 0)):
                c5_map[s0:s0 + dc] = range(seg * dc, (seg + 1) * dc)
            self._add_conv(b + 'c5', dc * 4, nf, 1, cin_map=c5_map)
            self._add_conv(b + 'mpa.conv1', nf, f, 1)
            self._add_conv(b + 'mpa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'mpa.conv_max', f, f, 3)
            self._add_conv(b + 'mpa.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'mpa.conv3', f, f, 3)
            self._add_conv(b + 'mpa.conv3_', f, f, 3)
            self._add_conv(b + 'mpa.conv4', f, nf, 1, dense=(FP, (nf + 3) // 4 * 4))
        self._add_conv('c.0', nf * num_modules, nf, 1, cin_map=_slice_map(num_modules, nf, _pad8(nf)))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * 16, 3)

    set_scale = set_scale

    @staticmethod
    def _step(j, s16=False):
        """(d_j's slot, the slots of the earlier distilled maps, the slot range [lo, hi) the second convolution reads, the slots of its
        identity taps).  Steps 1 and 2 read [d_j .. d_1 | a_l a_m]; step 3 reads [d_2 d_1 | a_l a_m | d_3], 160 slots.  That is more than
        conv_s16_kernel keeps resident (KMAX), so a 16-bit plan's third step first stores q = d_2 + d_1 (an identity 1x1 of d_2 with the
        residual d_1: ONE more rounding than the reference's sum has, in this form only) and reads [a_l a_m | d_3 | q], 128 slots."""
        if j == 3 and s16:
            return D3, (D2, D1), (A, Q + SEG), (D3, Q)
        return {1: (D1, (), (D1, A + 2 * SEG), (D1,)), 2: (D2, (D1,), (D2, A + 2 * SEG), (D2, D1)),
                3: (D3, (D2, D1), (D2, D3 + SEG), (D3, D2, D1))}[j]

    def _build_plan(self, plan, c):
        check_input('ARFDN', plan, c, self.in_nc)
        nf, dc, f = self.nf, self.dc, self.f
        s16 = plan.esize == 2
        KP = plan.cpad(nf)
        P = _pad8(nf) if (s16 and self.tight_pitch) else KP          # rfdn.py: the nf-wide tensors at the tight pitch in 16-bit plans
        skip = LongSkip(plan, self, nf, P)
        bcat = Concat(plan, 'bcat', 4, P, s16)
        S = plan.buffer('blk', SPITCH)                    # [r4 | d3 | d2 | d1 | a_l a_m]
        ra, rb = plan.buffer('ra', plan.cpad(dc)), plan.buffer('rb', plan.cpad(dc))
        v = plan.buffer('v', P)
        lr = None if skip.hl else plan.buffer('lr', P)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        act = dict(act=L.ACT_LRELU, slope=0.05)
        skip.head('fea_conv', self.in_nc)
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            r = cur
            for j, out in ((1, ra), (2, rb), (3, ra)):
                dj, ps, (lo, hi), _ = self._step(j)
                cin = nf if j == 1 else dc
                res = dict(res=r, res_mode=L.RES_PRE_ACT) if j > 1 else {}             # block.py:240: no `+ input` in the first step
                mark = len(plan.ops)
                plan.conv(b + f'c{j - 1}_d', r, S[dj:dj + SEG], cin, dc, k=1, **act)
                plan.conv(b + f'c{j}_l1' + FOLD_A, r, S[A:A + 2 * SEG], cin, 2 * dc, counted=False, **act)
                plan.conv(b + f'c{j}_l2' + FOLD_B, S[lo:hi], out, hi - lo, dc, counted=False, **res, **act)
                # (where the kernel takes the step; else the three launches stay)
                fused = self.fuse_asym and s16 and plan.asym_step(mark, [b + f'c{j}_{n}' for n in ('l1', 'm1', 'l2', 'm2')], p=[S[s:s + SEG] for s in ps])
                if s16 and j == 3 and not fused:                                      # 160 slots: q = d_2 + d_1 first (_step)
                    _, _, (lo, hi), _ = self._step(j, True)
                    del plan.ops[-1]
                    plan.conv(b + f'c{j}_l2' + FOLD_Q, S[D2:D2 + SEG], S[Q:Q + SEG], dc, dc, k=1, counted=False, res=S[D1:D1 + SEG], res_mode=L.RES_PRE_ACT)
                    plan.conv(b + f'c{j}_l2' + FOLD_B, S[lo:hi], out, hi - lo, dc, counted=False, **res, **act)
                r = out
            plan.conv(b + 'c4', r, S[R4:R4 + SEG], dc, dc, **act)
            c5 = dict(w=b + 'c5', src=S[0:D3 + SEG], dst=v, cin=D3 + SEG, cout=nf, k=1, cin_alg=4 * dc)
            ride = Conv(**c5, post=Post(b + 'mpa.conv1', c1, f, L.ACT_NONE)) if s16 else None
            if ride is not None and plan.post_supported(ride):
                plan.ops.append(ride)                     # esa.conv1 on the fp32 tile in c5's epilogue (rfdn.py)
            else:
                plan.ops.append(Conv(**c5))
                plan.conv(b + 'mpa.conv1', v, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'mpa.conv2', [(b + 'mpa.conv_max', L.ACT_RELU), (b + 'mpa.conv3', L.ACT_RELU), (b + 'mpa.conv3_', L.ACT_NONE)],
                            self.fuse_esa_lowres)
            out = bcat.seg(k - 1)
            plan.esa_apply(b + 'mpa.conv_f', b + 'mpa.conv4', v, c1, c3, out, nf, f)
            cur = out
        plan.conv('c.0', bcat.whole, v, 4 * KP, nf, k=1, cin_alg=4 * nf, act=L.ACT_LRELU, slope=0.1)      # c.1 = LeakyReLU(0.1)
        skip.close('LR_conv', 'upsampler.0', v, lr, self.out_nc * 16)

    _cin_map = block_cin_map

    def _extra_pack(self, packed, device):
        store = self._store()
        cpu = lambda t: t.detach().to("cpu", torch.float32)
        for k in range(1, 5):
            for j in (1, 2, 3):
                b = f'B{k}.c{j}_'
                l1, l2, m1, m2 = (self._leaf(b + n) for n in ('l1', 'l2', 'm1', 'm2'))
                wa, ba = fold_a(cpu(l1.weight), cpu(l1.bias), cpu(m1.weight), cpu(m1.bias))
                fb = lambda s16: fold_b(cpu(l2.weight), cpu(l2.bias), cpu(m2.weight), cpu(m2.bias), self._step(j, s16)[2][1] - self._step(j, s16)[2][0],
                                        A - self._step(j, s16)[2][0], [s - self._step(j, s16)[2][0] for s in self._step(j, s16)[3]])
                self._pack_own(packed, device, b + 'l1' + FOLD_A, wa, ba)
                packed[b + 'l2' + FOLD_B] = pack_conv(*fb(False)).to(device)
                if store != "f32":
                    packed[b + 'l2' + FOLD_B + S16] = pack_conv_s16(*fb(True), store).to(device)
                    if j == 3:
                        packed[b + 'l2' + FOLD_Q + S16] = pack_conv_s16(torch.eye(self.dc)[:, :, None, None], torch.zeros(self.dc), store).to(device)

    def _complexity_terms(self, plan, o):
        """the folded 3x3s stand for two nn.Conv2d calls of three taps each (block.py:236-254); the activation of a step's sum is a call of
        the block's LeakyReLU like those behind c{j}_l1 / c{j}_m1"""
        if o.kind == "asym":
            terms = [self._complexity_terms(plan, q) for q in o.replaces]
            return tuple(sum(t[i] for t in terms) for i in range(3))
        if o.kind == "conv" and o.w.endswith(FOLD_A):
            return 2 * (3 * o.cin_alg * self.dc + self.dc) * plan.npix, 2 * self.dc * plan.npix, 2
        if o.kind == "conv" and o.w.endswith(FOLD_B):
            return 2 * (3 * self.dc * self.dc) * plan.npix + self.dc * plan.npix, 2 * self.dc * plan.npix, 2
        return super()._complexity_terms(plan, o)
