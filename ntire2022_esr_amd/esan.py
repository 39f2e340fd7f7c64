"""ESAN (x4) on the HIP engine -- drop-in for `models.team34_esan.ESAN` at level 1 (team34_esan.py:78-124; NTIRE 2022 ESR team 34, test_demo.py
`make_model(1)`, data_range 255).

Same constructor keywords and the same 262 state_dict keys (`upconv0`, `conv_first.0`, `recon_trunk.0.{0..15}.{conv1, conv2,
ESA.{conv1, conv2, conv3_1, conv3_2, conv3_3, conv4}}`, `upconv.0`).  A trunk of 16 identical residual blocks at nf = 32,

    x' = x + ESA(conv2(relu(conv1(x))))                                                     (ResidualBlock_ESA, team34_esan.py:71-76)

whose ESA (:48-58) is the baseline's with f = 8, three 3x3s on the pooled map (ReLU, ReLU, none) and no conv_f: `conv4(bilinear(c3) + c1_)` runs
on esr_esa_apply_f32 with an identity conv_f (rfdn.py, esa_conv_f=False), which is not counted as a convolution.  The output is
PixelShuffle(upconv0(x_in) + upconv.0(trunk)) (:117-123); the shuffle is a permutation, so the sum is taken in the 48-channel domain:
  fp32     upconv0(x_in) goes to a 48-channel buffer that the output convolution adds before it stores (its pre-activation residual)
  16-bit   ONE 3x3 over [trunk | x_in] with the weights cat([W_upconv.0, W_upconv0], 1) and the bias b + b0 (`upconv.0#fold`): the trunk and the
           packed input (esr_pack_input_s16: hi and lo halves, so the image term keeps ~fp32 accuracy in bf16 too) share one 48-channel buffer.
32 channels are exactly two 16-bit K chunks and one 64-byte run per pixel: no pitch is padded.

The head of a block -- the `+` of the previous block, conv1, conv2 and ESA.conv1 -- has two forms (model.fuse_head):
  per-op   four launches on the existing kernels: x = x_prev + g as a 1x1 with identity weights, zero bias and the residual x_prev (exact in
           fp32; a 16-bit plan rounds g = u * sigmoid(..) to the storage type before the sum, once more than the reference's graph does),
           t = relu(conv1(x)), u = conv2(t), c1 = ESA.conv1(u).  The only form of an fp32 plan.
  fused    ONE esr_resblock_head_s16 launch (resblock_head_kernel; Plan.resblock_head): the previous x and g are read once, x, u and c1 are
           written once, t stays in LDS.  It stores what the four launches store.  The last block's `+` in front of the output convolution
           stays a per-op launch.  Measurements: DESIGN.md 7e.
Which form a plan takes depends on the per-image shape and esr_resblock_head_supported only, never on the batch size.

ESA's maps and its low-resolution branch are the shared frame's (frame.py); ESAN has no long skip.
"""
import torch

from . import _lib as L
from .engine import FOLD, HEAD, INPUT, OUTPUT, S16, Conv, HipSRModel, Pack
from .frame import FP, EsaBranch, check_input, identity_conv_f

IDENT = "ident"     # the blob of the 32 -> 32 identity 1x1 behind every `x + g`


class ESAN(HipSRModel):
    def __init__(self, in_nc=3, out_nc=3, nf=32, level=1, upscale=4):
        super().__init__()
        if level != 1 or upscale != 4 or nf != 32 or in_nc > 4 or out_nc != 3:
            raise NotImplementedError('HIP ESAN supports level=1, upscale=4, nf=32, in_nc <= 4, out_nc=3')
        self.in_nc, self.out_nc, self.nf, self.level, self.upscale = in_nc, out_nc, nf, level, upscale
        self.f = nf // 4                         # team34_esan.py:38
        self.n_blocks = 16                       # team34_esan.py:91
        nf, f = self.nf, self.f
        self._add_conv('upconv0', in_nc, out_nc * 16, 3)
        self._add_conv('conv_first.0', in_nc, nf, 3)
        for k in range(self.n_blocks):
            b = f'recon_trunk.0.{k}.'
            self._add_conv(b + 'conv1', nf, nf, 3)
            self._add_conv(b + 'conv2', nf, nf, 3)
            self._add_conv(b + 'ESA.conv1', nf, f, 1)
            self._add_conv(b + 'ESA.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'ESA.conv3_1', f, f, 3)
            self._add_conv(b + 'ESA.conv3_2', f, f, 3)
            self._add_conv(b + 'ESA.conv3_3', f, f, 3)
            self._add_conv(b + 'ESA.conv4', f, nf, 1, dense=(FP, nf))
        self._add_conv('upconv.0', nf, out_nc * 16, 3)

    def _build_plan(self, plan, c):
        check_input('ESAN', plan, c, self.in_nc)
        nf, f, co = self.nf, self.f, self.out_nc * 16
        s16 = plan.esize == 2
        xa, xb = plan.buffer('xa', nf), plan.buffer('xb', nf)             # the trunk, ping-pong: x' is never stored over the x it is made from
        t, u, g = plan.buffer('t', nf), plan.buffer('u', nf), plan.buffer('g', nf)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        if s16:
            # [trunk (32) | the packed input's 16 slots]: the output convolution's folded 3x3 reads both, the head convolution the slots
            cat = plan.buffer('cat', nf + 16)
            x16, last = (cat, nf, 16), (cat, 0, nf)
            plan.ops.append(Pack(x16, self.in_nc))
            plan.ops.append(Conv('conv_first.0' + HEAD, x16, xa, self.in_nc, nf, head=self.in_nc))
        else:
            up0, last = plan.buffer('up0', co), None
            plan.conv('upconv0', INPUT, up0, self.in_nc, co)
            plan.conv('conv_first.0', INPUT, xa, self.in_nc, nf)
        cur = xa
        for k in range(self.n_blocks):
            b = f'recon_trunk.0.{k}.'
            mark = len(plan.ops)
            if k:                                             # the previous block's `identity + out` (team34_esan.py:76)
                nxt = xb if cur is xa else xa
                plan.conv(IDENT, g, nxt, nf, nf, k=1, res=cur, res_mode=L.RES_PRE_ACT, counted=False)
                cur = nxt
            plan.conv(b + 'conv1', cur, t, nf, nf, act=L.ACT_RELU)
            plan.conv(b + 'conv2', t, u, nf, nf)
            plan.conv(b + 'ESA.conv1', u, c1, nf, f, k=1)
            if self.fuse_head and s16:
                plan.resblock_head(mark)                      # (where the kernel takes the head; else the launches stay)
            c3 = esa.lowres(b + 'ESA.conv2', [(b + 'ESA.conv3_1', L.ACT_RELU), (b + 'ESA.conv3_2', L.ACT_RELU), (b + 'ESA.conv3_3', L.ACT_NONE)],
                            self.fuse_esa_lowres)
            plan.esa_apply(b + 'ESA.conv_f', b + 'ESA.conv4', u, c1, c3, g, nf, f)
        if s16:
            plan.conv(IDENT, g, last, nf, nf, k=1, res=cur, res_mode=L.RES_PRE_ACT, counted=False)
            plan.conv('upconv.0' + FOLD, cat, OUTPUT, nf + 16, co, cin_alg=nf + self.in_nc)
        else:
            last = xb if cur is xa else xa
            plan.conv(IDENT, g, last, nf, nf, k=1, res=cur, res_mode=L.RES_PRE_ACT, counted=False)
            plan.conv('upconv.0', last, OUTPUT, nf, co, res=up0, res_mode=L.RES_PRE_ACT)

    def _extra_pack(self, packed, device):
        from .engine import pack_conv_s16
        store = self._store()
        eye, zero = torch.eye(self.nf)[:, :, None, None], torch.zeros(self.nf)
        self._pack_own(packed, device, IDENT, eye, zero)
        conv_f = identity_conv_f(self.f, device)
        for k in range(self.n_blocks):
            packed[f'recon_trunk.0.{k}.ESA.conv_f'] = conv_f
        if store != "f32":
            # upconv.0 over the trunk and upconv0 over the packed input [x_hi | x_lo | x_hi] as ONE 3x3: upconv0's weights as [w_hi | w_hi | w_lo]
            # (engine.pack_head_s16), the biases added
            up, up0 = self._leaf('upconv.0'), self._leaf('upconv0')
            w0 = up0.weight.detach().float().cpu()
            hi = w0.to(torch.bfloat16 if store == "bf16" else torch.float16).float()
            w = torch.cat([up.weight.detach().float().cpu(), hi, hi, w0 - hi], dim=1)
            bias = up.bias.detach().float().cpu() + up0.bias.detach().float().cpu()
            packed['upconv.0' + FOLD + S16] = pack_conv_s16(w, bias, store, cin_phys=self.nf + 16).to(device)

    def _counted_convs(self, plan, o):
        """the reference's hooks see upconv0 and upconv.0 as two convolutions, no conv_f, and no module behind conv1 (F.relu is a function)"""
        r = super()._counted_convs(plan, o)
        if o.kind == "apply":
            return r[1:]
        if o.kind == "conv" and o.w == 'upconv.0' + FOLD:
            return [(self.in_nc, o.cout, 3, plan.npix, L.ACT_NONE), (self.nf, o.cout, 3, plan.npix, L.ACT_NONE)]
        return [(ci, co, k, npix, L.ACT_NONE) if (k == 3 and ci == self.nf and co == self.nf) else (ci, co, k, npix, act) for ci, co, k, npix, act in r]
