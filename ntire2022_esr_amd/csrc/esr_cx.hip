// esr_cx.hip -- the ConvNeXt block `CX` that ends RFDNeXt's RFDB (team38_rfdnext/rfdn_block.py:132-144):
//
//     t   = rnd(dw7(v) + b0)                       depthwise 7x7, zero padding, C -> C
//     h   = rnd(lrelu(W1 . t + b1))                1x1, C -> 4 C
//     out = rnd(W2 . h + b2 + v)                   1x1, 4 C -> C
//
// rnd = one rounding to the storage type.  Two things live here:
//
// dwconv7x7_kernel<ST> (esr_dwconv7x7; fp32, bf16 and fp16 storage): nn.Conv2d(C, C, 7, 1, 3, groups=C) on an NHWC tensor.  A thread owns
// four channels of one pixel, the [tap][c_p] weights sit in LDS, the taps are summed in fp32 with fmaf in (ky, kx) ascending order from 0,
// the bias is added last and the sum is rounded once.  The per-op form's first step and the only form of an fp32 plan.
//
// cx_block_kernel<BF16> (esr_cx_block_s16; 16-bit storage): the whole block as ONE launch.  As three launches a pixel moves about 1.36 KB
// through HBM at C = 50 (the 4 C hidden tensor twice); here v is read once and out written once: 224 bytes.  A 4-wave block owns one
// 16 x 16 output tile at a time (persistent over the tiles) and keeps in LDS
//
//     v    22 x 22 pixels  [pixel][128 B]   staged with a THREE-pixel halo by LDS-DMA, 16-byte pieces; the pieces outside the image and the
//                                           pieces behind round_up(C, 8) channels are requested out of range and arrive as zeros
//     t    16 x 16 pixels  [pixel][128 B]   dw7 of the tile, rounded: the first GEMM's B operand
//     W1, W2, b1, b2                        the two 1x1 weight images (esr_pack_cx_pw1_s16 / esr_pack_cx_pw2_s16), resident
//
// dw7 runs on the VALU: a thread owns a channel PAIR (its 49 x 2 weights in registers for the block's lifetime) and two rows of the tile;
// per row and ky it reads the 22 staged pixels of that pair once and slides the seven taps over them -- the same fmaf chain per output as
// dwconv7x7_kernel, so t is bit-identical to what that kernel stores.  The 1x1s run on v_mfma_f32_16x16x32: per 32 hidden channels (two
// output tiles of W1, bias as C) the accumulators are activated, rounded and packed, and ARE the B fragment of W2's next K step: lane
// (pixel, kq) holds hidden channels 4 kq .. 4 kq + 3 of both tiles, and esr_pack_cx_pw2_s16 orders W2's K that way.  The hidden tensor
// never leaves registers.  Then + b2 (W2's C operand), + v from the staged tile in fp32, one rounding, store.
// Numerics: each of t, h and out is rounded exactly where the per-op form stores it.  The weights are W1 and W2 rounded once to the
// storage type (the per-op 1x1s of conv_s16_kernel multiply by hi + lo pairs) and the K order is one pass over 64 / 32 channels, so the
// result is NOT bit-identical to the three launches; every stage stays within one rounding of its fp64 restatement on the effective weights.
// Pad channels: weight rows / columns and biases beyond C and 4 C are zero in the blobs; channels C .. post_cout - 1 of the output are
// stored as zeros.  LDS 158 KB, one block per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

// ---- depthwise 7x7 ---------------------------------------------------------------------------------------------------------------------------
constexpr int DW7_TAPS = 49;
constexpr int CX_CMAX = 64;

struct Dw7K {
    const void* x; const float* wp; void* y;
    int N, H, W, cp, nq;          // cp: channel pitch of the blob (round_up(C, 8)), nq: channel quads per pixel
    int x_pitch, x_coff, y_pitch, y_coff;
};

template <int ST>
__device__ __forceinline__ f32x4 cx_ld4(const void* p, size_t idx)
{
    if (ST == ESR_STORE_F32) return *reinterpret_cast<const f32x4*>(static_cast<const float*>(p) + idx);
    return unpack4<ST == ESR_STORE_BF16>(*reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p) + idx));
}

template <int ST>
__device__ __forceinline__ void cx_st4(void* p, size_t idx, f32x4 v)
{
    if (ST == ESR_STORE_F32) {
        *reinterpret_cast<f32x4*>(static_cast<float*>(p) + idx) = v;
    } else {
        uint2 u;
        u.x = pack2<ST == ESR_STORE_BF16>(v.x, v.y);
        u.y = pack2<ST == ESR_STORE_BF16>(v.z, v.w);
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p) + idx) = u;
    }
}

template <int ST>
__global__ __launch_bounds__(256) void dwconv7x7_kernel(const Dw7K p)
{
    extern __shared__ __attribute__((aligned(16))) float sdw7[];         // 50 * cp floats
    for (int i = threadIdx.x; i < (DW7_TAPS + 1) * p.cp; i += 256) sdw7[i] = p.wp[i];
    __syncthreads();
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pix = gid / p.nq;
    const int q = (int)(gid - pix * p.nq);
    if (pix >= (long long)p.N * p.H * p.W) return;
    const int ox = (int)(pix % p.W);
    const int oy = (int)((pix / p.W) % p.H);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 7; ++ky) {
        const int iy = oy + ky - 3;
        if (iy < 0 || iy >= p.H) continue;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = ox + kx - 3;
            if (ix < 0 || ix >= p.W) continue;
            const f32x4 xv = cx_ld4<ST>(p.x, (size_t)(pix + (long long)(ky - 3) * p.W + (kx - 3)) * p.x_pitch + p.x_coff + q * 4);
            const f32x4 wv = *reinterpret_cast<const f32x4*>(sdw7 + (ky * 7 + kx) * p.cp + q * 4);
            acc.x = fmaf(xv.x, wv.x, acc.x); acc.y = fmaf(xv.y, wv.y, acc.y);
            acc.z = fmaf(xv.z, wv.z, acc.z); acc.w = fmaf(xv.w, wv.w, acc.w);
        }
    }
    acc += *reinterpret_cast<const f32x4*>(sdw7 + DW7_TAPS * p.cp + q * 4);
    cx_st4<ST>(p.y, (size_t)pix * p.y_pitch + p.y_coff + q * 4, acc);
}

// ---- the fused block -------------------------------------------------------------------------------------------------------------------------
constexpr int CX_T = 16;                                   // output tile (pixels per side)
constexpr int CX_NW = 4;
constexpr int CX_RX = CX_T + 6, CX_XPIX = CX_RX * CX_RX;   // staged region of v
constexpr int CX_PB = 128;                                 // bytes of one pixel of v and of t in LDS: 64 channels
constexpr int CX_ITEMS = CX_XPIX * 8;                      // 16-byte pieces of the staged v
constexpr int CX_NINST = (CX_ITEMS + 63) / 64;             // DMA instructions (the last one's pieces beyond CX_ITEMS: zeros behind the region)
constexpr int CX_MAXHP = 8;                                // hidden channels in steps of 32: cmid <= 256
constexpr int CX_OFF_V = 0;
constexpr int CX_OFF_T = CX_OFF_V + CX_NINST * 1024;
constexpr int CX_OFF_W1 = CX_OFF_T + CX_T * CX_T * CX_PB;
constexpr int CX_OFF_W2 = CX_OFF_W1 + CX_MAXHP * 4096;
constexpr int CX_OFF_B1 = CX_OFF_W2 + CX_MAXHP * 4096;
constexpr int CX_OFF_B2 = CX_OFF_B1 + CX_MAXHP * 32 * 4;
constexpr int CX_LDS = CX_OFF_B2 + CX_CMAX * 4;
static_assert(CX_LDS <= LDS_LIMIT && CX_OFF_T % 16 == 0 && CX_OFF_W1 % 16 == 0 && CX_OFF_B1 % 16 == 0 && CX_OFF_B2 % 16 == 0, "LDS plan");

struct CxK {
    const char* x;            // NHWC 16-bit v
    const float* wdw;         // esr_pack_dw7_f32 blob
    const char* w1;           // esr_pack_cx_pw1_s16 blob
    const char* w2;           // esr_pack_cx_pw2_s16 blob
    char* y;                  // NHWC 16-bit result
    int N, H, W;
    int in_pitch, in_coff, y_pitch, y_coff;
    int c, cp;                // channels, round_up(c, 8): the 16-byte pieces staged per pixel
    int nhp;                  // ceil(cmid / 32)
    int cout_store;           // channels stored (c .. cout_store - 1 as zeros), a multiple of 8
    float slope;
    int tiles_x, tiles_y, ntiles;
};

template <bool BF16>
__global__ __launch_bounds__(64 * CX_NW, 1) void cx_block_kernel(const CxK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    const int pr = tid & 31, rs = tid >> 5;                // dw7: channel pair, row slab (tile rows 2 rs and 2 rs + 1)

    // the two 1x1 weight images and their biases into LDS, the pair's 49 x 2 depthwise weights into registers: once per block
    for (int i = tid; i < p.nhp * 256; i += 64 * CX_NW) {
        *reinterpret_cast<i32x4*>(smem + CX_OFF_W1 + i * 16) = *reinterpret_cast<const i32x4*>(p.w1 + (size_t)i * 16);
        *reinterpret_cast<i32x4*>(smem + CX_OFF_W2 + i * 16) = *reinterpret_cast<const i32x4*>(p.w2 + (size_t)i * 16);
    }
    for (int i = tid; i < p.nhp * 32; i += 64 * CX_NW)
        *reinterpret_cast<float*>(smem + CX_OFF_B1 + i * 4) = *reinterpret_cast<const float*>(p.w1 + (size_t)p.nhp * 4096 + i * 4);
    if (tid < CX_CMAX) *reinterpret_cast<float*>(smem + CX_OFF_B2 + tid * 4) = *reinterpret_cast<const float*>(p.w2 + (size_t)p.nhp * 4096 + tid * 4);
    f32x2 wd[DW7_TAPS], bd = {0.f, 0.f};
    const bool have = 2 * pr < p.cp;                       // (a pair behind the blob's channels: zero weights on zero input)
    static_for<DW7_TAPS>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        wd[t] = have ? *reinterpret_cast<const f32x2*>(p.wdw + t * p.cp + 2 * pr) : f32x2{0.f, 0.f};
    });
    if (have) bd = *reinterpret_cast<const f32x2*>(p.wdw + DW7_TAPS * p.cp + 2 * pr);
    const float slope = p.slope;
    const int npieces = p.cp >> 3;
    const size_t in_img = (size_t)p.H * p.W * p.in_pitch * 2;

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * CX_T, x0 = (rem % p.tiles_x) * CX_T;

        __syncthreads();          // the previous tile's reads of v and t are over (first tile: the weight images are in LDS)

        // ---- v with a three-pixel halo: piece (pixel, j) -> LDS byte pixel * 128 + j * 16 ----------------------------------------------------------
        const i32x4 rsrc = make_rsrc(p.x + (size_t)n * in_img, in_img);
        for (int i = wv; i < CX_NINST; i += CX_NW) {
            const int item = i * 64 + lane;
            const int pix = item >> 3, j = item & 7;
            const int gy = y0 - 3 + pix / CX_RX, gx = x0 - 3 + pix % CX_RX;
            const bool ok = item < CX_ITEMS && j < npieces && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + j * 8) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(CX_OFF_V + i * 1024), voff, rsrc, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        // ---- t = rnd(dw7(v) + b0) on the tile: a channel pair and two rows per thread, the seven taps of a row slid over 22 staged pixels -----------
#pragma unroll 1
        for (int rr = 0; rr < 2; ++rr) {
            const int r = rs * 2 + rr;
            f32x2 acc[CX_T];
#pragma unroll
            for (int x = 0; x < CX_T; ++x) acc[x] = f32x2{0.f, 0.f};
            static_for<7>([&](auto ky_) {
                constexpr int ky = decltype(ky_)::value;
                const char* row = smem + CX_OFF_V + (r + ky) * CX_RX * CX_PB + pr * 4;
                f32x2 in[CX_RX];
#pragma unroll
                for (int x = 0; x < CX_RX; ++x) {
                    float a, b;
                    unpack2<BF16>(*reinterpret_cast<const unsigned*>(row + x * CX_PB), a, b);
                    in[x] = f32x2{a, b};
                }
#pragma unroll
                for (int x = 0; x < CX_T; ++x) {
                    static_for<7>([&](auto kx_) {
                        constexpr int kx = decltype(kx_)::value;
                        acc[x].x = fmaf(in[x + kx].x, wd[ky * 7 + kx].x, acc[x].x);
                        acc[x].y = fmaf(in[x + kx].y, wd[ky * 7 + kx].y, acc[x].y);
                    });
                }
            });
#pragma unroll
            for (int x = 0; x < CX_T; ++x)
                *reinterpret_cast<unsigned*>(smem + CX_OFF_T + (r * CX_T + x) * CX_PB + pr * 4) = pack2<BF16>(acc[x].x + bd.x, acc[x].y + bd.y);
        }
        __syncthreads();

        // ---- the two 1x1s: a wave owns four tile rows (16 pixels each); the hidden channels in steps of 32 -----------------------------------------
        i32x4 bt[4][2];
        f32x4 acc2[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                bt[i][ks] = *reinterpret_cast<const i32x4*>(smem + CX_OFF_T + ((wv * 4 + i) * CX_T + px) * CX_PB + ks * 64 + kq * 16);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc2[i][mt] = *reinterpret_cast<const f32x4*>(smem + CX_OFF_B2 + (mt * 16 + kq * 4) * 4);
        }
#pragma unroll 1
        for (int hp = 0; hp < p.nhp; ++hp) {
            i32x4 a1[2][2], a2[4];
            f32x4 b1[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) a1[m][ks] = *reinterpret_cast<const i32x4*>(smem + CX_OFF_W1 + ((hp * 2 + m) * 2 + ks) * 1024 + lane * 16);
                b1[m] = *reinterpret_cast<const f32x4*>(smem + CX_OFF_B1 + ((hp * 2 + m) * 16 + kq * 4) * 4);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a2[mt] = *reinterpret_cast<const i32x4*>(smem + CX_OFF_W2 + (hp * 4 + mt) * 1024 + lane * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 h[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    h[m] = mfma32<BF16>(a1[m][0], bt[i][0], b1[m]);
                    h[m] = mfma32<BF16>(a1[m][1], bt[i][1], h[m]);
                }
                // activated, rounded, packed: lane (pixel, kq) now holds W2's K indices 8 kq .. 8 kq + 7 of this step (esr_pack_cx_pw2_s16)
                i32x4 bh;
                bh.x = (int)pack2<BF16>(act1(h[0].x, slope), act1(h[0].y, slope));
                bh.y = (int)pack2<BF16>(act1(h[0].z, slope), act1(h[0].w, slope));
                bh.z = (int)pack2<BF16>(act1(h[1].x, slope), act1(h[1].y, slope));
                bh.w = (int)pack2<BF16>(act1(h[1].z, slope), act1(h[1].w, slope));
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc2[i][mt] = mfma32<BF16>(a2[mt], bh, acc2[i][mt]);
            }
        }
        // ---- + v (the staged tile's centre) in fp32, one rounding, store ----------------------------------------------------------------------------
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wv * 4 + i;
            const int gy = y0 + row, gx = x0 + px;
            const bool inside = gy < p.H && gx < p.W;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int cb = mt * 16 + kq * 4;
                f32x4 o = acc2[i][mt] + unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + CX_OFF_V + ((row + 3) * CX_RX + px + 3) * CX_PB + cb * 2));
                o.x = cb + 0 < p.c ? o.x : 0.f; o.y = cb + 1 < p.c ? o.y : 0.f;
                o.z = cb + 2 < p.c ? o.z : 0.f; o.w = cb + 3 < p.c ? o.w : 0.f;
                uint2 pk;
                pk.x = pack2<BF16>(o.x, o.y);
                pk.y = pack2<BF16>(o.z, o.w);
                if (inside && cb < p.cout_store)
                    *reinterpret_cast<uint2*>(p.y + (((size_t)n * p.H + gy) * p.W + gx) * p.y_pitch * 2 + (size_t)(p.y_coff + cb) * 2) = pk;
            }
        }
    }
}

template <bool BF16>
int launch_cx(const CxK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&cx_block_kernel<BF16>), CX_LDS, "cx_block_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (LDS), persistent over the tiles
    esr_note_kernel("cx_block_kernel<%s>", esr_tf(BF16));
    hipLaunchKernelGGL((cx_block_kernel<BF16>), dim3(grid), dim3(64 * CX_NW), CX_LDS, st, k);
    return esr_check_launch("cx_block_kernel launch");
}

inline int cx_nhp(int cmid) { return (cmid + 31) / 32; }

}  // namespace

extern "C" {

size_t esr_packed_dw7_bytes(int c) { return c <= 0 ? 0 : (size_t)(DW7_TAPS + 1) * esr_round_up(c, 8) * sizeof(float); }

int esr_pack_dw7_f32(const float* w, const float* bias, int c, void* out, size_t out_bytes)
{
    if (!w || !out || c <= 0 || out_bytes < esr_packed_dw7_bytes(c)) return ESR_ERR_BAD_ARG;
    const int cp = esr_round_up(c, 8);
    float* o = static_cast<float*>(out);
    memset(o, 0, esr_packed_dw7_bytes(c));
    for (int ch = 0; ch < c; ++ch) {
        for (int t = 0; t < DW7_TAPS; ++t) o[t * cp + ch] = w[ch * DW7_TAPS + t];
        if (bias) o[DW7_TAPS * cp + ch] = bias[ch];
    }
    return ESR_OK;
}

int esr_dwconv7x7_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (d->ksize != 7 || d->cin != d->cout || d->cin <= 0 || d->cin > CX_CMAX) return 0;
    if (d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC || d->act != ESR_ACT_NONE || d->res_mode != ESR_RES_NONE) return 0;
    if (d->storage != ESR_STORE_F32 && d->storage != ESR_STORE_BF16 && d->storage != ESR_STORE_F16) return 0;
    // nothing rides in this launch: a descriptor that asks for a tail, a post chain, a split store, hi + lo pairs, a border table, blocked or
    // segmented tensors or Winograd weights is refused, not run without them
    if (d->tail_wpacked || d->post_wpacked || d->post2_wpacked || d->split || d->out1.ptr || d->hilo || d->border_bias || d->blocked8 ||
        d->in_seg_stride || d->wino_wpacked)
        return 0;
    if ((double)d->n * d->h * d->w * (CX_CMAX / 4) >= (double)ESR_INDEX_LIMIT * 256.0) return 0;      // blocks of 256 threads in a 32-bit grid
    return 1;
}

int esr_dwconv7x7(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_dwconv7x7_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int gran = d->storage == ESR_STORE_F32 ? 4 : 8;
    const int ck = esr_round_up(d->cin, gran);             // channels the kernel touches: whole 16-byte lanes
    if (!esr_view_fits(d->in, gran, ck) || !esr_view_fits(d->out0, gran, ck)) return ESR_ERR_BAD_ARG;
    if (d->out0.ptr == d->in.ptr) return ESR_ERR_BAD_ARG;                      // neighbouring pixels read what this one would overwrite
    Dw7K k;
    k.x = d->in.ptr; k.wp = static_cast<const float*>(d->wpacked); k.y = d->out0.ptr;
    k.N = d->n; k.H = d->h; k.W = d->w; k.cp = esr_round_up(d->cin, 8); k.nq = ck / 4;
    k.x_pitch = d->in.pitch; k.x_coff = d->in.coff; k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    const long long nthreads = (long long)d->n * d->h * d->w * k.nq;
    const dim3 grid((unsigned)((nthreads + 255) / 256));
    const size_t lds = (size_t)(DW7_TAPS + 1) * k.cp * sizeof(float);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    switch (d->storage) {
        case ESR_STORE_F32: esr_note_kernel("dwconv7x7_kernel<0>"); hipLaunchKernelGGL(dwconv7x7_kernel<ESR_STORE_F32>, grid, dim3(256), lds, st, k); break;
        case ESR_STORE_BF16: esr_note_kernel("dwconv7x7_kernel<1>"); hipLaunchKernelGGL(dwconv7x7_kernel<ESR_STORE_BF16>, grid, dim3(256), lds, st, k); break;
        default: esr_note_kernel("dwconv7x7_kernel<2>"); hipLaunchKernelGGL(dwconv7x7_kernel<ESR_STORE_F16>, grid, dim3(256), lds, st, k); break;
    }
    return esr_check_launch("dwconv7x7_kernel launch");
}

// W1 [cmid][cin]: fragment (mt, ks) at byte (mt * 2 + ks) * 1024, lane l, element j = W1[mt * 16 + (l & 15)][ks * 32 + (l >> 4) * 8 + j]; mt < 2 nhp.
// Then the fp32 bias, 32 nhp floats.  Rows >= cmid and columns >= cin are zero.
size_t esr_packed_cx_pw1_bytes(int cin, int cmid)
{
    if (cin <= 0 || cin > CX_CMAX || cmid <= 0 || cmid > CX_MAXHP * 32) return 0;
    return (size_t)cx_nhp(cmid) * (4096 + 32 * sizeof(float));
}

int esr_pack_cx_pw1_s16(const float* w, const float* bias, int cin, int cmid, int compute, void* out, size_t out_bytes)
{
    const size_t need = esr_packed_cx_pw1_bytes(cin, cmid);
    if (!w || !out || !need || out_bytes < need || !esr_is_s16(compute)) return ESR_ERR_BAD_ARG;
    const int nhp = cx_nhp(cmid);
    memset(out, 0, need);
    uint16_t* img = static_cast<uint16_t*>(out);
    float* b = reinterpret_cast<float*>(static_cast<char*>(out) + (size_t)nhp * 4096);
    for (int mt = 0; mt < 2 * nhp; ++mt)
        for (int ks = 0; ks < 2; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int h = mt * 16 + (l & 15), c = ks * 32 + (l >> 4) * 8 + j;
                    if (h < cmid && c < cin) img[((mt * 2 + ks) * 64 + l) * 8 + j] = esr_host_to16(w[(size_t)h * cin + c], compute);
                }
    if (bias)
        for (int h = 0; h < cmid; ++h) b[h] = bias[h];
    return ESR_OK;
}

// W2 [cout][cmid]: fragment (hp, mt) at byte (hp * 4 + mt) * 1024, lane l, element j = W2[mt * 16 + (l & 15)][hp * 32 + (j >> 2) * 16 + (l >> 4) * 4 + (j & 3)]:
// the K order in which cx_block_kernel's first GEMM leaves the hidden channels in a lane.  Then the fp32 bias, 64 floats.
size_t esr_packed_cx_pw2_bytes(int cmid, int cout)
{
    if (cout <= 0 || cout > CX_CMAX || cmid <= 0 || cmid > CX_MAXHP * 32) return 0;
    return (size_t)cx_nhp(cmid) * 4096 + CX_CMAX * sizeof(float);
}

int esr_pack_cx_pw2_s16(const float* w, const float* bias, int cmid, int cout, int compute, void* out, size_t out_bytes)
{
    const size_t need = esr_packed_cx_pw2_bytes(cmid, cout);
    if (!w || !out || !need || out_bytes < need || !esr_is_s16(compute)) return ESR_ERR_BAD_ARG;
    const int nhp = cx_nhp(cmid);
    memset(out, 0, need);
    uint16_t* img = static_cast<uint16_t*>(out);
    float* b = reinterpret_cast<float*>(static_cast<char*>(out) + (size_t)nhp * 4096);
    for (int hp = 0; hp < nhp; ++hp)
        for (int mt = 0; mt < 4; ++mt)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int o = mt * 16 + (l & 15), h = hp * 32 + (j >> 2) * 16 + (l >> 4) * 4 + (j & 3);
                    if (o < cout && h < cmid) img[((hp * 4 + mt) * 64 + l) * 8 + j] = esr_host_to16(w[(size_t)o * cmid + h], compute);
                }
    if (bias)
        for (int o = 0; o < cout; ++o) b[o] = bias[o];
    return ESR_OK;
}

int esr_cx_block_supported(const esr_chain_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->n_layers != 3 || d->act != ESR_ACT_LRELU || d->res_mode != ESR_RES_POST_ACT) return 0;
    if (d->cin != d->cout || d->cin <= 32 || d->cin > CX_CMAX || d->cmid <= 128 || d->cmid > CX_MAXHP * 32) return 0;
    if (d->post_wpacked || d->post2_wpacked) return 0;
    if ((d->post_cout & 7) || d->post_cout < d->cout || d->post_cout > esr_round_up(d->cout, 16)) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, CX_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_cx_block_s16(const esr_chain_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->post_out.ptr || !d->wpacked[0] || !d->wpacked[1] || !d->wpacked[2]) return ESR_ERR_BAD_ARG;
    if (!esr_cx_block_supported(d)) return ESR_ERR_UNSUPPORTED;
    if (!esr_view_fits(d->in, 8, esr_round_up(d->cin, 8)) || !esr_view_fits(d->post_out, 8, d->post_cout)) return ESR_ERR_BAD_ARG;
    if (d->post_out.ptr == d->in.ptr) return ESR_ERR_BAD_ARG;                  // neighbouring tiles read the halo of v
    CxK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.wdw = static_cast<const float*>(d->wpacked[0]);
    k.w1 = static_cast<const char*>(d->wpacked[1]);
    k.w2 = static_cast<const char*>(d->wpacked[2]);
    k.y = static_cast<char*>(d->post_out.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.y_pitch = d->post_out.pitch; k.y_coff = d->post_out.coff;
    k.c = d->cin; k.cp = esr_round_up(d->cin, 8);
    k.nhp = cx_nhp(d->cmid);
    k.cout_store = d->post_cout;
    k.slope = esr_act_slope(d->act, d->slope);
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, CX_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return d->storage == ESR_STORE_BF16 ? launch_cx<true>(k, st) : launch_cx<false>(k, st);
}

}  // extern "C"
