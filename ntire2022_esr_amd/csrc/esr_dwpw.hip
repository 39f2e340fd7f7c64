// esr_dwpw.hip -- the refinement path of team 35's RFDB (models/team35_rfdn/rmsrb1.py:22-27, :199-210): `conv_four_layer(C)` and the block's
// `act(c_r(x) + x)` behind it,
//
//     u1 = rnd(dw3_a(x) + x)                       Residual(depthwise 3x3, zero padding, bias)
//     h  = rnd(relu(Wa . u1 + ba))                 1x1, C -> C
//     u2 = rnd(dw3_b(h) + h)
//     r  = rnd(lrelu(Wb . u2 + bb + x))            1x1, C -> C, the block input added before the activation
//
// rnd = one rounding to the storage type.  As four launches (esr_dwconv3x3_f32 with a pre-activation residual, esr_conv2d_f32 1x1, twice)
// a pixel moves nine tensor passes through HBM, 1008 bytes in bf16 at pitch 56; dwpw_pair_kernel<BF16> (esr_dwpw_pair_s16; 16-bit storage)
// reads x once and writes r once: 224 bytes.  An 8-wave block owns one 16 x 16 output tile at a time (persistent over the tiles) and keeps
// in LDS
//
//     x    20 x 20 pixels  [pixel][128 B]   staged with a TWO-pixel halo by LDS-DMA, 16-byte pieces; the pieces outside the image and the
//                                           pieces behind round_up(C, 8) channels are requested out of range and arrive as zeros
//     u1   18 x 18 pixels  [pixel][144 B]   the tile and a one-pixel ring; h overwrites it, one 16-pixel group at a time
//     u2   16 x 16 pixels  [pixel][144 B]
//
// (144 = 128 + 16: the 16 pixels of an MFMA operand on different banks.)  The depthwise steps run on the VALU in fp32 from the fp32
// esr_pack_dw_f32 blobs: a thread owns a channel PAIR (its 2 x 9 x 2 weights in registers for the block's lifetime) and half an image row at
// a time; bias first, the nine taps added in (ky, kx) ascending order, the centre pixel (the residual) last -- dwconv3x3_kernel's order.  The
// 1x1s run on v_mfma_f32_16x16x32, 16 pixels x 64 channels per group, their weight fragments (8 + 8) and biases in registers for the
// block's lifetime; h is rounded and written back over the group's u1.
//
// h IS ZERO AT RING POSITIONS OUTSIDE THE IMAGE: dw3_b zero-pads the stored tensor h, it does not see relu(ba) there (nor does u1 need a
// value there: only h's own pixel feeds h).
//
// Numerics: u1, h, u2 and r are each rounded exactly where the per-op form stores them.  Wa and Wb are ROUNDED ONCE to the storage type (the
// blobs are esr_pack_cx_pw1_s16's; the per-op 1x1s of conv_s16_kernel multiply by hi + lo pairs) and K is one pass over 64 channels, so the
// result is NOT bit-identical to the four launches; every stage stays within one rounding of its fp64 restatement on the effective weights.
// Pad channels: weight rows / columns and biases beyond C are zero in the blobs; channels C .. post_cout - 1 of the output are stored as
// zeros.  LDS 133 KB, one block per CU; eight waves, two per SIMD: the phases of a tile are serial (staging, dw, GEMM, dw, GEMM and store), and
// a second wave per SIMD hides the LDS and MFMA latencies inside each (4 waves: 0.384 ms per launch at 32 x 256 x 256, 8 waves: 0.270 ms).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int DP_T = 16;                                   // output tile (pixels per side)
constexpr int DP_NW = 8;
constexpr int DP_CMAX = 64;
constexpr int DP_RX = DP_T + 4, DP_XPIX = DP_RX * DP_RX;   // staged region of x
constexpr int DP_RU = DP_T + 2, DP_UPIX = DP_RU * DP_RU;   // u1 / h: the tile and its ring
constexpr int DP_UGRP = (DP_UPIX + 15) / 16;               // 16-pixel MFMA groups of the ring region (the last one partly behind it)
constexpr int DP_PB = 128;                                 // bytes of one staged pixel of x: 64 channels
constexpr int DP_SB = 144;                                 // bytes of one pixel of u1 / h and of u2
constexpr int DP_ITEMS = DP_XPIX * 8;                      // 16-byte pieces of the staged x
constexpr int DP_NINST = (DP_ITEMS + 63) / 64;             // DMA instructions
constexpr int DP_OFF_X = 0;
constexpr int DP_OFF_U = DP_OFF_X + DP_NINST * 1024;
constexpr int DP_OFF_V = DP_OFF_U + DP_UGRP * 16 * DP_SB;
constexpr int DP_LDS = DP_OFF_V + DP_T * DP_T * DP_SB;
static_assert(DP_LDS <= LDS_LIMIT && DP_OFF_U % 16 == 0 && DP_OFF_V % 16 == 0 && DP_SB % 16 == 0 && DP_NINST * 64 == DP_ITEMS, "LDS plan");

struct DpK {
    const char* x;            // NHWC 16-bit block input
    const float* dwa;         // esr_pack_dw_f32 blobs: [tap][cq] + bias[cq], cq = round_up(c, 4)
    const float* dwb;
    const char* wa;           // esr_pack_cx_pw1_s16 blobs (cin = cmid = c): 8 fragments of 1 KB, then 64 fp32 biases
    const char* wb;
    char* y;                  // NHWC 16-bit result
    int N, H, W;
    int in_pitch, in_coff, y_pitch, y_coff;
    int c, cp, cq;            // channels, round_up(c, 8): the 16-byte pieces staged per pixel, round_up(c, 4): the depthwise blobs' pitch
    int cout_store;           // channels stored (c .. cout_store - 1 as zeros), a multiple of 8
    float slope;
    int tiles_x, tiles_y, ntiles;
};

// One depthwise row piece: WOUT pixels of row r from column c0 of the destination, dst(r, c0 + x) = rnd(bias + sum_taps src(r + ky, c0 + x + kx) w
// + src(r + 1, c0 + x + 1)) for the thread's channel pair; src is two pixels wider and higher than dst.
template <bool BF16, int WOUT, int SRC_W, int SRC_PB, int DST_W>
__device__ __forceinline__ void dp_dw_piece(const char* src, char* dst, int r, int c0, const f32x2 (&w)[9], f32x2 b)
{
    f32x2 acc[WOUT], ctr[WOUT];
#pragma unroll
    for (int x = 0; x < WOUT; ++x) acc[x] = b;
    static_for<3>([&](auto ky_) {
        constexpr int ky = decltype(ky_)::value;
        const char* row = src + ((r + ky) * SRC_W + c0) * SRC_PB;
        f32x2 in[WOUT + 2];
#pragma unroll
        for (int x = 0; x < WOUT + 2; ++x) {
            float a, c;
            unpack2<BF16>(*reinterpret_cast<const unsigned*>(row + x * SRC_PB), a, c);
            in[x] = f32x2{a, c};
        }
#pragma unroll
        for (int x = 0; x < WOUT; ++x) {
            static_for<3>([&](auto kx_) {
                constexpr int kx = decltype(kx_)::value;
                acc[x].x = fmaf(in[x + kx].x, w[ky * 3 + kx].x, acc[x].x);
                acc[x].y = fmaf(in[x + kx].y, w[ky * 3 + kx].y, acc[x].y);
            });
            if (ky == 1) ctr[x] = in[x + 1];
        }
    });
#pragma unroll
    for (int x = 0; x < WOUT; ++x)
        *reinterpret_cast<unsigned*>(dst + (r * DST_W + c0 + x) * DP_SB) = pack2<BF16>(acc[x].x + ctr[x].x, acc[x].y + ctr[x].y);
}

template <bool BF16>
__global__ __launch_bounds__(64 * DP_NW, 1) void dwpw_pair_kernel(const DpK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    const int pr = tid & 31, rs = tid >> 5;                // depthwise: channel pair, piece slab

    // both 1x1 weight images and their biases, and the pair's 2 x 9 x 2 depthwise weights, into registers: once per block
    i32x4 wa[4][2], wb[4][2];
    f32x4 ba[4], bb[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            wa[mt][ks] = *reinterpret_cast<const i32x4*>(p.wa + ((mt * 2 + ks) * 64 + lane) * 16);
            wb[mt][ks] = *reinterpret_cast<const i32x4*>(p.wb + ((mt * 2 + ks) * 64 + lane) * 16);
        }
        ba[mt] = *reinterpret_cast<const f32x4*>(p.wa + 8192 + (mt * 16 + kq * 4) * 4);
        bb[mt] = *reinterpret_cast<const f32x4*>(p.wb + 8192 + (mt * 16 + kq * 4) * 4);
    }
    f32x2 da[9], db[9], bda = {0.f, 0.f}, bdb = {0.f, 0.f};
    const bool have = 2 * pr < p.cq;                       // (a pair behind the blobs' channels: zero weights on zero input)
    static_for<9>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        da[t] = have ? *reinterpret_cast<const f32x2*>(p.dwa + t * p.cq + 2 * pr) : f32x2{0.f, 0.f};
        db[t] = have ? *reinterpret_cast<const f32x2*>(p.dwb + t * p.cq + 2 * pr) : f32x2{0.f, 0.f};
    });
    if (have) {
        bda = *reinterpret_cast<const f32x2*>(p.dwa + 9 * p.cq + 2 * pr);
        bdb = *reinterpret_cast<const f32x2*>(p.dwb + 9 * p.cq + 2 * pr);
    }
    const float slope = p.slope;
    const int npieces = p.cp >> 3;
    const size_t in_img = (size_t)p.H * p.W * p.in_pitch * 2;

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * DP_T, x0 = (rem % p.tiles_x) * DP_T;

        __syncthreads();          // the previous tile's reads of x and u2 are over

        // ---- x with a two-pixel halo: piece (pixel, j) -> LDS byte pixel * 128 + j * 16 ------------------------------------------------------------
        const i32x4 rsrc = make_rsrc(p.x + (size_t)n * in_img, in_img);
        for (int i = wv; i < DP_NINST; i += DP_NW) {
            const int item = i * 64 + lane;
            const int pix = item >> 3, j = item & 7;
            const int gy = y0 - 2 + pix / DP_RX, gx = x0 - 2 + pix % DP_RX;
            const bool ok = j < npieces && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + j * 8) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(DP_OFF_X + i * 1024), voff, rsrc, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        // ---- u1 = rnd(dw3_a(x) + x) on the 18 x 18 ring region: 36 half rows of 9 pixels over the 16 slabs ------------------------------------------
#pragma unroll 1
        for (int it = rs; it < 2 * DP_RU; it += 2 * DP_NW)
            dp_dw_piece<BF16, 9, DP_RX, DP_PB, DP_RU>(smem + DP_OFF_X + pr * 4, smem + DP_OFF_U + pr * 4, it >> 1, (it & 1) * 9, da, bda);
        __syncthreads();

        // ---- h = rnd(relu(Wa . u1 + ba)) over u1, group by group; zero outside the image --------------------------------------------------------------
#pragma unroll 1
        for (int g = wv; g < DP_UGRP; g += DP_NW) {
            const int pi = g * 16 + px;
            char* pu = smem + DP_OFF_U + pi * DP_SB;
            const i32x4 b0 = *reinterpret_cast<const i32x4*>(pu + kq * 16);
            const i32x4 b1 = *reinterpret_cast<const i32x4*>(pu + 64 + kq * 16);
            const int ry = pi / DP_RU, rx = pi - ry * DP_RU;
            const int gy = y0 - 1 + ry, gx = x0 - 1 + rx;
            const bool inside = pi < DP_UPIX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            uint2 hq[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 a = mfma32<BF16>(wa[mt][0], b0, ba[mt]);
                a = mfma32<BF16>(wa[mt][1], b1, a);
                hq[mt].x = inside ? pack2<BF16>(act1(a.x, 0.f), act1(a.y, 0.f)) : 0u;
                hq[mt].y = inside ? pack2<BF16>(act1(a.z, 0.f), act1(a.w, 0.f)) : 0u;
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<uint2*>(pu + (mt * 16 + kq * 4) * 2) = hq[mt];
        }
        __syncthreads();

        // ---- u2 = rnd(dw3_b(h) + h) on the tile: 32 half rows of 8 pixels over the 16 slabs -------------------------------------------------------------
#pragma unroll 1
        for (int it = rs; it < 2 * DP_T; it += 2 * DP_NW)
            dp_dw_piece<BF16, 8, DP_RU, DP_SB, DP_T>(smem + DP_OFF_U + pr * 4, smem + DP_OFF_V + pr * 4, it >> 1, (it & 1) * 8, db, bdb);
        __syncthreads();

        // ---- r = rnd(lrelu(Wb . u2 + bb + x)): a wave owns two tile rows; x from the staged tile's centre in fp32 ------------------------------------
#pragma unroll
        for (int i = 0; i < DP_T / DP_NW; ++i) {
            const int row = wv * (DP_T / DP_NW) + i;
            const char* pv = smem + DP_OFF_V + (row * DP_T + px) * DP_SB;
            const i32x4 b0 = *reinterpret_cast<const i32x4*>(pv + kq * 16);
            const i32x4 b1 = *reinterpret_cast<const i32x4*>(pv + 64 + kq * 16);
            const int gy = y0 + row, gx = x0 + px;
            const bool inside = gy < p.H && gx < p.W;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int cb = mt * 16 + kq * 4;
                f32x4 o = mfma32<BF16>(wb[mt][0], b0, bb[mt]);
                o = mfma32<BF16>(wb[mt][1], b1, o);
                o += unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + DP_OFF_X + ((row + 2) * DP_RX + px + 2) * DP_PB + cb * 2));
                o.x = cb + 0 < p.c ? act1(o.x, slope) : 0.f; o.y = cb + 1 < p.c ? act1(o.y, slope) : 0.f;
                o.z = cb + 2 < p.c ? act1(o.z, slope) : 0.f; o.w = cb + 3 < p.c ? act1(o.w, slope) : 0.f;
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
int launch_dwpw(const DpK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&dwpw_pair_kernel<BF16>), DP_LDS, "dwpw_pair_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (LDS), persistent over the tiles
    esr_note_kernel("dwpw_pair_kernel<%s>", esr_tf(BF16));
    hipLaunchKernelGGL((dwpw_pair_kernel<BF16>), dim3(grid), dim3(64 * DP_NW), DP_LDS, st, k);
    return esr_check_launch("dwpw_pair_kernel launch");
}

}  // namespace

extern "C" {

int esr_dwpw_pair_supported(const esr_chain_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->n_layers != 4 || d->act != ESR_ACT_LRELU || d->res_mode != ESR_RES_PRE_ACT) return 0;
    if (d->cin != d->cout || d->cmid != d->cin || d->cin <= 32 || d->cin > DP_CMAX) return 0;
    if (d->post_wpacked || d->post2_wpacked) return 0;
    if ((d->post_cout & 7) || d->post_cout < d->cout || d->post_cout > esr_round_up(d->cout, 16)) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, DP_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_dwpw_pair_s16(const esr_chain_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->post_out.ptr || !d->wpacked[0] || !d->wpacked[1] || !d->wpacked[2] || !d->wpacked[3]) return ESR_ERR_BAD_ARG;
    if (!esr_dwpw_pair_supported(d)) return ESR_ERR_UNSUPPORTED;
    if (!esr_view_fits(d->in, 8, esr_round_up(d->cin, 8)) || !esr_view_fits(d->post_out, 8, d->post_cout)) return ESR_ERR_BAD_ARG;
    if (d->post_out.ptr == d->in.ptr) return ESR_ERR_BAD_ARG;                  // neighbouring tiles read the halo of x
    DpK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.dwa = static_cast<const float*>(d->wpacked[0]);
    k.wa = static_cast<const char*>(d->wpacked[1]);
    k.dwb = static_cast<const float*>(d->wpacked[2]);
    k.wb = static_cast<const char*>(d->wpacked[3]);
    k.y = static_cast<char*>(d->post_out.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.y_pitch = d->post_out.pitch; k.y_coff = d->post_out.coff;
    k.c = d->cin; k.cp = esr_round_up(d->cin, 8); k.cq = esr_round_up(d->cin, 4);
    k.cout_store = d->post_cout;
    k.slope = esr_act_slope(d->act, d->slope);
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, DP_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return d->storage == ESR_STORE_BF16 ? launch_dwpw<true>(k, st) : launch_dwpw<false>(k, st);
}

}  // extern "C"
