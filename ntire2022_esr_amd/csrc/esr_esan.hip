// esr_esan.hip -- the head of ESAN's residual block (team34_esan.py:71-76, :49) as ONE launch (esr_resblock_head_s16; 16-bit storage, 32 channels).
//
//     x  = rnd(xin + g)                          the previous block's `identity + ESA(..)` (G; the first block has x = xin and stores no x)
//     t  = rnd(relu(W1 (*) x + b1))              3x3, 32 -> 32, never stored
//     u  = rnd(W2 (*) t~ + b2)                   3x3, 32 -> 32, stored (out1)
//     c1 = rnd(Wc . u + bc)                      ESA.conv1, 1x1 on u AS STORED, 32 -> f <= 16, stored into the pitch-16 ESA map (post_out)
//
// rnd = one rounding to the storage type, the one the separate launches do when they store.  t~ is t as rounded and 0 OUTSIDE THE IMAGE: the
// reference zero-pads t, so a halo pixel outside the image is 0, not relu(b1).  As four launches (identity 1x1 + residual, two 3x3s, the 1x1) a
// pixel moves 464 bytes through HBM; here xin and g are read once and x, u, c1 written once: 288 bytes, and t never exists.
//
// A 4-wave block owns one 16 x 16 output tile at a time (persistent over the tiles) and keeps in LDS
//
//     xin, g   20 x 20 pixels  [chunk][pixel][32 B]   staged with a TWO-pixel halo by LDS-DMA (conv_s16_kernel's stage layout: a B fragment is 16 B
//                                                     of one pixel); pieces outside the image are requested out of range and arrive as zeros.  The
//                                                     sum is rounded into the xin tile in place; its centre goes to out0
//     t        18 x 18 pixels  [chunk][pixel][32 B]   the first 3x3 on the tile and a one-pixel ring (324 instead of 256 pixels), rounded, 0 outside
//                                                     the image
//     u        16 x 16 pixels  [chunk][pixel][32 B]   as stored: the 1x1's B operand
//
// The images of both 3x3s -- 2 chunks x 5 tap pairs x 2 output tiles = 20 A fragments each -- and of the 1x1 (2) live in REGISTERS for the
// block's lifetime (168 VGPRs of the 512 a lone wave per SIMD has).  Per accumulator: bias as the first MFMA's C, chunks in order, tap pairs in
// order -- conv_s16_kernel's order; the 1x1 multiplies the chunk's 16 channels by the [hi | lo] weight halves of esr_pack_conv_s16's ksize 1
// image, as distill_step_kernel does.
// 32 channels are two whole K chunks and one whole 64-byte run per pixel: nothing is padded and nothing beyond the 32 channels is read.
// LDS: 25 KB xin + 25 KB g + 21 KB t + 16 KB u = 87 KB; one block per CU (registers).  Staging and MFMAs of consecutive tiles are not overlapped.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int RH_T = 16;                                   // output tile (pixels per side)
constexpr int RH_NW = 4;
constexpr int RH_C = 32;                                   // channels of xin, g, x, t, u
constexpr int RH_NCH = RH_C / 16;                          // K chunks = output tiles of both 3x3s
constexpr int RH_RX = RH_T + 4, RH_XPIX = RH_RX * RH_RX;   // staged region of xin / g / x
constexpr int RH_RT = RH_T + 2, RH_TPIX = RH_RT * RH_RT;   // region of t
constexpr int RH_GT = (RH_TPIX + 15) / 16;                 // groups of 16 pixels of t (the last one is partial)
constexpr int RH_PAIRS = 5;
constexpr int RH_XCH = RH_XPIX * 32;                       // bytes of one 16-channel chunk of the staged tiles
constexpr int RH_TCH = RH_GT * 16 * 32;                    // ... of t (whole groups: the partial group's pad pixels are stored, as zeros)
constexpr int RH_UCH = RH_T * RH_T * 32;                   // ... of u
constexpr int RH_ITEMS = RH_NCH * RH_XPIX * 2;             // 16-byte pieces of one staged tile
constexpr int RH_NINST = RH_ITEMS / 64;                    // DMA instructions per staged tile
constexpr int RH_OFF_X = 0;
constexpr int RH_OFF_G = RH_OFF_X + RH_NCH * RH_XCH;
constexpr int RH_OFF_T = RH_OFF_G + RH_NCH * RH_XCH;
constexpr int RH_OFF_U = RH_OFF_T + RH_NCH * RH_TCH;
constexpr int RH_LDS = RH_OFF_U + RH_NCH * RH_UCH;
static_assert(RH_ITEMS % 64 == 0, "a staged tile is whole DMA instructions");
static_assert(RH_LDS <= LDS_LIMIT && RH_OFF_G % 1024 == 0 && RH_OFF_T % 16 == 0 && RH_OFF_U % 16 == 0, "LDS plan");

struct ResHeadK {
    const char* xin;          // NHWC 16-bit block input (32 channels from in_coff)
    const char* g;            // NHWC 16-bit, added to xin (G kernels)
    const char* w1;           // esr_pack_conv_s16 blob of the first 3x3
    const char* w2;           // ... of the second
    const char* wc;           // esr_pack_conv_s16 blob (ksize 1: hi + lo) of the 1x1
    char* x;                  // NHWC 16-bit xin + g (G kernels)
    char* u;                  // NHWC 16-bit
    char* c1;                 // NHWC 16-bit ESA map
    int N, H, W;
    int in_pitch, in_coff, g_pitch, g_coff, x_pitch, x_coff, u_pitch, u_coff, c1_pitch, c1_coff;
    int c1_cout8;             // channels of c1 stored
    int tiles_x, tiles_y, ntiles;
};

__device__ __forceinline__ f32x4 rh_relu(f32x4 v)
{
    v.x = act1(v.x, 0.f); v.y = act1(v.y, 0.f); v.z = act1(v.z, 0.f); v.w = act1(v.w, 0.f);
    return v;
}

// one 16-byte piece of xin + one of g -> the rounded sum
template <bool BF16>
__device__ __forceinline__ i32x4 rh_add8(i32x4 a, i32x4 b)
{
    const f32x4 a0 = unpack4<BF16>(uint2{(unsigned)a.x, (unsigned)a.y}), a1 = unpack4<BF16>(uint2{(unsigned)a.z, (unsigned)a.w});
    const f32x4 b0 = unpack4<BF16>(uint2{(unsigned)b.x, (unsigned)b.y}), b1 = unpack4<BF16>(uint2{(unsigned)b.z, (unsigned)b.w});
    i32x4 r;
    r.x = (int)pack2<BF16>(a0.x + b0.x, a0.y + b0.y);
    r.y = (int)pack2<BF16>(a0.z + b0.z, a0.w + b0.w);
    r.z = (int)pack2<BF16>(a1.x + b1.x, a1.y + b1.y);
    r.w = (int)pack2<BF16>(a1.z + b1.z, a1.w + b1.w);
    return r;
}

// G: x = xin + g, stored to p.x (blocks 2..16 of the trunk); !G: x = xin (the first block)
template <bool BF16, bool G>
__global__ __launch_bounds__(64 * RH_NW, 1) void resblock_head_kernel(const ResHeadK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    constexpr int W3B = RH_NCH * RH_PAIRS * RH_NCH * 1024, WCB = RH_NCH * 1024;       // weight image bytes: a 3x3, the 1x1 (one output tile)

    // all three weight images into registers: once per block
    i32x4 a1[RH_NCH][RH_PAIRS][RH_NCH], a2[RH_NCH][RH_PAIRS][RH_NCH], ac[RH_NCH];
    static_for<RH_NCH>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        static_for<RH_PAIRS>([&](auto q_) {
            constexpr int q = decltype(q_)::value;
            static_for<RH_NCH>([&](auto t_) {
                constexpr int t = decltype(t_)::value;
                a1[c][q][t] = *reinterpret_cast<const i32x4*>(p.w1 + ((c * RH_PAIRS + q) * RH_NCH + t) * 1024 + lane * 16);
                a2[c][q][t] = *reinterpret_cast<const i32x4*>(p.w2 + ((c * RH_PAIRS + q) * RH_NCH + t) * 1024 + lane * 16);
            });
        });
        ac[c] = *reinterpret_cast<const i32x4*>(p.wc + c * 1024 + lane * 16);
    });
    f32x4 bia1[RH_NCH], bia2[RH_NCH];
    static_for<RH_NCH>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bia1[t] = *reinterpret_cast<const f32x4*>(p.w1 + W3B + (t * 16 + kq * 4) * 4);
        bia2[t] = *reinterpret_cast<const f32x4*>(p.w2 + W3B + (t * 16 + kq * 4) * 4);
    });
    const f32x4 biac = *reinterpret_cast<const f32x4*>(p.wc + WCB + kq * 4 * 4);
    // pair q: tap min(2 q + (kq >> 1), 8), channel half kq & 1 (conv_s16_kernel's map); in the x tile (rows of 20) and in the t tile (rows of 18)
    int tapx[RH_PAIRS], tapt[RH_PAIRS];
    static_for<RH_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        const int tap = min(2 * q + (kq >> 1), 8);
        tapx[q] = ((tap / 3) * RH_RX + tap % 3) * 32 + (kq & 1) * 16;
        tapt[q] = ((tap / 3) * RH_RT + px + tap % 3) * 32 + (kq & 1) * 16;
    });

    const size_t in_img = (size_t)p.H * p.W * p.in_pitch * 2, g_img = (size_t)p.H * p.W * p.g_pitch * 2;

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * RH_T, x0 = (rem % p.tiles_x) * RH_T;

        // ---- xin (and g) with a two-pixel halo: piece (chunk c, pixel, half h) -> LDS byte c * RH_XCH + pixel * 32 + h * 16 of its tile --------
        const i32x4 rs_x = make_rsrc(p.xin + (size_t)n * in_img, in_img);
        const i32x4 rs_g = make_rsrc(G ? p.g + (size_t)n * g_img : p.xin, G ? g_img : 0);
        for (int i = wv; i < RH_NINST; i += RH_NW) {
            const int item = i * 64 + lane;
            const int c = item / (RH_XPIX * 2), pr = item - c * (RH_XPIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 2 + pix / RH_RX, gx = x0 - 2 + pix % RH_RX;
            const int ch = c * 16 + h * 8;
            const bool ok = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            const unsigned vx = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + ch) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(RH_OFF_X + i * 1024), vx, rs_x, 0u);
            if constexpr (G) {
                const unsigned vg = ok ? (unsigned)(((gy * p.W + gx) * p.g_pitch + p.g_coff + ch) * 2) : OOB;
                dma_buf16(smem_lds + (unsigned)(RH_OFF_G + i * 1024), vg, rs_g, 0u);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (G) {
            // x = rnd(xin + g) in place (0 + 0 outside the image); the tile's centre is the block's x output
            for (int item = tid; item < RH_ITEMS; item += 64 * RH_NW) {
                const int c = item / (RH_XPIX * 2), pr = item - c * (RH_XPIX * 2);
                const int pix = pr >> 1, h = pr & 1;
                const int ry = pix / RH_RX, rx = pix - ry * RH_RX;
                const int off = c * RH_XCH + pix * 32 + h * 16;
                const i32x4 s = rh_add8<BF16>(*reinterpret_cast<const i32x4*>(smem + RH_OFF_X + off), *reinterpret_cast<const i32x4*>(smem + RH_OFF_G + off));
                *reinterpret_cast<i32x4*>(smem + RH_OFF_X + off) = s;
                const int gy = y0 - 2 + ry, gx = x0 - 2 + rx;
                if (ry >= 2 && ry < 2 + RH_T && rx >= 2 && rx < 2 + RH_T && gy < p.H && gx < p.W)
                    *reinterpret_cast<i32x4*>(p.x + (((size_t)n * p.H + gy) * p.W + gx) * p.x_pitch * 2 + (size_t)(p.x_coff + c * 16 + h * 8) * 2) = s;
            }
            __syncthreads();
        }

        // ---- t = relu(3x3(x)) on the 18 x 18 region, two groups of 16 pixels at a time; 0 outside the image ---------------------------------------
        for (int g0 = wv; g0 < RH_GT; g0 += 2 * RH_NW) {
            const int g1 = g0 + RH_NW < RH_GT ? g0 + RH_NW : g0;           // (an odd last group is computed twice)
            const int gg[2] = {g0, g1};
            int pp[2], ry[2], rx[2], bx[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                pp[j] = gg[j] * 16 + px;
                const int pc = min(pp[j], RH_TPIX - 1);                    // (the partial group's pad pixels read the last pixel's window)
                ry[j] = pc / RH_RT; rx[j] = pc - ry[j] * RH_RT;
                bx[j] = (ry[j] * RH_RX + rx[j]) * 32;                      // t pixel (ry, rx) = x pixel (ry + 1, rx + 1): its window starts at (ry, rx)
            }
            f32x4 acc[2][RH_NCH];
            static_for<RH_NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                static_for<RH_PAIRS>([&](auto q_) {
                    constexpr int q = decltype(q_)::value;
                    i32x4 b[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + RH_OFF_X + c * RH_XCH + bx[j] + tapx[q]);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        static_for<RH_NCH>([&](auto t_) {
                            constexpr int tt = decltype(t_)::value;
                            acc[j][tt] = mfma32<BF16>(a1[c][q][tt], b[j], (c == 0 && q == 0) ? bia1[tt] : acc[j][tt]);
                        });
                });
            });
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int gy = y0 - 1 + ry[j], gx = x0 - 1 + rx[j];
                const bool inside = pp[j] < RH_TPIX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                static_for<RH_NCH>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    const f32x4 v = rh_relu(acc[j][tt]);
                    uint2 pk;
                    pk.x = inside ? pack2<BF16>(v.x, v.y) : 0u;           // outside the image: the second 3x3's zero padding of t
                    pk.y = inside ? pack2<BF16>(v.z, v.w) : 0u;
                    *reinterpret_cast<uint2*>(smem + RH_OFF_T + tt * RH_TCH + pp[j] * 32 + kq * 8) = pk;
                });
            }
        }
        __syncthreads();

        // ---- u = 3x3(t) on the tile: four image rows per wave; then c1 = 1x1(u as stored) on the same rows ------------------------------------------
        {
            int bb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bb[j] = (wv * 4 + j) * RH_RT * 32;
            f32x4 acc[4][RH_NCH];
            static_for<RH_NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                static_for<RH_PAIRS>([&](auto q_) {
                    constexpr int q = decltype(q_)::value;
                    i32x4 b[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + RH_OFF_T + c * RH_TCH + bb[j] + tapt[q]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        static_for<RH_NCH>([&](auto t_) {
                            constexpr int tt = decltype(t_)::value;
                            acc[j][tt] = mfma32<BF16>(a2[c][q][tt], b[j], (c == 0 && q == 0) ? bia2[tt] : acc[j][tt]);
                        });
                });
            });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wv * 4 + j;
                const int gy = y0 + row, gx = x0 + px;
                const bool inside = gy < p.H && gx < p.W;
                char* const up = p.u + (((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0)) * p.u_pitch * 2 + (size_t)p.u_coff * 2;
                static_for<RH_NCH>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    const f32x4 v = acc[j][tt];
                    uint2 pk;
                    pk.x = pack2<BF16>(v.x, v.y);
                    pk.y = pack2<BF16>(v.z, v.w);
                    *reinterpret_cast<uint2*>(smem + RH_OFF_U + tt * RH_UCH + (row * RH_T + px) * 32 + kq * 8) = pk;
                    if (inside) *reinterpret_cast<uint2*>(up + (tt * 16 + kq * 4) * 2) = pk;
                });
            }
        }
        __syncthreads();
        {
            // K = 32: [hi | lo] weights x the chunk's 16 channels twice
            f32x4 acc[4];
            static_for<RH_NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const i32x4 b = *reinterpret_cast<const i32x4*>(smem + RH_OFF_U + c * RH_UCH + ((wv * 4 + j) * RH_T + px) * 32 + (kq & 1) * 16);
                    acc[j] = mfma32<BF16>(ac[c], b, c == 0 ? biac : acc[j]);
                }
            });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gy = y0 + wv * 4 + j, gx = x0 + px;
                if (gy < p.H && gx < p.W && kq * 4 < p.c1_cout8) {
                    uint2 pk;
                    pk.x = pack2<BF16>(acc[j].x, acc[j].y);
                    pk.y = pack2<BF16>(acc[j].z, acc[j].w);
                    *reinterpret_cast<uint2*>(p.c1 + (((size_t)n * p.H + gy) * p.W + gx) * p.c1_pitch * 2 + (size_t)(p.c1_coff + kq * 4) * 2) = pk;
                }
            }
        }
        __syncthreads();                                  // x, t and u are read: the next tile's DMA may overwrite them
    }
}

template <bool BF16, bool G>
int launch_reshead(const ResHeadK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&resblock_head_kernel<BF16, G>), RH_LDS, "resblock_head_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (registers), persistent over the tiles
    esr_note_kernel("resblock_head_kernel<%s, %s>", esr_tf(BF16), esr_tf(G));
    hipLaunchKernelGGL((resblock_head_kernel<BF16, G>), dim3(grid), dim3(64 * RH_NW), RH_LDS, st, k);
    return esr_check_launch("resblock_head_kernel launch");
}

}  // namespace

extern "C" int esr_resblock_head_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->cin != RH_C || d->cout != RH_C || d->ksize != 3 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->act != ESR_ACT_RELU) return 0;
    if (d->res_mode != ESR_RES_NONE && d->res_mode != ESR_RES_PRE_ACT) return 0;
    if (d->split > 0 && d->split < d->cout) return 0;
    if (d->post_cout <= 0 || d->post_cout > ESR_ESA_FP || d->post_act != ESR_ACT_NONE) return 0;
    if (d->post2_wpacked || d->tail_cat.ptr || d->tail_cat_c || d->border_bias || d->in_seg_stride || d->blocked8 || d->hilo || d->wino_wpacked) return 0;
    const double px = (double)d->h * d->w;
    if (!esr_image_below_1g(px, d->in.pitch, 2)) return 0;
    if (d->res_mode != ESR_RES_NONE && !esr_image_below_1g(px, d->res.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, RH_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

extern "C" int esr_resblock_head_s16(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out1.ptr || !d->post_out.ptr || !d->wpacked || !d->tail_wpacked || !d->post_wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_resblock_head_supported(d)) return ESR_ERR_UNSUPPORTED;
    const bool g = d->res_mode == ESR_RES_PRE_ACT;
    const int c8 = esr_round_up(d->post_cout, 8);
    if (!esr_view_fits(d->in, 8, RH_C) || !esr_view_fits(d->out1, 8, RH_C) || !esr_view_fits(d->post_out, 8, c8)) return ESR_ERR_BAD_ARG;
    if (g && (!esr_view_ok(d->res, 8, RH_C) || !esr_view_ok(d->out0, 8, RH_C))) return ESR_ERR_BAD_ARG;
    if (g && (d->out0.ptr == d->in.ptr || d->out0.ptr == d->res.ptr)) return ESR_ERR_BAD_ARG;      // neighbouring tiles read the halo of xin and g
    if (d->out1.ptr == d->in.ptr || (g && d->out1.ptr == d->res.ptr)) return ESR_ERR_BAD_ARG;
    ResHeadK k;
    memset(&k, 0, sizeof(k));
    k.xin = static_cast<const char*>(d->in.ptr);
    k.g = static_cast<const char*>(d->res.ptr);
    k.w1 = static_cast<const char*>(d->wpacked);
    k.w2 = static_cast<const char*>(d->tail_wpacked);
    k.wc = static_cast<const char*>(d->post_wpacked);
    k.x = static_cast<char*>(d->out0.ptr);
    k.u = static_cast<char*>(d->out1.ptr);
    k.c1 = static_cast<char*>(d->post_out.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.g_pitch = d->res.pitch; k.g_coff = d->res.coff;
    k.x_pitch = d->out0.pitch; k.x_coff = d->out0.coff;
    k.u_pitch = d->out1.pitch; k.u_coff = d->out1.coff;
    k.c1_pitch = d->post_out.pitch; k.c1_coff = d->post_out.coff;
    k.c1_cout8 = c8;
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, RH_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const bool bf16 = d->storage == ESR_STORE_BF16;
    if (g) return bf16 ? launch_reshead<true, true>(k, st) : launch_reshead<false, true>(k, st);
    return bf16 ? launch_reshead<true, false>(k, st) : launch_reshead<false, false>(k, st);
}
