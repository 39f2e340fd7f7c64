// esr_cascade.hip -- the narrowing refinement path of FasterRFDN's block (team25_frfdn/block.py:115-122) as ONE launch
// (esr_refine_cascade_s16; 16-bit storage).  Behind c1_r and its epilogue 1x1 (d2 = lrelu(c2_d . r1), 32 channels) FRFDB runs
//
//     r2 = rnd(lrelu(W2r (*) d2  + b2r + d2))          3x3, 32 -> 32, never stored
//     d3 = rnd(lrelu(W3d  .  r2~ + b3d))               1x1, 32 -> 16, stored (post_out)
//     r3 = rnd(lrelu(W3r (*) d3~ + b3r + d3~))         3x3, 16 -> 16, never stored
//     r4 = rnd(lrelu(W4  (*) r3~ + b4  + r3~))         3x3, 16 -> 16, stored (post2_out)
//
// rnd = one rounding to the storage type, the one the separate launches do when they store.  x~ is x as rounded and 0 OUTSIDE THE IMAGE: the
// reference zero-pads stored tensors, so a halo pixel of r2, d3 or r3 outside the image is 0, not lrelu(bias).  As four launches a pixel moves
// 320 bytes through HBM and the launches -- one or two output tiles over one or two K chunks -- are launch-bound on a single image; here d2 is
// read once and d3 and r4 are written once: 128 bytes, one launch.
//
// A 4-wave block owns one 16 x 16 output tile at a time (persistent over the tiles) and keeps in LDS
//
//     d2   22 x 22 pixels  [chunk][pixel][32 B]   staged with a THREE-pixel halo by LDS-DMA (conv_s16_kernel's stage layout: a B fragment is 16 B
//                                                 of one pixel); pieces outside the image are requested out of range and arrive as zeros
//     r2   20 x 20 pixels  [chunk][pixel][32 B]   the first 3x3 on the tile and a two-pixel ring, rounded, 0 outside the image
//     d3   20 x 20 pixels  [pixel][32 B]          the 1x1 on every pixel of r2, rounded, 0 outside the image; its centre also goes to post_out
//     r3   18 x 18 pixels  [pixel][32 B]          the second 3x3 on the tile and a one-pixel ring, rounded, 0 outside the image
//
// The four weight images -- 2 chunks x 5 tap pairs x 2 output tiles, 2 chunks, 5 tap pairs, 5 tap pairs = 32 A fragments -- live in
// REGISTERS for the block's lifetime (128 VGPRs of the 512 a lone wave per SIMD has).  Per accumulator: bias as the first MFMA's C, chunks in
// order, tap pairs in order, and a 3x3's own input added to output tile t behind the MFMAs of chunk t (the centre pixel of the staged
// chunk) -- conv_s16_kernel's order with the residual that is its input; the 1x1 multiplies a chunk's 16 channels by the [hi | lo] weight
// halves of esr_pack_conv_s16's ksize 1 image.  What is stored is therefore bit-identical to the four launches.
// 32 and 16 channels are whole K chunks and whole 16-byte pieces: nothing is padded and nothing beyond d2's 32 channels is read.
// LDS: 31 KB d2 + 25 KB r2 + 12.5 KB d3 + 10.5 KB r3 = 79 KB; one block per CU (registers).  Staging and MFMAs of consecutive tiles are not
// overlapped.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int RC_T = 16;                                   // output tile (pixels per side)
constexpr int RC_NW = 4;
constexpr int RC_CIN = 32, RC_CM = 16;                     // channels of d2 / r2, of d3 / r3 / r4
constexpr int RC_NCH = RC_CIN / 16;                        // K chunks of d2 and r2 = output tiles of the first 3x3
constexpr int RC_RX = RC_T + 6, RC_XPIX = RC_RX * RC_RX;   // staged region of d2
constexpr int RC_R2 = RC_T + 4, RC_2PIX = RC_R2 * RC_R2;   // region of r2 and d3
constexpr int RC_R3 = RC_T + 2, RC_3PIX = RC_R3 * RC_R3;   // region of r3
constexpr int RC_G2 = RC_2PIX / 16;                        // groups of 16 pixels of r2 / d3
constexpr int RC_G3 = (RC_3PIX + 15) / 16;                 // ... of r3 (the last one is partial)
constexpr int RC_PAIRS = 5;
constexpr int RC_XCH = RC_XPIX * 32;                       // bytes of one 16-channel chunk of the staged d2
constexpr int RC_2CH = RC_2PIX * 32;                       // ... of r2, and of d3
constexpr int RC_3CH = RC_G3 * 16 * 32;                    // ... of r3 (whole groups: the partial group's pad pixels are stored, as zeros)
constexpr int RC_ITEMS = RC_NCH * RC_XPIX * 2;             // 16-byte pieces of the staged d2
constexpr int RC_NINST = (RC_ITEMS + 63) / 64;             // DMA instructions (the last one's pieces beyond RC_ITEMS: zeros behind the last chunk)
constexpr int RC_OFF_X = 0;
constexpr int RC_OFF_R2 = RC_OFF_X + RC_NINST * 1024;
constexpr int RC_OFF_D3 = RC_OFF_R2 + RC_NCH * RC_2CH;
constexpr int RC_OFF_R3 = RC_OFF_D3 + RC_2CH;
constexpr int RC_LDS = RC_OFF_R3 + RC_3CH;
constexpr int RC_W2R = RC_NCH * RC_PAIRS * RC_NCH * 1024;  // weight image bytes of c2_r (the fp32 bias follows), ...
constexpr int RC_W3D = RC_NCH * 1024;                      // ... of c3_d (ksize 1: one [hi | lo] fragment per chunk)
constexpr int RC_W3 = RC_PAIRS * 1024;                     // ... of c3_r and of c4
static_assert(RC_2PIX % 16 == 0, "r2 / d3 are whole groups");
static_assert(RC_LDS <= LDS_LIMIT && RC_OFF_R2 % 16 == 0 && RC_OFF_D3 % 16 == 0 && RC_OFF_R3 % 16 == 0, "LDS plan");

struct CascK {
    const char* x;            // NHWC 16-bit d2 (32 channels from in_coff)
    const char* w2r;          // esr_pack_conv_s16 blobs: c2_r (3x3, 32 -> 32),
    const char* w3d;          // c3_d (1x1, 32 -> 16; hi + lo),
    const char* w3r;          // c3_r (3x3, 16 -> 16),
    const char* w4;           // c4 (3x3, 16 -> 16)
    char* d3;                 // NHWC 16-bit outputs, 16 channels each
    char* r4;
    int N, H, W;
    int in_pitch, in_coff, d3_pitch, d3_coff, r4_pitch, r4_coff;
    float slope;              // of max(v, slope v)
    int tiles_x, tiles_y, ntiles;
};

// the epilogue of every layer: activation, one rounding; 0 where `keep` is false (a pixel outside the image)
template <bool BF16>
__device__ __forceinline__ uint2 rc_act_pack(f32x4 v, float slope, bool keep)
{
    v.x = act1(v.x, slope); v.y = act1(v.y, slope); v.z = act1(v.z, slope); v.w = act1(v.w, slope);
    uint2 pk;
    pk.x = keep ? pack2<BF16>(v.x, v.y) : 0u;
    pk.y = keep ? pack2<BF16>(v.z, v.w) : 0u;
    return pk;
}

template <bool BF16>
__global__ __launch_bounds__(64 * RC_NW, 1) void refine_cascade_kernel(const CascK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;

    // all four weight images into registers: once per block
    i32x4 a2[RC_NCH][RC_PAIRS][RC_NCH], ad[RC_NCH], a3[RC_PAIRS], a4[RC_PAIRS];
    static_for<RC_NCH>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        static_for<RC_PAIRS>([&](auto q_) {
            constexpr int q = decltype(q_)::value;
            static_for<RC_NCH>([&](auto t_) {
                constexpr int t = decltype(t_)::value;
                a2[c][q][t] = *reinterpret_cast<const i32x4*>(p.w2r + ((c * RC_PAIRS + q) * RC_NCH + t) * 1024 + lane * 16);
            });
        });
        ad[c] = *reinterpret_cast<const i32x4*>(p.w3d + c * 1024 + lane * 16);
    });
    static_for<RC_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        a3[q] = *reinterpret_cast<const i32x4*>(p.w3r + q * 1024 + lane * 16);
        a4[q] = *reinterpret_cast<const i32x4*>(p.w4 + q * 1024 + lane * 16);
    });
    f32x4 bia2[RC_NCH];
    static_for<RC_NCH>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bia2[t] = *reinterpret_cast<const f32x4*>(p.w2r + RC_W2R + (t * 16 + kq * 4) * 4);
    });
    const f32x4 biad = *reinterpret_cast<const f32x4*>(p.w3d + RC_W3D + kq * 4 * 4);
    const f32x4 bia3 = *reinterpret_cast<const f32x4*>(p.w3r + RC_W3 + kq * 4 * 4);
    const f32x4 bia4 = *reinterpret_cast<const f32x4*>(p.w4 + RC_W3 + kq * 4 * 4);
    const float slope = p.slope;
    // pair q: tap min(2 q + (kq >> 1), 8), channel half kq & 1 (conv_s16_kernel's map); in the d2 tile (rows of 22), the d3 tile (rows of 20)
    // and the r3 tile (rows of 18; with the lane's pixel of the row)
    int tapx[RC_PAIRS], tapd[RC_PAIRS], tapr[RC_PAIRS];
    static_for<RC_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        const int tap = min(2 * q + (kq >> 1), 8);
        tapx[q] = ((tap / 3) * RC_RX + tap % 3) * 32 + (kq & 1) * 16;
        tapd[q] = ((tap / 3) * RC_R2 + tap % 3) * 32 + (kq & 1) * 16;
        tapr[q] = ((tap / 3) * RC_R3 + px + tap % 3) * 32 + (kq & 1) * 16;
    });

    const size_t in_img = (size_t)p.H * p.W * p.in_pitch * 2;

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * RC_T, x0 = (rem % p.tiles_x) * RC_T;

        // ---- d2 with a three-pixel halo: piece (chunk c, pixel, half h) -> LDS byte c * RC_XCH + pixel * 32 + h * 16 --------------------------------
        // (the previous tile's last reads of this region lie three barriers back)
        const i32x4 rs = make_rsrc(p.x + (size_t)n * in_img, in_img);
        for (int i = wv; i < RC_NINST; i += RC_NW) {
            const int item = i * 64 + lane;
            const int c = item / (RC_XPIX * 2), pr = item - c * (RC_XPIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 3 + pix / RC_RX, gx = x0 - 3 + pix % RC_RX;
            const bool ok = item < RC_ITEMS && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + c * 16 + h * 8) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(RC_OFF_X + i * 1024), voff, rs, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        // ---- r2 = lrelu(3x3(d2) + d2) on the 20 x 20 region, two groups of 16 pixels at a time; 0 outside the image ---------------------------------
        for (int g0 = wv; g0 < RC_G2; g0 += 2 * RC_NW) {
            const int g1 = g0 + RC_NW < RC_G2 ? g0 + RC_NW : g0;           // (an odd last group is computed twice)
            const int gg[2] = {g0, g1};
            int pp[2], ry[2], rx[2], bx[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                pp[j] = gg[j] * 16 + px;
                ry[j] = pp[j] / RC_R2; rx[j] = pp[j] - ry[j] * RC_R2;
                bx[j] = (ry[j] * RC_RX + rx[j]) * 32;                      // r2 pixel (ry, rx) = d2 pixel (ry + 1, rx + 1): its window starts at (ry, rx)
            }
            f32x4 acc[2][RC_NCH];
            static_for<RC_NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                static_for<RC_PAIRS>([&](auto q_) {
                    constexpr int q = decltype(q_)::value;
                    i32x4 b[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + RC_OFF_X + c * RC_XCH + bx[j] + tapx[q]);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        static_for<RC_NCH>([&](auto t_) {
                            constexpr int tt = decltype(t_)::value;
                            acc[j][tt] = mfma32<BF16>(a2[c][q][tt], b[j], (c == 0 && q == 0) ? bia2[tt] : acc[j][tt]);
                        });
                });
                // + d2: output channels 16 c + 4 kq .. + 3 are the centre pixel of chunk c, added behind that chunk's MFMAs (conv_s16_kernel's res_in)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[j][c] += unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + RC_OFF_X + c * RC_XCH + bx[j] + (RC_RX + 1) * 32 + kq * 8));
            });
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int gy = y0 - 2 + ry[j], gx = x0 - 2 + rx[j];
                const bool inside = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                static_for<RC_NCH>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    *reinterpret_cast<uint2*>(smem + RC_OFF_R2 + tt * RC_2CH + pp[j] * 32 + kq * 8) = rc_act_pack<BF16>(acc[j][tt], slope, inside);
                });
            }
        }
        __syncthreads();

        // ---- d3 = lrelu(1x1(r2)) on the same region; K = 32: [hi | lo] weights x the chunk's 16 channels twice; the centre is stored ---------------
        for (int g0 = wv; g0 < RC_G2; g0 += 2 * RC_NW) {
            const int g1 = g0 + RC_NW < RC_G2 ? g0 + RC_NW : g0;
            const int gg[2] = {g0, g1};
            f32x4 acc[2];
            static_for<RC_NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const i32x4 b = *reinterpret_cast<const i32x4*>(smem + RC_OFF_R2 + c * RC_2CH + (gg[j] * 16 + px) * 32 + (kq & 1) * 16);
                    acc[j] = mfma32<BF16>(ad[c], b, c == 0 ? biad : acc[j]);
                }
            });
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int pp = gg[j] * 16 + px, ry = pp / RC_R2, rx = pp - ry * RC_R2;
                const int gy = y0 - 2 + ry, gx = x0 - 2 + rx;
                const bool inside = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                const uint2 pk = rc_act_pack<BF16>(acc[j], slope, inside);
                *reinterpret_cast<uint2*>(smem + RC_OFF_D3 + pp * 32 + kq * 8) = pk;
                if (inside && ry >= 2 && ry < 2 + RC_T && rx >= 2 && rx < 2 + RC_T)
                    *reinterpret_cast<uint2*>(p.d3 + (((size_t)n * p.H + gy) * p.W + gx) * p.d3_pitch * 2 + (size_t)(p.d3_coff + kq * 4) * 2) = pk;
            }
        }
        __syncthreads();

        // ---- r3 = lrelu(3x3(d3) + d3) on the 18 x 18 region; 0 outside the image --------------------------------------------------------------------
        for (int g0 = wv; g0 < RC_G3; g0 += 2 * RC_NW) {
            const int g1 = g0 + RC_NW < RC_G3 ? g0 + RC_NW : g0;
            const int gg[2] = {g0, g1};
            int pp[2], ry[2], rx[2], bx[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                pp[j] = gg[j] * 16 + px;
                const int pc = min(pp[j], RC_3PIX - 1);                    // (the partial group's pad pixels read the last pixel's window)
                ry[j] = pc / RC_R3; rx[j] = pc - ry[j] * RC_R3;
                bx[j] = (ry[j] * RC_R2 + rx[j]) * 32;                      // r3 pixel (ry, rx) = d3 pixel (ry + 1, rx + 1)
            }
            f32x4 acc[2];
            static_for<RC_PAIRS>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                i32x4 b[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + RC_OFF_D3 + bx[j] + tapd[q]);
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = mfma32<BF16>(a3[q], b[j], q == 0 ? bia3 : acc[j]);
            });
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[j] += unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + RC_OFF_D3 + bx[j] + (RC_R2 + 1) * 32 + kq * 8));
                const int gy = y0 - 1 + ry[j], gx = x0 - 1 + rx[j];
                const bool inside = pp[j] < RC_3PIX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                *reinterpret_cast<uint2*>(smem + RC_OFF_R3 + pp[j] * 32 + kq * 8) = rc_act_pack<BF16>(acc[j], slope, inside);
            }
        }
        __syncthreads();

        // ---- r4 = lrelu(3x3(r3) + r3) on the tile: four image rows per wave --------------------------------------------------------------------------
        {
            f32x4 acc[4];
            static_for<RC_PAIRS>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                i32x4 b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + RC_OFF_R3 + (wv * 4 + j) * RC_R3 * 32 + tapr[q]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = mfma32<BF16>(a4[q], b[j], q == 0 ? bia4 : acc[j]);
            });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wv * 4 + j;
                acc[j] += unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + RC_OFF_R3 + ((row + 1) * RC_R3 + px + 1) * 32 + kq * 8));
                const int gy = y0 + row, gx = x0 + px;
                const uint2 pk = rc_act_pack<BF16>(acc[j], slope, true);
                if (gy < p.H && gx < p.W)
                    *reinterpret_cast<uint2*>(p.r4 + (((size_t)n * p.H + gy) * p.W + gx) * p.r4_pitch * 2 + (size_t)(p.r4_coff + kq * 4) * 2) = pk;
            }
        }
        // (no barrier here: the next tile's DMA and layers each overwrite a region whose last reader lies at least one barrier back)
    }
}

template <bool BF16>
int launch_cascade(const CascK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&refine_cascade_kernel<BF16>), RC_LDS, "refine_cascade_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (registers), persistent over the tiles
    esr_note_kernel("refine_cascade_kernel<%s>", esr_tf(BF16));
    hipLaunchKernelGGL((refine_cascade_kernel<BF16>), dim3(grid), dim3(64 * RC_NW), RC_LDS, st, k);
    return esr_check_launch("refine_cascade_kernel launch");
}

}  // namespace

extern "C" int esr_refine_cascade_supported(const esr_chain_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->n_layers != 4 || d->act != ESR_ACT_LRELU || d->res_mode != ESR_RES_PRE_ACT) return 0;
    if (d->cin != RC_CIN || d->cmid != RC_CM || d->cout != RC_CM) return 0;
    if (d->post_wpacked || d->post2_wpacked) return 0;
    if (d->post_cout != RC_CM || d->post2_cout != RC_CM) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, RC_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

extern "C" int esr_refine_cascade_s16(const esr_chain_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->post_out.ptr || !d->post2_out.ptr || !d->wpacked[0] || !d->wpacked[1] || !d->wpacked[2] || !d->wpacked[3]) return ESR_ERR_BAD_ARG;
    if (!esr_refine_cascade_supported(d)) return ESR_ERR_UNSUPPORTED;
    if (!esr_view_fits(d->in, 8, RC_CIN) || !esr_view_fits(d->post_out, 8, RC_CM) || !esr_view_fits(d->post2_out, 8, RC_CM)) return ESR_ERR_BAD_ARG;
    if (d->post_out.ptr == d->in.ptr || d->post2_out.ptr == d->in.ptr) return ESR_ERR_BAD_ARG;      // neighbouring tiles read the halo of d2
    CascK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.w2r = static_cast<const char*>(d->wpacked[0]);
    k.w3d = static_cast<const char*>(d->wpacked[1]);
    k.w3r = static_cast<const char*>(d->wpacked[2]);
    k.w4 = static_cast<const char*>(d->wpacked[3]);
    k.d3 = static_cast<char*>(d->post_out.ptr);
    k.r4 = static_cast<char*>(d->post2_out.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.d3_pitch = d->post_out.pitch; k.d3_coff = d->post_out.coff;
    k.r4_pitch = d->post2_out.pitch; k.r4_coff = d->post2_out.coff;
    k.slope = esr_act_slope(d->act, d->slope);
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, RC_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return d->storage == ESR_STORE_BF16 ? launch_cascade<true>(k, st) : launch_cascade<false>(k, st);
}
