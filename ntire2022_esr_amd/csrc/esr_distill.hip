// esr_distill.hip -- one distillation step of BMDN's block (team37_bmdn.py:154-171) as ONE launch (esr_distill_step_s16; 16-bit storage).
//
//     d   = relu(W_d . in + b_d)                                  1x1, cin (17..48) -> cmid (17..32), stored 16-bit (post_out)
//     out = relu(W_3 (*) [in | d~] + b_3  (+ in))                 3x3 over cin + cmid channels -> cout (17..32)           (post2_out)
//
// d~ is d AS STORED (rounded to the storage type) and 0 outside the image: the reference zero-pads d, so a halo pixel outside the image is
// 0, not relu(b_d).  W_3 / b_3 are the fold of the block's two 3x3s over the same pixel, cat([W_r, W_b], 1) and b_r + b_b
// (engine.pack_distill_s16).  As three launches (1x1, 3x3 over d, 3x3 over in + the sum) a pixel moves 440 / 320 bytes through HBM
// (cin = 40 / 20); here `in` is read once and d and out are written once: 160 / 120 bytes.
//
// A block owns one 16 x 16 output tile at a time (persistent over the tiles) and keeps in LDS
//
//     in  18 x 18 pixels   [chunk][pixel][32 B]    staged ONCE with a one-pixel halo by LDS-DMA (conv_s16_kernel's stage layout: a B fragment
//                                                  is 16 B of one pixel); pieces outside the image arrive as zeros
//     d   18 x 18 pixels   [chunk][pixel][32 B]    the 1x1 on every staged pixel (the halo ring is recomputed: 324 instead of 256 pixels, on
//                                                  the cheap layer), rounded, 0 outside the image; its centre also goes to post_out
//
// and the 1x1's esr_pack_conv_s16 image (6 KB).  The 3x3's image -- (NCH + 2) chunks x 5 tap pairs x 2 output tiles = 40 / 50 A fragments --
// lives in REGISTERS for the block's lifetime (160 / 200 VGPRs of the 512 a lone wave per SIMD has): each wave computes four image rows of
// the tile at a time against every fragment, so a B fragment read from LDS feeds two MFMAs and no A fragment is read again.
// Per accumulator: bias as the first MFMA's C, chunks in order (in's, then d's), tap pairs in order -- conv_s16_kernel's order.  The
// residual (ESR_RES_PRE_ACT, cin == cout) is added from the staged tile's centre, not read again.
// `in`'s channels at and beyond cin are zero in LDS: 16-byte pieces beyond round_up(cin, 8) are requested with an out-of-range offset (the
// hardware writes zeros) and the part of the last piece beyond cin is cleared after the DMA, so a tensor's pad slots and the bytes behind it
// never reach an MFMA or the residual.
// LDS: 6 KB + 31 KB in + 21 KB d = 58 KB; one 4-wave block per CU (registers).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int DS_T = 16;                                   // output tile (pixels per side)
constexpr int DS_NW = 4;
constexpr int DS_R = DS_T + 2;                             // staged region (pixels per side)
constexpr int DS_PIX = DS_R * DS_R;
constexpr int DS_G1 = (DS_PIX + 15) / 16;                  // groups of 16 pixels of the 1x1 (the last one is partial)
constexpr int DS_XCH = DS_PIX * 32;                        // bytes of one 16-channel chunk of the staged input
constexpr int DS_DCH = DS_G1 * 16 * 32;                    // ... of d (whole groups: the partial group's pad pixels are stored, as zeros)
constexpr int DS_PAIRS = 5;
constexpr int DS_NT = 2;                                   // output tiles of both layers (cmid, cout in 17..32)
constexpr int DS_MAXCH = 3;                                // chunks of `in` (cin <= 48)
constexpr int ds_x_bytes(int nch) { return (nch * DS_PIX * 2 + 63) / 64 * 64 * 16; }      // whole DMA instructions (64 pieces of 16 bytes)
constexpr int DS_OFF_W1 = 0;
constexpr int DS_OFF_X = DS_MAXCH * DS_NT * 1024;
constexpr int DS_OFF_D = DS_OFF_X + ds_x_bytes(DS_MAXCH);
constexpr int DS_LDS = DS_OFF_D + DS_NT * DS_DCH;
// the 1x1's partial last group reads pixels DS_PIX .. 16 DS_G1 - 1 of every chunk: bytes of the next chunk, of the DMA's zero pad behind the last
static_assert(DS_LDS <= LDS_LIMIT && DS_OFF_X % 1024 == 0 && DS_OFF_D % 16 == 0, "LDS plan");
static_assert(2 * DS_XCH + DS_DCH <= ds_x_bytes(3) && DS_XCH + DS_DCH <= ds_x_bytes(2), "the partial group's reads stay inside the staged bytes");

struct DistK {
    const char* x;            // NHWC 16-bit input (cin channels from in_coff)
    const char* w1;           // esr_pack_conv_s16 blob of the 1x1 (cin -> cmid; hi + lo)
    const char* w3;           // esr_pack_conv_s16 blob of the folded 3x3 over [in chunks | d chunks] (-> cout)
    char* d;                  // NHWC 16-bit distilled map
    char* y;                  // NHWC 16-bit step result
    int N, H, W;
    int in_pitch, in_coff, d_pitch, d_coff, y_pitch, y_coff;
    int cin;                  // logical input channels: nothing at or beyond them is read
    int d_cout8, y_cout8;     // channels stored
    int tiles_x, tiles_y, ntiles;
};

__device__ __forceinline__ f32x4 ds_relu(f32x4 v)
{
    v.x = act1(v.x, 0.f); v.y = act1(v.y, 0.f); v.z = act1(v.z, 0.f); v.w = act1(v.w, 0.f);
    return v;
}

// NCH: 16-channel chunks of `in` (3: cin 33..48, 2: 17..32); RES: + in before the activation (cin == cout: NCH == 2)
template <bool BF16, int NCH, bool RES>
__global__ __launch_bounds__(64 * DS_NW, 1) void distill_step_kernel(const DistK p)
{
    static_assert(!RES || NCH == DS_NT, "the residual is the input: as many chunks as output tiles");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    constexpr int NC3 = NCH + DS_NT;                       // chunks of the 3x3: in's, then d's
    constexpr int W1B = NCH * DS_NT * 1024, W3B = NC3 * DS_PAIRS * DS_NT * 1024;       // weight image bytes

    // the 1x1's image into LDS, the 3x3's into registers: once per block
    for (int i = tid * 16; i < W1B; i += 64 * DS_NW * 16)
        *reinterpret_cast<i32x4*>(smem + DS_OFF_W1 + i) = *reinterpret_cast<const i32x4*>(p.w1 + i);
    i32x4 a3[NC3][DS_PAIRS][DS_NT];
    static_for<NC3>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        static_for<DS_PAIRS>([&](auto q_) {
            constexpr int q = decltype(q_)::value;
            static_for<DS_NT>([&](auto t_) {
                constexpr int t = decltype(t_)::value;
                a3[c][q][t] = *reinterpret_cast<const i32x4*>(p.w3 + ((c * DS_PAIRS + q) * DS_NT + t) * 1024 + lane * 16);
            });
        });
    });
    f32x4 bia1[DS_NT], bia3[DS_NT];
    static_for<DS_NT>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bia1[t] = *reinterpret_cast<const f32x4*>(p.w1 + W1B + (t * 16 + kq * 4) * 4);
        bia3[t] = *reinterpret_cast<const f32x4*>(p.w3 + W3B + (t * 16 + kq * 4) * 4);
    });
    int laneoff[DS_PAIRS];                                 // pair q: tap min(2 q + (kq >> 1), 8), channel half kq & 1 (conv_s16_kernel's map)
    static_for<DS_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        const int tap = min(2 * q + (kq >> 1), 8);
        laneoff[q] = ((tap / 3) * DS_R + px + tap % 3) * 32 + (kq & 1) * 16;
    });

    const size_t img_bytes = (size_t)p.H * p.W * p.in_pitch * 2;
    const int cvalid8 = (p.cin + 7) & ~7;                 // channels moved per pixel: whole 16-byte pieces up to round_up(cin, 8)
    constexpr int ITEMS = NCH * DS_PIX * 2;               // 16-byte pieces of the staged input
    constexpr int NINST = (ITEMS + 63) / 64;              // (the last instruction's pieces beyond ITEMS: zeros behind the last chunk)

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * DS_T, x0 = (rem % p.tiles_x) * DS_T;

        // ---- in with a one-pixel halo: piece (chunk c, pixel, half h) -> LDS byte DS_OFF_X + c * DS_XCH + pixel * 32 + h * 16 -----------------
        const i32x4 rs = make_rsrc(p.x + (size_t)n * img_bytes, img_bytes);
        for (int i = wv; i < NINST; i += DS_NW) {
            const int item = i * 64 + lane;
            const int c = item / (DS_PIX * 2), pr = item - c * (DS_PIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 1 + pix / DS_R, gx = x0 - 1 + pix % DS_R;
            const int ch = c * 16 + h * 8;
            const bool ok = item < ITEMS && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W && ch < cvalid8;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + ch) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(DS_OFF_X + i * 1024), voff, rs, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (p.cin & 7) {
            // the last piece holds channels cvalid8 - 8 .. cvalid8 - 1, of which those >= cin are pad slots of the tensor: zero
            const int cl = cvalid8 - 8, keep = p.cin - cl;
            const int base = DS_OFF_X + (cl >> 4) * DS_XCH + ((cl >> 3) & 1) * 16;
            for (int pix = tid; pix < DS_PIX; pix += 64 * DS_NW) {
                i32x4 v = *reinterpret_cast<const i32x4*>(smem + base + pix * 32);
                v.x = keep >= 2 ? v.x : (keep == 1 ? (v.x & 0xffff) : 0);
                v.y = keep >= 4 ? v.y : (keep == 3 ? (v.y & 0xffff) : 0);
                v.z = keep >= 6 ? v.z : (keep == 5 ? (v.z & 0xffff) : 0);
                v.w = keep == 7 ? (v.w & 0xffff) : 0;
                *reinterpret_cast<i32x4*>(smem + base + pix * 32) = v;
            }
            __syncthreads();
        }

        // ---- d = relu(1x1(in)) on every staged pixel, two groups of 16 pixels at a time; K = 32: [hi | lo] weights x the chunk's 16 channels twice
        for (int g0 = wv; g0 < DS_G1; g0 += 2 * DS_NW) {
            const int g1 = g0 + DS_NW < DS_G1 ? g0 + DS_NW : g0;           // (an odd last group is computed twice)
            const int gg[2] = {g0, g1};
            f32x4 acc[2][DS_NT];
            static_for<NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                i32x4 b[2];
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    b[j] = *reinterpret_cast<const i32x4*>(smem + DS_OFF_X + c * DS_XCH + (gg[j] * 16 + px) * 32 + (kq & 1) * 16);
                static_for<DS_NT>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    const i32x4 a = *reinterpret_cast<const i32x4*>(smem + DS_OFF_W1 + (c * DS_NT + tt) * 1024 + lane * 16);
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j][tt] = mfma32<BF16>(a, b[j], c == 0 ? bia1[tt] : acc[j][tt]);
                });
            });
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int pp = gg[j] * 16 + px, ry = pp / DS_R, rx = pp - ry * DS_R;
                const int gy = y0 - 1 + ry, gx = x0 - 1 + rx;
                const bool inside = pp < DS_PIX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                const bool centre = inside && ry >= 1 && ry <= DS_T && rx >= 1 && rx <= DS_T;
                char* const dp = p.d + (((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0)) * p.d_pitch * 2 + (size_t)p.d_coff * 2;
                static_for<DS_NT>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    const f32x4 v = ds_relu(acc[j][tt]);
                    uint2 pk;
                    pk.x = inside ? pack2<BF16>(v.x, v.y) : 0u;           // outside the image: the 3x3's zero padding of d
                    pk.y = inside ? pack2<BF16>(v.z, v.w) : 0u;
                    *reinterpret_cast<uint2*>(smem + DS_OFF_D + tt * DS_DCH + pp * 32 + kq * 8) = pk;
                    const int ch = tt * 16 + kq * 4;
                    if (centre && ch < p.d_cout8) *reinterpret_cast<uint2*>(dp + ch * 2) = pk;
                });
            }
        }
        __syncthreads();

        // ---- out = relu(3x3([in | d]) (+ in)): four image rows of the tile per wave ------------------------------------------------------------
        {
            int bb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bb[j] = (wv * 4 + j) * DS_R * 32;
            f32x4 acc[4][DS_NT];
            static_for<NC3>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                constexpr int src = c < NCH ? DS_OFF_X + c * DS_XCH : DS_OFF_D + (c - NCH) * DS_DCH;
                static_for<DS_PAIRS>([&](auto q_) {
                    constexpr int q = decltype(q_)::value;
                    i32x4 b[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + src + bb[j] + laneoff[q]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        static_for<DS_NT>([&](auto t_) {
                            constexpr int tt = decltype(t_)::value;
                            acc[j][tt] = mfma32<BF16>(a3[c][q][tt], b[j], (c == 0 && q == 0) ? bia3[tt] : acc[j][tt]);
                        });
                });
            });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wv * 4 + j;
                const int gy = y0 + row, gx = x0 + px;
                const bool inside = gy < p.H && gx < p.W;
                char* const yp = p.y + (((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0)) * p.y_pitch * 2 + (size_t)p.y_coff * 2;
                static_for<DS_NT>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    f32x4 v = acc[j][tt];
                    if constexpr (RES) {
                        // + in: channels 16 tt + 4 kq .. + 3 of the staged tile's pixel (row + 1, px + 1)
                        const f32x4 xf = unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + DS_OFF_X + tt * DS_XCH + ((row + 1) * DS_R + px + 1) * 32 + kq * 8));
                        v.x += xf.x; v.y += xf.y; v.z += xf.z; v.w += xf.w;
                    }
                    v = ds_relu(v);
                    const int ch = tt * 16 + kq * 4;
                    if (inside && ch < p.y_cout8) {
                        uint2 pk;
                        pk.x = pack2<BF16>(v.x, v.y);
                        pk.y = pack2<BF16>(v.z, v.w);
                        *reinterpret_cast<uint2*>(yp + ch * 2) = pk;
                    }
                });
            }
        }
        __syncthreads();                                  // in and d are read: the next tile's DMA and 1x1 may overwrite them
    }
}

template <bool BF16, int NCH, bool RES>
int launch_distill(const DistK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&distill_step_kernel<BF16, NCH, RES>), DS_LDS, "distill_step_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (registers), persistent over the tiles
    esr_note_kernel("distill_step_kernel<%s, %d, %s>", esr_tf(BF16), NCH, esr_tf(RES));
    hipLaunchKernelGGL((distill_step_kernel<BF16, NCH, RES>), dim3(grid), dim3(64 * DS_NW), DS_LDS, st, k);
    return esr_check_launch("distill_step_kernel launch");
}

}  // namespace

extern "C" int esr_distill_step_supported(const esr_chain_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->n_layers != 2 || d->act != ESR_ACT_RELU) return 0;
    if (d->res_mode != ESR_RES_NONE && d->res_mode != ESR_RES_PRE_ACT) return 0;
    if (d->cin < 17 || d->cin > 48 || d->cmid < 17 || d->cmid > 32 || d->cout < 17 || d->cout > 32) return 0;
    if (d->res_mode == ESR_RES_PRE_ACT && d->cin != d->cout) return 0;            // the residual is the input
    if (d->post_wpacked || d->post2_wpacked) return 0;
    if (d->post_cout < d->cmid || d->post_cout > esr_round_up(d->cmid, 16)) return 0;
    if (d->post2_cout < d->cout || d->post2_cout > esr_round_up(d->cout, 16)) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    return 1;
}

extern "C" int esr_distill_step_s16(const esr_chain_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->post_out.ptr || !d->post2_out.ptr || !d->wpacked[0] || !d->wpacked[1]) return ESR_ERR_BAD_ARG;
    if (!esr_distill_step_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int d8 = esr_round_up(d->post_cout, 8), y8 = esr_round_up(d->post2_cout, 8);
    if (!esr_view_fits(d->in, 8, esr_round_up(d->cin, 8)) || !esr_view_fits(d->post_out, 8, d8) || !esr_view_fits(d->post2_out, 8, y8)) return ESR_ERR_BAD_ARG;
    DistK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.w1 = static_cast<const char*>(d->wpacked[0]);
    k.w3 = static_cast<const char*>(d->wpacked[1]);
    k.d = static_cast<char*>(d->post_out.ptr);
    k.y = static_cast<char*>(d->post2_out.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.d_pitch = d->post_out.pitch; k.d_coff = d->post_out.coff;
    k.y_pitch = d->post2_out.pitch; k.y_coff = d->post2_out.coff;
    k.cin = d->cin;
    k.d_cout8 = d8; k.y_cout8 = y8;
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, DS_T);
    if (tg.count >= ESR_INDEX_LIMIT) return ESR_ERR_UNSUPPORTED;
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const bool bf16 = d->storage == ESR_STORE_BF16;
    if (d->res_mode == ESR_RES_PRE_ACT) return bf16 ? launch_distill<true, 2, true>(k, st) : launch_distill<false, 2, true>(k, st);
    if (d->cin > 32) return bf16 ? launch_distill<true, 3, false>(k, st) : launch_distill<false, 3, false>(k, st);
    return bf16 ? launch_distill<true, 2, false>(k, st) : launch_distill<false, 2, false>(k, st);
}
