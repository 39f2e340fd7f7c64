// esr_hfab.hip -- FMEN's HFAB with one BasicBlock (team03_fmen.py:60-73) as ONE launch (esr_chain_desc with res_mode ESR_RES_GATE; 16-bit storage).
//
//     t1 = lrelu(squeeze(x)), t2 = lrelu(conv1(t1)), t3 = lrelu(conv2(t2)), y = sigmoid(excitate(t3)) * x         (x: 33..64 channels, t_i: <= 16)
//
// As four conv_s16_kernel launches a pixel moves about 490 bytes through HBM (x twice, t1 .. t3 written and read back); here a block stages one
// 16 x 16 output tile's x with a 4-pixel halo ONCE by LDS-DMA and keeps everything else in LDS:
//
//     x   24 x 24 pixels   [chunk][pixel][32 B]    (the conv_s16_kernel stage layout: a B fragment is 16 B of one pixel)
//     t1  22 x 22 pixels   [pixel][32 B]           layer 1 on the x tile minus one pixel per side
//     t2  20 x 20 pixels                           layer 2 ...
//     t3  18 x 18 pixels   (t1's bytes)            layer 3 ...
//     y   16 x 16 pixels   -> HBM                  layer 4 + the gate, x read from the staged tile
//
// The halo is recomputed (the middle layers are 16 channels wide: 5 MFMAs per 16 pixels).  Intermediate pixels outside the image are stored as
// 0 -- every layer's own zero padding --, never computed from clamped data.  x's channels at and beyond cin are zero in LDS: 16-byte pieces
// beyond round_up(cin, 8) are requested with an out-of-range offset (the hardware writes zeros) and the part of the last piece beyond cin is
// cleared after the DMA, so pad slots (50 .. 55 at pitch 56) and the next pixel's bytes never reach an MFMA or the gate.
// The four layers' esr_pack_conv_s16 images are staged once per block (persistent blocks walk the tiles); a layer's A fragments are read into
// registers from LDS at the start of the layer.  Per accumulator: bias as the first MFMA's C, chunks in order, tap pairs in order -- the
// order of conv_s16_kernel --, the same act1 / pack2 / esr_sigmoid epilogue arithmetic, each t_i rounded where the per-layer launches store
// it: the result is bit-identical to the four launches (tests/test_gpu_fmen.py).
// LDS: 50 KB weights + 72 KB x + 15 KB t1 / t3 + 12.5 KB t2 = 150 KB: one 4-wave block per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int HF_T = 16;                                   // output tile (pixels per side)
constexpr int HF_NW = 4;
constexpr int HF_R0 = HF_T + 8, HF_R1 = HF_T + 6, HF_R2 = HF_T + 4, HF_R3 = HF_T + 2;     // region widths of x, t1, t2, t3
constexpr int HF_XCH = HF_R0 * HF_R0 * 32;                 // bytes of one 16-channel chunk of the x tile
constexpr int HF_PAIRS = 5;
constexpr int HF_W1MAX = 4 * HF_PAIRS * 1024, HF_WMID = HF_PAIRS * 1024, HF_W4MAX = 4 * HF_PAIRS * 1024;
constexpr int HF_OFF_W1 = 0, HF_OFF_W2 = HF_OFF_W1 + HF_W1MAX, HF_OFF_W3 = HF_OFF_W2 + HF_WMID, HF_OFF_W4 = HF_OFF_W3 + HF_WMID;
constexpr int HF_OFF_X = HF_OFF_W4 + HF_W4MAX;
constexpr int HF_OFF_T1 = HF_OFF_X + 4 * HF_XCH;
constexpr int HF_OFF_T2 = HF_OFF_T1 + HF_R1 * HF_R1 * 32;
constexpr int HF_LDS = HF_OFF_T2 + HF_R2 * HF_R2 * 32;
static_assert(HF_LDS <= LDS_LIMIT && HF_R3 * HF_R3 <= HF_R1 * HF_R1 && HF_OFF_X % 1024 == 0, "LDS plan");

struct HfabK {
    const char* x;            // NHWC 16-bit block input (cin channels from in_coff)
    const char* w[4];         // esr_pack_conv_s16 blobs: squeeze (cin -> cmid), two cmid -> cmid, excitate (cmid -> cout)
    char* y;                  // NHWC 16-bit gated result
    int N, H, W;
    int in_pitch, in_coff, y_pitch, y_coff;
    int cin;                  // logical input channels: nothing at or beyond them is read
    int cout8;                // channels stored
    float slope;              // LeakyReLU of layers 1 .. 3 as max(v, slope v)
    int tiles_x, tiles_y, ntiles;
};

// One layer over the groups of 16 pixels of its output region (DW x DW pixels; row segments at columns 0 and DW - 16, which overlap when
// DW < 32: the overlap is computed twice and stored twice with the same bits).  Source region SW = DW + 2 wide, NCHK chunks of `cstride` bytes.
// MID: act + rounding into the destination region in LDS (0 outside the image; region origin = tile origin - OFF pixels).  !MID: the gate
// and the store to HBM.  Two groups at a time (independent accumulator chains).
template <bool BF16, bool MID, int NCHK, int NT, int DW, int OFF>
__device__ __forceinline__ void hfab_layer(const HfabK& p, char* const smem, int woff, const float* bias_g, int src, int cstride, int dst,
                                           int n, int x0, int y0)
{
    constexpr int SW = DW + 2;
    constexpr int NSEG = DW > HF_T ? 2 : 1;
    constexpr int NG = DW * NSEG;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, px = lane & 15, kq = lane >> 4;

    i32x4 a[NCHK][HF_PAIRS][NT];
    static_for<NCHK>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        static_for<HF_PAIRS>([&](auto q_) {
            constexpr int q = decltype(q_)::value;
            static_for<NT>([&](auto t_) {
                constexpr int t = decltype(t_)::value;
                a[c][q][t] = *reinterpret_cast<const i32x4*>(smem + woff + ((c * HF_PAIRS + q) * NT + t) * 1024 + lane * 16);
            });
        });
    });
    f32x4 bia[NT];
    static_for<NT>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bia[t] = *reinterpret_cast<const f32x4*>(bias_g + t * 16 + kq * 4);
    });
    int laneoff[HF_PAIRS];                                 // pair q: tap min(2 q + (kq >> 1), 8), channel half kq & 1 (conv_s16_kernel's map)
    static_for<HF_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        const int tap = min(2 * q + (kq >> 1), 8);
        laneoff[q] = ((tap / 3) * SW + px + tap % 3) * 32 + (kq & 1) * 16;
    });

    for (int g0 = wv; g0 < NG; g0 += 2 * HF_NW) {
        const int g1 = g0 + HF_NW < NG ? g0 + HF_NW : g0;           // (an odd last group is computed twice)
        const int gg[2] = {g0, g1};
        int row[2], col[2], bb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            row[j] = NSEG == 2 ? gg[j] >> 1 : gg[j];
            col[j] = (NSEG == 2 && (gg[j] & 1)) ? DW - HF_T : 0;
            bb[j] = src + (row[j] * SW + col[j]) * 32;
        }
        f32x4 acc[2][NT];
        static_for<NCHK>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            static_for<HF_PAIRS>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                i32x4 b[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + bb[j] + c * cstride + laneoff[q]);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    static_for<NT>([&](auto t_) {
                        constexpr int t = decltype(t_)::value;
                        acc[j][t] = mfma32<BF16>(a[c][q][t], b[j], (c == 0 && q == 0) ? bia[t] : acc[j][t]);
                    });
            });
        });
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gy = y0 - OFF + row[j], gx = x0 - OFF + col[j] + px;
            const bool inside = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            if constexpr (MID) {
                f32x4 v = acc[j][0];
                const float sl = p.slope;
                v.x = act1(v.x, sl); v.y = act1(v.y, sl); v.z = act1(v.z, sl); v.w = act1(v.w, sl);
                uint2 pk;
                pk.x = inside ? pack2<BF16>(v.x, v.y) : 0u;
                pk.y = inside ? pack2<BF16>(v.z, v.w) : 0u;
                *reinterpret_cast<uint2*>(smem + dst + (row[j] * DW + col[j] + px) * 32 + kq * 8) = pk;
            } else {
                // sigmoid(excitate(t3)) * x: x = channels 16 t + 4 kq .. + 3 of the staged tile's pixel (row + 4, px + 4)
                const int xo = HF_OFF_X + ((row[j] + 4) * HF_R0 + px + 4) * 32 + kq * 8;
                char* const yp = p.y + (((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0)) * p.y_pitch * 2 + (size_t)p.y_coff * 2;
                static_for<NT>([&](auto t_) {
                    constexpr int t = decltype(t_)::value;
                    const f32x4 xf = unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + xo + t * HF_XCH));
                    const f32x4 v = acc[j][t];
                    f32x4 o;
                    o.x = esr_sigmoid(v.x) * xf.x; o.y = esr_sigmoid(v.y) * xf.y;
                    o.z = esr_sigmoid(v.z) * xf.z; o.w = esr_sigmoid(v.w) * xf.w;
                    const int ch = t * 16 + kq * 4;
                    if (inside && ch < p.cout8) {
                        uint2 pk;
                        pk.x = pack2<BF16>(o.x, o.y);
                        pk.y = pack2<BF16>(o.z, o.w);
                        *reinterpret_cast<uint2*>(yp + ch * 2) = pk;
                    }
                });
            }
        }
    }
}

// NCH: 16-channel chunks of x (3: cin 33..48, 4: 49..64); the excitate has as many output tiles
template <bool BF16, int NCH>
__global__ __launch_bounds__(64 * HF_NW, 1) void hfab_kernel(const HfabK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int WB[4] = {NCH * HF_PAIRS * 1024, HF_PAIRS * 1024, HF_PAIRS * 1024, HF_PAIRS * NCH * 1024};   // weight image bytes
    constexpr int WO[4] = {HF_OFF_W1, HF_OFF_W2, HF_OFF_W3, HF_OFF_W4};

    // the four weight images, once per block
#pragma unroll
    for (int l = 0; l < 4; ++l)
        for (int i = tid * 16; i < WB[l]; i += 64 * HF_NW * 16)
            *reinterpret_cast<i32x4*>(smem + WO[l] + i) = *reinterpret_cast<const i32x4*>(p.w[l] + i);
    const float* const b1 = reinterpret_cast<const float*>(p.w[0] + WB[0]);
    const float* const b2 = reinterpret_cast<const float*>(p.w[1] + WB[1]);
    const float* const b3 = reinterpret_cast<const float*>(p.w[2] + WB[2]);
    const float* const b4 = reinterpret_cast<const float*>(p.w[3] + WB[3]);

    const size_t img_bytes = (size_t)p.H * p.W * p.in_pitch * 2;
    const int cvalid8 = (p.cin + 7) & ~7;                 // channels moved per pixel: whole 16-byte pieces up to round_up(cin, 8)
    constexpr int ITEMS = NCH * HF_R0 * HF_R0 * 2;        // 16-byte pieces of the x tile
    static_assert(ITEMS % 64 == 0, "whole DMA instructions");
    constexpr int NINST = ITEMS / 64;

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * HF_T, x0 = (rem % p.tiles_x) * HF_T;

        // ---- x with a 4-pixel halo: piece (chunk c, pixel, half h) -> LDS byte HF_OFF_X + c * HF_XCH + pixel * 32 + h * 16 ----------------
        const i32x4 rs = make_rsrc(p.x + (size_t)n * img_bytes, img_bytes);
        for (int i = wv; i < NINST; i += HF_NW) {
            const int item = i * 64 + lane;
            const int c = item / (HF_R0 * HF_R0 * 2), pr = item - c * (HF_R0 * HF_R0 * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 4 + pix / HF_R0, gx = x0 - 4 + pix % HF_R0;
            const int ch = c * 16 + h * 8;
            const bool ok = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W && ch < cvalid8;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + ch) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(HF_OFF_X + i * 1024), voff, rs, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (p.cin & 7) {
            // the last piece holds channels cvalid8 - 8 .. cvalid8 - 1, of which those >= cin are pad slots of the tensor: zero
            const int cl = cvalid8 - 8, keep = p.cin - cl;
            const int base = HF_OFF_X + (cl >> 4) * HF_XCH + ((cl >> 3) & 1) * 16;
            for (int pix = tid; pix < HF_R0 * HF_R0; pix += 64 * HF_NW) {
                i32x4 v = *reinterpret_cast<const i32x4*>(smem + base + pix * 32);
                v.x = keep >= 2 ? v.x : (keep == 1 ? (v.x & 0xffff) : 0);
                v.y = keep >= 4 ? v.y : (keep == 3 ? (v.y & 0xffff) : 0);
                v.z = keep >= 6 ? v.z : (keep == 5 ? (v.z & 0xffff) : 0);
                v.w = keep == 7 ? (v.w & 0xffff) : 0;
                *reinterpret_cast<i32x4*>(smem + base + pix * 32) = v;
            }
            __syncthreads();
        }
        hfab_layer<BF16, true, NCH, 1, HF_R1, 3>(p, smem, HF_OFF_W1, b1, HF_OFF_X, HF_XCH, HF_OFF_T1, n, x0, y0);
        __syncthreads();
        hfab_layer<BF16, true, 1, 1, HF_R2, 2>(p, smem, HF_OFF_W2, b2, HF_OFF_T1, 0, HF_OFF_T2, n, x0, y0);
        __syncthreads();
        hfab_layer<BF16, true, 1, 1, HF_R3, 1>(p, smem, HF_OFF_W3, b3, HF_OFF_T2, 0, HF_OFF_T1, n, x0, y0);
        __syncthreads();
        hfab_layer<BF16, false, 1, NCH, HF_T, 0>(p, smem, HF_OFF_W4, b4, HF_OFF_T1, 0, 0, n, x0, y0);
        __syncthreads();                                  // x and t3 are read: the next tile's DMA may overwrite them
    }
}

template <bool BF16, int NCH>
int launch_hfab(const HfabK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&hfab_kernel<BF16, NCH>), HF_LDS, "hfab_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (LDS), persistent over the tiles
    esr_note_kernel("hfab_kernel<%s, %d>", esr_tf(BF16), NCH);
    hipLaunchKernelGGL((hfab_kernel<BF16, NCH>), dim3(grid), dim3(64 * HF_NW), HF_LDS, st, k);
    return esr_check_launch("hfab_kernel launch");
}

}  // namespace

int esr_hfab_supported(const esr_chain_desc* d)
{
    if (!d || d->res_mode != ESR_RES_GATE || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->n_layers != 4 || d->act != ESR_ACT_LRELU || !(d->slope >= 0.f && d->slope <= 1.f)) return 0;
    if (d->cin != d->cout || d->cin < 33 || d->cin > 64 || d->cmid < 1 || d->cmid > 16) return 0;
    if (d->post_wpacked || d->post2_wpacked) return 0;
    if (d->post_cout < d->cout || d->post_cout > esr_round_up(d->cout, 16)) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    return 1;
}

int esr_hfab_s16(const esr_chain_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->post_out.ptr) return ESR_ERR_BAD_ARG;
    for (int i = 0; i < 4; ++i)
        if (!d->wpacked[i]) return ESR_ERR_BAD_ARG;
    if (!esr_hfab_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int cout8 = esr_round_up(d->post_cout, 8);
    if (!esr_view_fits(d->in, 8, esr_round_up(d->cin, 8)) || !esr_view_fits(d->post_out, 8, cout8)) return ESR_ERR_BAD_ARG;
    HfabK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    for (int i = 0; i < 4; ++i) k.w[i] = static_cast<const char*>(d->wpacked[i]);
    k.y = static_cast<char*>(d->post_out.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.y_pitch = d->post_out.pitch; k.y_coff = d->post_out.coff;
    k.cin = d->cin;
    k.cout8 = cout8;
    k.slope = d->slope;
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, HF_T);
    if (tg.count >= ESR_INDEX_LIMIT) return ESR_ERR_UNSUPPORTED;
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const bool bf16 = d->storage == ESR_STORE_BF16;
    if (esr_round_up(d->cin, 16) == 48) return bf16 ? launch_hfab<true, 3>(k, st) : launch_hfab<false, 3>(k, st);
    return bf16 ? launch_hfab<true, 4>(k, st) : launch_hfab<false, 4>(k, st);
}
