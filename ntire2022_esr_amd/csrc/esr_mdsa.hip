// esr_mdsa.hip -- MDGN's block (MDSA, models/team24_mdgn.py:5-28) on 16-bit storage: a dense 64 -> 64 3x3 with the per-channel nn.PReLU BEHIND
// it in the convolution's epilogue (esr_conv_prelu, conv_prelu_kernel), and the end of the block -- the 192 -> 64 fuse 1x1, its PReLU, the
// one-channel sigmoid gate and the product -- as one streaming launch (esr_mdsa_gate, mdsa_gate_kernel).  prelu(v, a) = v >= 0 ? v : a v with an
// fp32 slope of any sign and size, as esr_prelu (esr_resdb.hip); it is NOT max(v, a v).
//
// conv_prelu_kernel<BF16>:      out[c] = store(prelu(b[c] + sum W[c,k,i,j] in[y+i-1, x+j-1, k], a[c]))          zero padding, ONE rounding
//   A 4-wave block (one wave per SIMD, one block per CU) is persistent over 16 x 16 output tiles.
//   weights   the esr_pack_conv_s16 image -- 4 chunks x 5 tap pairs x 4 output tiles of 1 KB, the very fragments conv_s16_kernel multiplies by,
//             error-diffused taps included -- lives in REGISTERS for the wave's lifetime: 80 fragments = 320 VGPRs of the 512 a wave has at
//             one wave per SIMD.  So no A fragment is ever re-read from LDS, and the LDS holds nothing but the input.
//   input     staged by LDS-DMA with a one-pixel halo as [16-channel chunk][18 x 18 pixels][32 B] (a B fragment of a tap pair is 16 B of one
//             pixel; pieces outside the image arrive as zeros: the zero padding), in a ring of THREE stages of 41 KB: the pieces of tile
//             k + 1 are issued before tile k is computed and waited for with a counted vmcnt, one barrier per tile.
//   compute   a wave takes four image rows of the tile against all four output tiles: per (chunk, tap pair) 4 ds_read_b128 feed 16 MFMAs
//             (v_mfma_f32_16x16x32), a quarter of the LDS read rate at which the array saturates.  Chunks in order, tap pairs in order, from
//             the bias: conv_s16_kernel's order.
//   epilogue  on the accumulators, nothing more: a non-negative value is converted (RNE), a negative one's exact product with the slope is
//             rounded once (esr_s16_dev.h: prelu_store16x4); lane (pixel, kq) holds channels 16 mt + 4 kq + {0 .. 3}: 8-byte stores.  The
//             wave's 16 slopes stay in registers for its lifetime; the 64 biases lie in LDS and start each tile's accumulators.
//
// mdsa_gate_kernel<BF16>:       f = prelu(b_f + W_f . cat(f1, f2, f3), a_f);  s = sigmoid(b_s + w_s . x);  y = store(f * s)
//   One streaming pass: a wave owns 16 consecutive pixels at a time (grid-stride over the groups of 16).  Lane (pixel, kq) loads 16-byte pieces:
//   channels 32 s + 8 kq + {0 .. 7} of each of f1, f2, f3 and x -- for the f_i that IS the B fragment of v_mfma_f32_16x16x32's K step 2 i + s, so
//   the stored values are the operands as they are.  W_f is a hi + lo pair of 16-bit images (w = hi + lo, 48 KB) in LDS, read as A fragments;
//   accumulation is fp32 from the bias, all hi steps, then all lo steps.  The gate is an fp32 dot product on the VALU (16 channels per lane,
//   summed over the four kq lanes of a pixel), esr_sigmoid (ESR_RES_GATE's definition); the PReLU's product, f * s and the store's rounding
//   are one fp32 operation each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_internal.h"
#include "esr_s16_dev.h"

namespace {

// ---- esr_conv_prelu ---------------------------------------------------------------------------------------------------------------------------
constexpr int CP_C = 64;                                   // input = output channels
constexpr int CP_T = 16, CP_R = CP_T + 2, CP_PIX = CP_R * CP_R, CP_NW = 4;
constexpr int CP_NCH = CP_C / 16, CP_PAIRS = 5;
constexpr int CP_XCH = CP_PIX * 32;                        // bytes of one staged 16-channel chunk
constexpr int CP_ITEMS = CP_NCH * CP_PIX * 2;              // 16-byte pieces of a staged tile
constexpr int CP_NINST = (CP_ITEMS + 63) / 64;             // DMA instructions per tile (1 KB each), dealt round-robin to the waves
constexpr int CP_XBYTES = CP_NINST * 1024;                 // one stage: 41 KB
constexpr int CP_NBUF = 3;
constexpr int CP_OFF_BIAS = CP_NBUF * CP_XBYTES;             // 64 fp32 biases behind the stages: read where a tile's accumulators start
constexpr int CP_LDS = CP_OFF_BIAS + CP_C * 4;
constexpr int CP_W3B = CP_NCH * CP_PAIRS * CP_NCH * 1024;  // bytes of the weight image (the fp32 biases lie behind it)
static_assert(CP_LDS <= LDS_LIMIT && CP_OFF_BIAS % 16 == 0 && CP_NCH * CP_XCH <= CP_XBYTES, "LDS plan");

struct CpK {
    const char* x;            // NHWC 16-bit input
    const char* w3;           // esr_pack_conv_s16 blob (64 -> 64, ksize 3)
    const float* a;           // esr_pack_prelu blob: 64 fp32 slopes
    char* y;                  // NHWC 16-bit output
    int N, H, W;
    int in_pitch, in_coff, y_pitch, y_coff;
    int tiles_x, tiles_y, ntiles;
};

template <bool BF16>
__global__ __launch_bounds__(64 * CP_NW, 1) void conv_prelu_kernel(const CpK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, px = lane & 15, kq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

    // the whole weight image and the wave's slopes: registers, once per wave; the biases: LDS
    i32x4 wa[CP_NCH * CP_PAIRS * CP_NCH];
    static_for<CP_NCH * CP_PAIRS * CP_NCH>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        wa[i] = *reinterpret_cast<const i32x4*>(p.w3 + i * 1024 + lane * 16);
    });
    f32x4 slope[CP_NCH];
    static_for<CP_NCH>([&](auto m_) {
        constexpr int mt = decltype(m_)::value;
        slope[mt] = *reinterpret_cast<const f32x4*>(p.a + mt * 16 + kq * 4);
    });
    if (tid < CP_C) *reinterpret_cast<float*>(smem + CP_OFF_BIAS + tid * 4) = *reinterpret_cast<const float*>(p.w3 + CP_W3B + tid * 4);
    int laneoff[CP_PAIRS];                                 // pair q: tap min(2 q + (kq >> 1), 8), channel half kq & 1 (conv_s16_kernel's map)
    static_for<CP_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        const int tap = min(2 * q + (kq >> 1), 8);
        laneoff[q] = ((tap / 3) * CP_R + px + tap % 3) * 32 + (kq & 1) * 16;
    });

    const size_t img_bytes = (size_t)p.H * p.W * p.in_pitch * 2;
    const int per = p.tiles_x * p.tiles_y;
    const int mine = (CP_NINST - wv + CP_NW - 1) / CP_NW;  // DMA instructions this wave issues per tile

    // tile t with a one-pixel halo -> stage `buf`: piece (chunk c, pixel, half h) at byte c * CP_XCH + pixel * 32 + h * 16
    auto stage = [&](int t, int buf) {
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * CP_T, x0 = (rem % p.tiles_x) * CP_T;
        const i32x4 rs = make_rsrc(p.x + (size_t)n * img_bytes, img_bytes);
        for (int i = wv; i < CP_NINST; i += CP_NW) {
            const int item = i * 64 + lane;
            const int c = item / (CP_PIX * 2), pr = item - c * (CP_PIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 1 + pix / CP_R, gx = x0 - 1 + pix % CP_R;
            const bool ok = item < CP_ITEMS && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + c * 16 + h * 8) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(buf * CP_XBYTES + i * 1024), voff, rs, 0u);
        }
    };

    int t = blockIdx.x, buf = 0;
    if (t < p.ntiles) stage(t, 0);
    for (; t < p.ntiles; t += gridDim.x) {
        const int tn = t + (int)gridDim.x;
        const int nbuf = buf + 1 == CP_NBUF ? 0 : buf + 1;
        // the next tile's pieces go to the stage that was read two tiles ago: every wave has passed the previous tile's barrier since
        if (tn < p.ntiles) {
            stage(tn, nbuf);
            wait_vm_dyn(mine);                             // all but the pieces just issued: this tile's have landed (the last tile's stores too)
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();

        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * CP_T, x0 = (rem % p.tiles_x) * CP_T;
        const char* xs = smem + buf * CP_XBYTES;
        int bb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bb[j] = (wv * 4 + j) * CP_R * 32;
        f32x4 acc[4][CP_NCH];
        static_for<CP_NCH>([&](auto m_) {
            constexpr int mt = decltype(m_)::value;
            const f32x4 bv = *reinterpret_cast<const f32x4*>(smem + CP_OFF_BIAS + (mt * 16 + kq * 4) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j][mt] = bv;
        });
        static_for<CP_NCH>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            static_for<CP_PAIRS>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                i32x4 b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const i32x4*>(xs + c * CP_XCH + bb[j] + laneoff[q]);
                static_for<CP_NCH>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[j][tt] = mfma32<BF16>(wa[(c * CP_PAIRS + q) * CP_NCH + tt], b[j], acc[j][tt]);
                });
            });
        });

        // the PReLU on the accumulators, one rounding, stored: lane (px, kq) holds channels 16 mt + 4 kq + {0 .. 3} of pixel px of row j
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gy = y0 + wv * 4 + j, gx = x0 + px;
            if (gy < p.H && gx < p.W) {
                char* yp = p.y + ((((size_t)n * p.H + gy) * p.W + gx) * p.y_pitch + p.y_coff) * 2;
                static_for<CP_NCH>([&](auto m_) {
                    constexpr int mt = decltype(m_)::value;
                    const uint2 o = prelu_store16x4<BF16>(acc[j][mt], slope[mt]);
                    *reinterpret_cast<uint2*>(yp + (mt * 16 + kq * 4) * 2) = o;
                });
            }
        }
        buf = nbuf;
    }
}

template <bool BF16>
int launch_conv_prelu(const CpK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&conv_prelu_kernel<BF16>), CP_LDS, "conv_prelu_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (512 registers per wave), persistent over the tiles
    esr_note_kernel("conv_prelu_kernel<%s>", esr_tf(BF16));
    hipLaunchKernelGGL((conv_prelu_kernel<BF16>), dim3(grid), dim3(64 * CP_NW), CP_LDS, st, k);
    return esr_check_launch("conv_prelu_kernel launch");
}

// ---- esr_mdsa_gate ----------------------------------------------------------------------------------------------------------------------------
constexpr int MG_C = 64, MG_K = 3 * MG_C;                  // output channels; channels of cat(f1, f2, f3)
constexpr int MG_NW = 4;
constexpr int MG_MT = MG_C / 16, MG_KS = MG_K / 32;        // output tiles, K steps
constexpr int MG_IMG = MG_MT * MG_KS * 64 * 16;            // bytes of one 16-bit weight image: [mt][ks][lane][8]
constexpr int MG_OFF_BF = 2 * MG_IMG, MG_OFF_AF = MG_OFF_BF + MG_C * 4, MG_OFF_WS = MG_OFF_AF + MG_C * 4, MG_OFF_BS = MG_OFF_WS + MG_C * 4;
constexpr int MG_BLOB = MG_OFF_BS + 16;
constexpr int MG_GRID_CAP = 768;                           // three blocks of 48 KB LDS per CU

struct MgK {
    const char* f;            // f1; f2 and f3 lie f_step bytes apart
    const char* x;            // the block's input (the gate's operand)
    const char* w;            // esr_pack_mdsa_gate blob
    char* y;
    long long f_step;
    long long npix;
    int ngroups;              // groups of 16 pixels
    int f_pitch, f_coff, x_pitch, x_coff, y_pitch, y_coff;
};

template <bool BF16>
__global__ __launch_bounds__(64 * MG_NW) void mdsa_gate_kernel(const MgK p)
{
    __shared__ __attribute__((aligned(16))) char wimg[2 * MG_IMG];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    for (int i = tid * 16; i < 2 * MG_IMG; i += 64 * MG_NW * 16)
        *reinterpret_cast<i32x4*>(wimg + i) = *reinterpret_cast<const i32x4*>(p.w + i);
    f32x4 bias[MG_MT], slope[MG_MT];
#pragma unroll
    for (int mt = 0; mt < MG_MT; ++mt) {
        bias[mt] = *reinterpret_cast<const f32x4*>(p.w + MG_OFF_BF + (mt * 16 + kq * 4) * 4);
        slope[mt] = *reinterpret_cast<const f32x4*>(p.w + MG_OFF_AF + (mt * 16 + kq * 4) * 4);
    }
    f32x4 ws[2][2];                                        // w_s of the lane's channels 32 s + 8 kq + {0 .. 7}
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        ws[s][0] = *reinterpret_cast<const f32x4*>(p.w + MG_OFF_WS + (32 * s + 8 * kq) * 4);
        ws[s][1] = *reinterpret_cast<const f32x4*>(p.w + MG_OFF_WS + (32 * s + 8 * kq + 4) * 4);
    }
    const float bs = *reinterpret_cast<const float*>(p.w + MG_OFF_BS);
    __syncthreads();

    for (int g = blockIdx.x * MG_NW + wv; g < p.ngroups; g += gridDim.x * MG_NW) {
        const long long pix = (long long)g * 16 + px;
        const bool inside = pix < p.npix;
        const i32x4 zero = {0, 0, 0, 0};
        i32x4 b[MG_KS], xv[2];
        const char* fp = p.f + ((size_t)pix * p.f_pitch + p.f_coff + 8 * kq) * 2;
        const char* xp = p.x + ((size_t)pix * p.x_pitch + p.x_coff + 8 * kq) * 2;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) b[2 * i + s] = inside ? *reinterpret_cast<const i32x4*>(fp + i * p.f_step + 64 * s) : zero;
#pragma unroll
        for (int s = 0; s < 2; ++s) xv[s] = inside ? *reinterpret_cast<const i32x4*>(xp + 64 * s) : zero;

        // the gate: b_s + w_s . x in fp32, the lane's 16 channels, then the four kq lanes of the pixel
        float d = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 lo = unpack4<BF16>(make_uint2((unsigned)xv[s].x, (unsigned)xv[s].y));
            const f32x4 hi = unpack4<BF16>(make_uint2((unsigned)xv[s].z, (unsigned)xv[s].w));
            d = fmaf(ws[s][0].x, lo.x, d); d = fmaf(ws[s][0].y, lo.y, d); d = fmaf(ws[s][0].z, lo.z, d); d = fmaf(ws[s][0].w, lo.w, d);
            d = fmaf(ws[s][1].x, hi.x, d); d = fmaf(ws[s][1].y, hi.y, d); d = fmaf(ws[s][1].z, hi.z, d); d = fmaf(ws[s][1].w, hi.w, d);
        }
        d += __shfl_xor(d, 16);
        d += __shfl_xor(d, 32);
        const float sg = esr_sigmoid(bs + d);

        const size_t yo = ((size_t)pix * p.y_pitch + p.y_coff) * 2;
        int wo = lane * 16;                                // (opaque to the compiler: the 48 A fragments are read from LDS per group, not hoisted
        asm volatile("" : "+v"(wo));                       // into 192 registers that would leave one wave per SIMD to hide the loads' latency)
#pragma unroll
        for (int mt = 0; mt < MG_MT; ++mt) {
            f32x4 a = bias[mt];
#pragma unroll
            for (int ks = 0; ks < MG_KS; ++ks)
                a = mfma32<BF16>(*reinterpret_cast<const i32x4*>(wimg + (mt * MG_KS + ks) * 1024 + wo), b[ks], a);
#pragma unroll
            for (int ks = 0; ks < MG_KS; ++ks)
                a = mfma32<BF16>(*reinterpret_cast<const i32x4*>(wimg + MG_IMG + (mt * MG_KS + ks) * 1024 + wo), b[ks], a);
            f32x4 v;
            v.x = __fmul_rn(a.x >= 0.f ? a.x : __fmul_rn(slope[mt].x, a.x), sg);
            v.y = __fmul_rn(a.y >= 0.f ? a.y : __fmul_rn(slope[mt].y, a.y), sg);
            v.z = __fmul_rn(a.z >= 0.f ? a.z : __fmul_rn(slope[mt].z, a.z), sg);
            v.w = __fmul_rn(a.w >= 0.f ? a.w : __fmul_rn(slope[mt].w, a.w), sg);
            if (inside) {
                uint2 o;
                o.x = pack2<BF16>(v.x, v.y);
                o.y = pack2<BF16>(v.z, v.w);
                *reinterpret_cast<uint2*>(p.y + yo + (mt * 16 + kq * 4) * 2) = o;
            }
        }
    }
}

template <bool BF16>
int launch_mdsa_gate(const MgK& k, hipStream_t st)
{
    const int blocks = (k.ngroups + MG_NW - 1) / MG_NW;
    esr_note_kernel("mdsa_gate_kernel<%s>", esr_tf(BF16));
    hipLaunchKernelGGL((mdsa_gate_kernel<BF16>), dim3(blocks < MG_GRID_CAP ? blocks : MG_GRID_CAP), dim3(64 * MG_NW), 0, st, k);
    return esr_check_launch("mdsa_gate_kernel launch");
}

}  // namespace

extern "C" {

int esr_conv_prelu_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->ksize != 3 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->cin != CP_C || d->cout != CP_C) return 0;
    if (d->act != ESR_ACT_NONE || d->res_mode != ESR_RES_NONE) return 0;
    if (d->split || d->res.ptr || d->out1.ptr || d->tail_cat.ptr || d->tail_cat_c || d->tail_cout || d->tail_mid_act || d->tail_seg_stride16 || d->post_wpacked ||
        d->post_out.ptr || d->post_cout || d->post_act || d->post2_wpacked || d->post2_out.ptr || d->post2_cout || d->border_bias || d->blocked8 ||
        d->in_seg_stride || d->in_seg_chunks || d->wino_wpacked || d->hilo || d->hilo_stride) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, CP_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_conv_prelu(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->wpacked || !d->tail_wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_conv_prelu_supported(d)) return ESR_ERR_UNSUPPORTED;
    if (!esr_view_ok(d->in, 8, CP_C) || !esr_view_ok(d->out0, 8, CP_C)) return ESR_ERR_BAD_ARG;
    // no byte of the output belongs to the input: the neighbouring tiles read it as halo
    if (esr_views_meet(d->out0, CP_C, d->in, CP_C, (size_t)d->n * d->h * d->w, 2)) return ESR_ERR_BAD_ARG;
    CpK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.w3 = static_cast<const char*>(d->wpacked);
    k.a = static_cast<const float*>(d->tail_wpacked);
    k.y = static_cast<char*>(d->out0.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, CP_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return d->storage == ESR_STORE_BF16 ? launch_conv_prelu<true>(k, st) : launch_conv_prelu<false>(k, st);
}

size_t esr_packed_mdsa_gate_bytes(int storage)
{
    return esr_is_s16(storage) ? (size_t)MG_BLOB : 0;
}

int esr_pack_mdsa_gate(const float* w_f, const float* b_f, const float* a_f, const float* w_s, const float* b_s, int storage, void* out, size_t out_bytes)
{
    const size_t need = esr_packed_mdsa_gate_bytes(storage);
    if (!w_f || !a_f || !w_s || !out || !need || out_bytes < need) return ESR_ERR_BAD_ARG;
    memset(out, 0, need);
    char* o = static_cast<char*>(out);
    for (int mt = 0; mt < MG_MT; ++mt)
        for (int ks = 0; ks < MG_KS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const float v = w_f[(size_t)(mt * 16 + (lane & 15)) * MG_K + 32 * ks + 8 * (lane >> 4) + e];
                    const uint16_t hi = esr_host_to16(v, storage);
                    const uint16_t lo = esr_host_to16((float)((double)v - esr_host_from16(hi, storage)), storage);
                    const size_t at = ((size_t)((mt * MG_KS + ks) * 64 + lane) * 8 + e) * 2;
                    memcpy(o + at, &hi, 2);
                    memcpy(o + MG_IMG + at, &lo, 2);
                }
    if (b_f) memcpy(o + MG_OFF_BF, b_f, MG_C * 4);
    memcpy(o + MG_OFF_AF, a_f, MG_C * 4);
    memcpy(o + MG_OFF_WS, w_s, MG_C * 4);
    if (b_s) memcpy(o + MG_OFF_BS, b_s, 4);
    return ESR_OK;
}

int esr_unpack_mdsa_gate(const void* packed, size_t packed_bytes, int storage, float* w_f, float* b_f, float* a_f, float* w_s, float* b_s)
{
    const size_t need = esr_packed_mdsa_gate_bytes(storage);
    if (!packed || !w_f || !b_f || !a_f || !w_s || !b_s || !need || packed_bytes < need) return ESR_ERR_BAD_ARG;
    const char* o = static_cast<const char*>(packed);
    for (int mt = 0; mt < MG_MT; ++mt)
        for (int ks = 0; ks < MG_KS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    uint16_t hi, lo;
                    const size_t at = ((size_t)((mt * MG_KS + ks) * 64 + lane) * 8 + e) * 2;
                    memcpy(&hi, o + at, 2);
                    memcpy(&lo, o + MG_IMG + at, 2);
                    w_f[(size_t)(mt * 16 + (lane & 15)) * MG_K + 32 * ks + 8 * (lane >> 4) + e] =
                        (float)((double)esr_host_from16(hi, storage) + (double)esr_host_from16(lo, storage));
                }
    memcpy(b_f, o + MG_OFF_BF, MG_C * 4);
    memcpy(a_f, o + MG_OFF_AF, MG_C * 4);
    memcpy(w_s, o + MG_OFF_WS, MG_C * 4);
    memcpy(b_s, o + MG_OFF_BS, 4);
    return ESR_OK;
}

int esr_mdsa_gate_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->ksize != 1 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->cin != MG_K || d->cout != MG_C) return 0;
    if (d->act != ESR_ACT_NONE || d->res_mode != ESR_RES_GATE) return 0;
    if (d->in_seg_stride ? (d->in_seg_stride < 0 || (d->in_seg_stride & 15) || d->in_seg_chunks != MG_C / 16) : d->in_seg_chunks != 0) return 0;
    if (d->split || d->out1.ptr || d->tail_wpacked || d->tail_cat.ptr || d->tail_cat_c || d->tail_cout || d->tail_mid_act || d->tail_seg_stride16 || d->post_wpacked ||
        d->post_out.ptr || d->post_cout || d->post_act || d->post2_wpacked || d->post2_out.ptr || d->post2_cout || d->border_bias || d->blocked8 ||
        d->wino_wpacked || d->hilo || d->hilo_stride) return 0;
    if ((double)d->n * d->h * d->w >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_mdsa_gate(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->res.ptr || !d->out0.ptr || !d->wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_mdsa_gate_supported(d)) return ESR_ERR_UNSUPPORTED;
    const bool planar = d->in_seg_stride != 0;
    if (!esr_view_ok(d->in, 8, planar ? MG_C : MG_K) || !esr_view_ok(d->res, 8, MG_C) || !esr_view_ok(d->out0, 8, MG_C)) return ESR_ERR_BAD_ARG;
    MgK k;
    memset(&k, 0, sizeof(k));
    k.f = static_cast<const char*>(d->in.ptr);
    k.x = static_cast<const char*>(d->res.ptr);
    k.y = static_cast<char*>(d->out0.ptr);
    k.f_step = planar ? d->in_seg_stride : (long long)MG_C * 2;
    // y shares no byte with f1 .. f3 or x: the op is not specified in place (esr_bytes_overlap over the whole tensors)
    const size_t npx = (size_t)d->n * d->h * d->w;
    const size_t f_n = npx * d->in.pitch * 2, x_n = npx * d->res.pitch * 2, y_n = npx * d->out0.pitch * 2;
    for (int i = 0; i < (planar ? 3 : 1); ++i)
        if (esr_bytes_overlap(k.y, y_n, k.f + i * k.f_step, f_n)) return ESR_ERR_BAD_ARG;
    if (esr_bytes_overlap(k.y, y_n, k.x, x_n)) return ESR_ERR_BAD_ARG;
    k.w = static_cast<const char*>(d->wpacked);
    k.npix = (long long)npx;
    k.ngroups = (int)((k.npix + 15) / 16);
    k.f_pitch = d->in.pitch; k.f_coff = d->in.coff;
    k.x_pitch = d->res.pitch; k.x_coff = d->res.coff;
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return d->storage == ESR_STORE_BF16 ? launch_mdsa_gate<true>(k, st) : launch_mdsa_gate<false>(k, st);
}

}  // extern "C"
