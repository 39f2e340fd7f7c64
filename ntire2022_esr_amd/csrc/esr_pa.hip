// esr_pa.hip -- pixel attention (PA, models/team10_repafdn/block.py:151-166) and the long skip behind it, the end of RePAFDN's forward
// (repafdn.py:55-57):
//
//     y = t (.) sigmoid(W . t + b) + s             W: 1x1, C -> C, gates its own input; s: nothing, one tensor, or a hi + lo pair
//
// pa_gate_kernel<ST> (esr_pa_gate; ST = esr_storage of t / s / y: fp32, bf16 or fp16) is one streaming pass: t and s are read once, y is
// written once.  A wave owns 16 consecutive pixels at a time (grid-stride over the groups of 16) and holds W and b in registers for its
// lifetime.  Lane (px, kq) loads channels mt * 16 + kq * 4 + {0 .. 3} (mt = 0 .. 3) of pixel px -- the layout in which the MFMA hands back
// its result -- and the SAME registers are the 1x1's B operand: esr_pack_pa_gate orders the K axis of the A fragments to match, so t
// crosses the memory pipeline once and no LDS is used.
//
//     16-bit storage   v_mfma_f32_16x16x32_{bf16,f16}; K step ks takes the lane's channels of mt = 2 ks, 2 ks + 1.  The weights are a hi + lo
//                      pair of 16-bit images (w = hi + lo, as conv_s16_kernel's 1x1s): the gate's argument reaches -52 on the real
//                      checkpoint, so 8 weight bits would move it by whole units.  The stored t IS the operand: nothing is rounded.
//     fp32 storage     v_mfma_f32_16x16x4_f32; K step (j, i) takes channel j * 16 + kq * 4 + i.
//
// Numerics: the argument is accumulated in fp32 from the bias; g = esr_sigmoid(arg); y = rnd(fl(fl(t g) + s)) with s = fl(s_hi + s_lo) for a
// pair: the product and the sum are fp32 operations of their own (no contraction), one rounding to the storage type at the store.  A hi + lo
// output is split as esr_conv_desc.hilo's ESR_HILO_OUT: hi = rnd(v), lo = rnd(v - hi).  Channels of t at and beyond C are masked to zero
// after the load (whatever the pad slots hold), channels C .. cout - 1 of y are stored as zeros.
//
// pa_tail_kernel<BF16, NCH> (esr_pa_tail; 16-bit storage) is the fused form, ONE launch for LR_conv -> PA -> + s:
//
//     t = conv3x3(x) + b3        zero padding of x at the image border; t stays in the fp32 accumulators and is never stored
//     y = t (.) sigmoid(W . rnd(t) + b) + s
//
// A 4-wave block owns one 16 x 16 output tile at a time, persistent over the tiles, one block per CU.  It keeps the 3x3's esr_pack_conv_s16
// image in LDS for its lifetime (NCH x 5 tap pairs x NCH output tiles of 1 KB: 45 / 80 KB) and stages x with a one-pixel halo by LDS-DMA
// in distill_step_kernel's layout ([chunk][18 x 18 pixels][32 B]; pieces outside the image and beyond round_up(C, 8) channels arrive as
// zeros, the pad slots of the last piece are cleared).  A wave computes four image rows of the tile against every A fragment -- chunks in
// order, tap pairs in order from the bias, conv_s16_kernel's order -- and then gates them in registers: the accumulators of a row ARE in
// pa_gate_kernel's layout (lane (px, kq): channels 16 mt + 4 kq + {0 .. 3}), so t rounded once to the storage type is the gate's B operand
// without leaving the lane, against the same esr_pack_pa_gate blob (hi + lo weights) held in registers.  The fp32 t multiplies the
// sigmoid; s, the masks and the stores are pa_gate_kernel's.  Against the two launches the only difference in value is that t meets the
// product unrounded; the 3x3's weights are esr_pack_conv_s16's (taps rounded with error diffusion), exactly what conv_s16_kernel multiplies by.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int PA_CMAX = 64;
constexpr int PA_NW = 4;                                   // waves per block
constexpr int PA_IMG16 = 4 * 2 * 64 * 16;                  // bytes of one 16-bit weight image: [mt][ks][lane][8]
constexpr int PA_IMG32 = 4 * 16 * 64 * 4;                  // bytes of the fp32 weight image: [mt][step][lane]
constexpr int PA_GRID_CAP = 2048;

struct PaK {
    const char* t;            // NHWC gate input
    const char* s;            // NHWC skip (high parts of a pair), or NULL
    const char* s_lo;         // low parts of a hi + lo skip, or NULL
    char* y;                  // NHWC result (high parts of a pair)
    char* y_lo;               // low parts of a hi + lo result, or NULL
    const char* w;            // esr_pack_pa_gate blob
    long long npix;
    int ngroups;              // groups of 16 pixels
    int t_pitch, t_coff, s_pitch, s_coff, y_pitch, y_coff;
    int c;                    // logical channels
    int cp;                   // channels of t and s that exist in a pixel: round_up(c, 8) (16-bit) / round_up(c, 4) (fp32)
    int cout_store;           // channels stored (c .. cout_store - 1 as zeros)
};

template <int ST>
__global__ __launch_bounds__(64 * PA_NW) void pa_gate_kernel(const PaK p)
{
    constexpr bool S16 = ST != ESR_STORE_F32;
    constexpr bool BF16 = ST == ESR_STORE_BF16;
    constexpr int ES = S16 ? 2 : 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, px = lane & 15, kq = lane >> 4;

    // the weights and the bias into registers: once per wave
    i32x4 wh[S16 ? 4 : 1][2], wl[S16 ? 4 : 1][2];
    float wf[S16 ? 1 : 4][16];
    f32x4 bias[4];
    if constexpr (S16) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                wh[mt][ks] = *reinterpret_cast<const i32x4*>(p.w + ((mt * 2 + ks) * 64 + lane) * 16);
                wl[mt][ks] = *reinterpret_cast<const i32x4*>(p.w + PA_IMG16 + ((mt * 2 + ks) * 64 + lane) * 16);
            }
    } else {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int st = 0; st < 16; ++st) wf[mt][st] = *reinterpret_cast<const float*>(p.w + ((mt * 16 + st) * 64 + lane) * 4);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) bias[mt] = *reinterpret_cast<const f32x4*>(p.w + (S16 ? 2 * PA_IMG16 : PA_IMG32) + (mt * 16 + kq * 4) * 4);

    for (int g = blockIdx.x * PA_NW + wv; g < p.ngroups; g += gridDim.x * PA_NW) {
        const long long pix = (long long)g * 16 + px;
        const bool inside = pix < p.npix;
        const char* tp = p.t + ((size_t)pix * p.t_pitch + p.t_coff) * ES;
        f32x4 tv[4];
        uint2 raw[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int cb = mt * 16 + kq * 4;
            const bool ok = inside && cb < p.cp;
            if constexpr (S16) {
                uint2 r = ok ? *reinterpret_cast<const uint2*>(tp + cb * 2) : make_uint2(0u, 0u);
                r.x &= (cb + 0 < p.c ? 0x0000ffffu : 0u) | (cb + 1 < p.c ? 0xffff0000u : 0u);
                r.y &= (cb + 2 < p.c ? 0x0000ffffu : 0u) | (cb + 3 < p.c ? 0xffff0000u : 0u);
                raw[mt] = r;
                tv[mt] = unpack4<BF16>(r);
            } else {
                f32x4 v = ok ? *reinterpret_cast<const f32x4*>(tp + cb * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
                v.x = cb + 0 < p.c ? v.x : 0.f; v.y = cb + 1 < p.c ? v.y : 0.f;
                v.z = cb + 2 < p.c ? v.z : 0.f; v.w = cb + 3 < p.c ? v.w : 0.f;
                tv[mt] = v;
            }
        }

        // arg = W . t + b on the matrix cores
        f32x4 acc[4];
        if constexpr (S16) {
            const i32x4 b0 = {(int)raw[0].x, (int)raw[0].y, (int)raw[1].x, (int)raw[1].y};
            const i32x4 b1 = {(int)raw[2].x, (int)raw[2].y, (int)raw[3].x, (int)raw[3].y};
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 a = mfma32<BF16>(wh[mt][0], b0, bias[mt]);
                a = mfma32<BF16>(wh[mt][1], b1, a);
                a = mfma32<BF16>(wl[mt][0], b0, a);
                acc[mt] = mfma32<BF16>(wl[mt][1], b1, a);
            }
        } else {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 a = bias[mt];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[mt][j * 4 + 0], tv[j].x, a, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[mt][j * 4 + 1], tv[j].y, a, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[mt][j * 4 + 2], tv[j].z, a, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[mt][j * 4 + 3], tv[j].w, a, 0, 0, 0);
                }
                acc[mt] = a;
            }
        }

        // y = t * sigmoid(arg) + s, stored
        const size_t so = ((size_t)pix * p.s_pitch + p.s_coff) * ES, yo = ((size_t)pix * p.y_pitch + p.y_coff) * ES;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int cb = mt * 16 + kq * 4;
            f32x4 v;
            v.x = __fmul_rn(tv[mt].x, esr_sigmoid(acc[mt].x)); v.y = __fmul_rn(tv[mt].y, esr_sigmoid(acc[mt].y));
            v.z = __fmul_rn(tv[mt].z, esr_sigmoid(acc[mt].z)); v.w = __fmul_rn(tv[mt].w, esr_sigmoid(acc[mt].w));
            if (p.s && inside && cb < p.cp) {
                f32x4 sv;
                if constexpr (S16) {
                    sv = unpack4<BF16>(*reinterpret_cast<const uint2*>(p.s + so + cb * 2));
                    if (p.s_lo) {
                        const f32x4 sl = unpack4<BF16>(*reinterpret_cast<const uint2*>(p.s_lo + so + cb * 2));
                        sv.x = __fadd_rn(sv.x, sl.x); sv.y = __fadd_rn(sv.y, sl.y); sv.z = __fadd_rn(sv.z, sl.z); sv.w = __fadd_rn(sv.w, sl.w);
                    }
                } else {
                    sv = *reinterpret_cast<const f32x4*>(p.s + so + cb * 4);
                }
                v.x = __fadd_rn(v.x, sv.x); v.y = __fadd_rn(v.y, sv.y); v.z = __fadd_rn(v.z, sv.z); v.w = __fadd_rn(v.w, sv.w);
            }
            v.x = cb + 0 < p.c ? v.x : 0.f; v.y = cb + 1 < p.c ? v.y : 0.f;
            v.z = cb + 2 < p.c ? v.z : 0.f; v.w = cb + 3 < p.c ? v.w : 0.f;
            if (!inside || cb >= p.cout_store) continue;
            if constexpr (S16) {
                uint2 hi;
                hi.x = pack2<BF16>(v.x, v.y);
                hi.y = pack2<BF16>(v.z, v.w);
                *reinterpret_cast<uint2*>(p.y + yo + cb * 2) = hi;
                if (p.y_lo) {
                    const f32x4 h = unpack4<BF16>(hi);
                    uint2 lo;
                    lo.x = pack2<BF16>(v.x - h.x, v.y - h.y);
                    lo.y = pack2<BF16>(v.z - h.z, v.w - h.w);
                    *reinterpret_cast<uint2*>(p.y_lo + yo + cb * 2) = lo;
                }
            } else {
                *reinterpret_cast<f32x4*>(p.y + yo + cb * 4) = v;
            }
        }
    }
}

template <int ST>
int launch_pa_gate(const PaK& k, hipStream_t st)
{
    const int blocks = (k.ngroups + PA_NW - 1) / PA_NW;
    esr_note_kernel("pa_gate_kernel<%d>", ST);
    hipLaunchKernelGGL((pa_gate_kernel<ST>), dim3(blocks < PA_GRID_CAP ? blocks : PA_GRID_CAP), dim3(64 * PA_NW), 0, st, k);
    return esr_check_launch("pa_gate_kernel launch");
}

// ---- the fused tail ---------------------------------------------------------------------------------------------------------------------------
constexpr int PT_T = 16;                                   // output tile (pixels per side)
constexpr int PT_NW = 4;
constexpr int PT_R = PT_T + 2;                             // staged region (pixels per side)
constexpr int PT_PIX = PT_R * PT_R;
constexpr int PT_XCH = PT_PIX * 32;                        // bytes of one 16-channel chunk of the staged input
constexpr int PT_PAIRS = 5;
constexpr int PT_MAXCH = 4;                                // chunks of x = output tiles (C <= 64)
constexpr int pt_x_bytes(int nch) { return (nch * PT_PIX * 2 + 63) / 64 * 64 * 16; }      // whole DMA instructions (64 pieces of 16 bytes)
// the LDS plan of an instantiation: the 3x3's image (nch x 5 x nch fragments of 1 KB), then the staged x -- 45 + 31 = 76 KB at nch = 3,
// 80 + 41 = 121 KB at nch = 4
constexpr int PT_OFF_W3 = 0;
constexpr int pt_off_x(int nch) { return nch * PT_PAIRS * nch * 1024; }
constexpr int pt_lds(int nch) { return pt_off_x(nch) + pt_x_bytes(nch); }
static_assert(pt_lds(PT_MAXCH) <= LDS_LIMIT && pt_off_x(3) % 1024 == 0 && pt_off_x(4) % 1024 == 0, "LDS plan");

struct PtK {
    const char* x;            // NHWC 16-bit input of the 3x3
    const char* w3;           // esr_pack_conv_s16 blob of the 3x3 (C -> C over round_up(C, 16) physical channels)
    const char* wg;           // esr_pack_pa_gate blob of the gate's 1x1
    const char* s;            // NHWC skip (high parts of a pair), or NULL
    const char* s_lo;
    char* y;                  // NHWC result (high parts of a pair)
    char* y_lo;
    int N, H, W;
    int in_pitch, in_coff, s_pitch, s_coff, y_pitch, y_coff;
    int c;                    // logical channels
    int cout_store;           // channels stored (c .. cout_store - 1 as zeros)
    int tiles_x, tiles_y, ntiles;
};

// NCH: 16-channel chunks of x = 16-channel tiles of t (3: C 33..48, 4: 49..64)
template <bool BF16, int NCH>
__global__ __launch_bounds__(64 * PT_NW, 1) void pa_tail_kernel(const PtK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    constexpr int W3B = NCH * PT_PAIRS * NCH * 1024;       // bytes of the 3x3's weight image
    constexpr int PT_OFF_X = pt_off_x(NCH);                // the staged x lies behind it
    static_assert(PT_OFF_X == W3B, "LDS plan");

    // the 3x3's image into LDS, the gate's into registers: once per block
    for (int i = tid * 16; i < W3B; i += 64 * PT_NW * 16)
        *reinterpret_cast<i32x4*>(smem + PT_OFF_W3 + i) = *reinterpret_cast<const i32x4*>(p.w3 + i);
    i32x4 wh[NCH][2], wl[NCH][2];
    f32x4 bia3[NCH], biag[NCH];
    static_for<NCH>([&](auto m_) {
        constexpr int mt = decltype(m_)::value;
        static_for<2>([&](auto k_) {
            constexpr int ks = decltype(k_)::value;
            wh[mt][ks] = *reinterpret_cast<const i32x4*>(p.wg + ((mt * 2 + ks) * 64 + lane) * 16);
            wl[mt][ks] = *reinterpret_cast<const i32x4*>(p.wg + PA_IMG16 + ((mt * 2 + ks) * 64 + lane) * 16);
        });
        bia3[mt] = *reinterpret_cast<const f32x4*>(p.w3 + W3B + (mt * 16 + kq * 4) * 4);
        biag[mt] = *reinterpret_cast<const f32x4*>(p.wg + 2 * PA_IMG16 + (mt * 16 + kq * 4) * 4);
    });
    int laneoff[PT_PAIRS];                                 // pair q: tap min(2 q + (kq >> 1), 8), channel half kq & 1 (conv_s16_kernel's map)
    static_for<PT_PAIRS>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        const int tap = min(2 * q + (kq >> 1), 8);
        laneoff[q] = ((tap / 3) * PT_R + px + tap % 3) * 32 + (kq & 1) * 16;
    });

    const size_t img_bytes = (size_t)p.H * p.W * p.in_pitch * 2;
    const int cvalid8 = (p.c + 7) & ~7;                   // channels moved per pixel: whole 16-byte pieces up to round_up(C, 8)
    constexpr int ITEMS = NCH * PT_PIX * 2;               // 16-byte pieces of the staged input
    constexpr int NINST = (ITEMS + 63) / 64;

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * PT_T, x0 = (rem % p.tiles_x) * PT_T;

        // ---- x with a one-pixel halo: piece (chunk c, pixel, half h) -> LDS byte PT_OFF_X + c * PT_XCH + pixel * 32 + h * 16 ----------------------
        const i32x4 rs = make_rsrc(p.x + (size_t)n * img_bytes, img_bytes);
        for (int i = wv; i < NINST; i += PT_NW) {
            const int item = i * 64 + lane;
            const int c = item / (PT_PIX * 2), pr = item - c * (PT_PIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 1 + pix / PT_R, gx = x0 - 1 + pix % PT_R;
            const int ch = c * 16 + h * 8;
            const bool ok = item < ITEMS && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W && ch < cvalid8;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + ch) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(PT_OFF_X + i * 1024), voff, rs, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (p.c & 7) {
            // the last piece holds channels cvalid8 - 8 .. cvalid8 - 1, of which those >= C are pad slots of the tensor: zero
            const int cl = cvalid8 - 8, keep = p.c - cl;
            const int base = PT_OFF_X + (cl >> 4) * PT_XCH + ((cl >> 3) & 1) * 16;
            for (int pix = tid; pix < PT_PIX; pix += 64 * PT_NW) {
                i32x4 v = *reinterpret_cast<const i32x4*>(smem + base + pix * 32);
                v.x = keep >= 2 ? v.x : (keep == 1 ? (v.x & 0xffff) : 0);
                v.y = keep >= 4 ? v.y : (keep == 3 ? (v.y & 0xffff) : 0);
                v.z = keep >= 6 ? v.z : (keep == 5 ? (v.z & 0xffff) : 0);
                v.w = keep == 7 ? (v.w & 0xffff) : 0;
                *reinterpret_cast<i32x4*>(smem + base + pix * 32) = v;
            }
            __syncthreads();
        }

        // ---- t = conv3x3(x) + b3: four image rows of the tile per wave ------------------------------------------------------------------------------
        int bb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bb[j] = (wv * 4 + j) * PT_R * 32;
        f32x4 acc[4][NCH];
        static_for<NCH>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            static_for<PT_PAIRS>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                i32x4 b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const i32x4*>(smem + PT_OFF_X + c * PT_XCH + bb[j] + laneoff[q]);
                static_for<NCH>([&](auto t_) {
                    constexpr int tt = decltype(t_)::value;
                    const i32x4 a = *reinterpret_cast<const i32x4*>(smem + PT_OFF_W3 + ((c * PT_PAIRS + q) * NCH + tt) * 1024 + lane * 16);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j][tt] = mfma32<BF16>(a, b[j], (c == 0 && q == 0) ? bia3[tt] : acc[j][tt]);
                });
            });
        });

        // ---- y = t * sigmoid(W . rnd(t) + b) + s, row by row: the accumulators are the gate's operand layout --------------------------------------
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gy = y0 + wv * 4 + j, gx = x0 + px;
            const bool inside = gy < p.H && gx < p.W;
            const size_t pix = ((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0);
            unsigned raw[8];
            static_for<4>([&](auto m_) {
                constexpr int mt = decltype(m_)::value;
                if constexpr (mt < NCH) {
                    raw[2 * mt] = pack2<BF16>(acc[j][mt].x, acc[j][mt].y);
                    raw[2 * mt + 1] = pack2<BF16>(acc[j][mt].z, acc[j][mt].w);
                } else {
                    raw[2 * mt] = raw[2 * mt + 1] = 0u;
                }
            });
            const i32x4 b0 = {(int)raw[0], (int)raw[1], (int)raw[2], (int)raw[3]};
            const i32x4 b1 = {(int)raw[4], (int)raw[5], (int)raw[6], (int)raw[7]};
            const size_t so = (pix * p.s_pitch + p.s_coff) * 2, yo = (pix * p.y_pitch + p.y_coff) * 2;
            static_for<NCH>([&](auto m_) {
                constexpr int mt = decltype(m_)::value;
                const int cb = mt * 16 + kq * 4;
                f32x4 a = mfma32<BF16>(wh[mt][0], b0, biag[mt]);
                a = mfma32<BF16>(wh[mt][1], b1, a);
                a = mfma32<BF16>(wl[mt][0], b0, a);
                a = mfma32<BF16>(wl[mt][1], b1, a);
                const f32x4 tv = acc[j][mt];
                f32x4 v;
                v.x = __fmul_rn(tv.x, esr_sigmoid(a.x)); v.y = __fmul_rn(tv.y, esr_sigmoid(a.y));
                v.z = __fmul_rn(tv.z, esr_sigmoid(a.z)); v.w = __fmul_rn(tv.w, esr_sigmoid(a.w));
                if (p.s && inside && cb < cvalid8) {
                    f32x4 sv = unpack4<BF16>(*reinterpret_cast<const uint2*>(p.s + so + cb * 2));
                    if (p.s_lo) {
                        const f32x4 sl = unpack4<BF16>(*reinterpret_cast<const uint2*>(p.s_lo + so + cb * 2));
                        sv.x = __fadd_rn(sv.x, sl.x); sv.y = __fadd_rn(sv.y, sl.y); sv.z = __fadd_rn(sv.z, sl.z); sv.w = __fadd_rn(sv.w, sl.w);
                    }
                    v.x = __fadd_rn(v.x, sv.x); v.y = __fadd_rn(v.y, sv.y); v.z = __fadd_rn(v.z, sv.z); v.w = __fadd_rn(v.w, sv.w);
                }
                v.x = cb + 0 < p.c ? v.x : 0.f; v.y = cb + 1 < p.c ? v.y : 0.f;
                v.z = cb + 2 < p.c ? v.z : 0.f; v.w = cb + 3 < p.c ? v.w : 0.f;
                if (inside && cb < p.cout_store) {
                    uint2 hi;
                    hi.x = pack2<BF16>(v.x, v.y);
                    hi.y = pack2<BF16>(v.z, v.w);
                    *reinterpret_cast<uint2*>(p.y + yo + cb * 2) = hi;
                    if (p.y_lo) {
                        const f32x4 h = unpack4<BF16>(hi);
                        uint2 lo;
                        lo.x = pack2<BF16>(v.x - h.x, v.y - h.y);
                        lo.y = pack2<BF16>(v.z - h.z, v.w - h.w);
                        *reinterpret_cast<uint2*>(p.y_lo + yo + cb * 2) = lo;
                    }
                }
            });
        }
        __syncthreads();                                  // x is read: the next tile's DMA may overwrite it
    }
}

template <bool BF16, int NCH>
int launch_pa_tail(const PtK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&pa_tail_kernel<BF16, NCH>), pt_lds(NCH), "pa_tail_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (LDS), persistent over the tiles
    esr_note_kernel("pa_tail_kernel<%s, %d>", esr_tf(BF16), NCH);
    hipLaunchKernelGGL((pa_tail_kernel<BF16, NCH>), dim3(grid), dim3(64 * PT_NW), pt_lds(NCH), st, k);
    return esr_check_launch("pa_tail_kernel launch");
}

}  // namespace

extern "C" {

size_t esr_packed_pa_gate_bytes(int c, int storage)
{
    if (c <= 0 || c > PA_CMAX || storage < ESR_STORE_F32 || storage > ESR_STORE_F16) return 0;
    return (size_t)(esr_is_s16(storage) ? 2 * PA_IMG16 : PA_IMG32) + PA_CMAX * 4;
}

int esr_pack_pa_gate(const float* w_oi, const float* bias, int c, int storage, void* out, size_t out_bytes)
{
    const size_t need = esr_packed_pa_gate_bytes(c, storage);
    if (!w_oi || !out || !need || out_bytes < need) return ESR_ERR_BAD_ARG;
    memset(out, 0, need);
    char* o = static_cast<char*>(out);
    auto wt = [&](int row, int col) { return (row < c && col < c) ? w_oi[(size_t)row * c + col] : 0.f; };
    for (int mt = 0; mt < 4; ++mt)
        for (int lane = 0; lane < 64; ++lane) {
            const int row = mt * 16 + (lane & 15), kq = lane >> 4;
            if (esr_is_s16(storage)) {
                for (int ks = 0; ks < 2; ++ks)
                    for (int e = 0; e < 8; ++e) {
                        const float v = wt(row, (2 * ks + e / 4) * 16 + kq * 4 + e % 4);
                        const uint16_t hi = esr_host_to16(v, storage);
                        const uint16_t lo = esr_host_to16(v - esr_host_from16(hi, storage), storage);
                        const size_t at = ((size_t)((mt * 2 + ks) * 64 + lane) * 8 + e) * 2;
                        memcpy(o + at, &hi, 2);
                        memcpy(o + PA_IMG16 + at, &lo, 2);
                    }
            } else {
                for (int j = 0; j < 4; ++j)
                    for (int i = 0; i < 4; ++i) {
                        const float v = wt(row, j * 16 + kq * 4 + i);
                        memcpy(o + ((size_t)(mt * 16 + j * 4 + i) * 64 + lane) * 4, &v, 4);
                    }
            }
        }
    float* b = reinterpret_cast<float*>(o + (esr_is_s16(storage) ? 2 * PA_IMG16 : PA_IMG32));
    for (int i = 0; i < c; ++i) b[i] = bias ? bias[i] : 0.f;
    return ESR_OK;
}

int esr_pa_gate_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (d->storage != ESR_STORE_F32 && !esr_is_s16(d->storage)) return 0;
    if (d->compute != d->storage) return 0;
    const int gran = esr_is_s16(d->storage) ? 8 : 4;
    if (d->ksize != 1 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->cin <= 32 || d->cin > PA_CMAX) return 0;
    if ((d->cout & (gran - 1)) || d->cout < d->cin || d->cout > esr_round_up(d->cin, 16)) return 0;
    if (d->act != ESR_ACT_NONE || (d->res_mode != ESR_RES_NONE && d->res_mode != ESR_RES_POST_ACT)) return 0;
    if (d->split || d->tail_wpacked || d->tail_cat.ptr || d->tail_cat_c || d->post_wpacked || d->post2_wpacked || d->border_bias || d->blocked8 || d->in_seg_stride || d->wino_wpacked) return 0;
    if (d->hilo & ~(ESR_HILO_RES | ESR_HILO_OUT)) return 0;
    if (d->hilo && (!esr_is_s16(d->storage) || d->hilo_stride <= 0 || (d->hilo_stride & 15))) return 0;
    if ((d->hilo & ESR_HILO_RES) && d->res_mode == ESR_RES_NONE) return 0;
    if ((double)d->n * d->h * d->w >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_pa_gate(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_pa_gate_supported(d)) return ESR_ERR_UNSUPPORTED;
    const bool s16 = esr_is_s16(d->storage);
    const int gran = s16 ? 8 : 4, cp = esr_round_up(d->cin, gran);
    const bool has_s = d->res_mode != ESR_RES_NONE;
    if (has_s && !d->res.ptr) return ESR_ERR_BAD_ARG;
    if (!esr_view_fits(d->in, gran, cp) || !esr_view_fits(d->out0, gran, d->cout) || (has_s && !esr_view_fits(d->res, gran, cp))) return ESR_ERR_BAD_ARG;
    PaK k;
    memset(&k, 0, sizeof(k));
    k.t = static_cast<const char*>(d->in.ptr);
    k.s = has_s ? static_cast<const char*>(d->res.ptr) : nullptr;
    k.s_lo = (has_s && (d->hilo & ESR_HILO_RES)) ? k.s + d->hilo_stride : nullptr;
    k.y = static_cast<char*>(d->out0.ptr);
    k.y_lo = (d->hilo & ESR_HILO_OUT) ? k.y + d->hilo_stride : nullptr;
    // y's bytes meet neither t's nor s's (low parts included): the op is not specified in place
    const size_t es = s16 ? 2 : 4, npx = (size_t)d->n * d->h * d->w;
    const size_t in_n[3] = {npx * d->in.pitch * es, npx * d->res.pitch * es, npx * d->res.pitch * es}, out_n = npx * d->out0.pitch * es;
    const char* ins[3] = {k.t, k.s, k.s_lo};
    const char* outs[2] = {k.y, k.y_lo};
    for (const char* o : outs)
        for (int i = 0; i < 3; ++i)
            if (esr_bytes_overlap(o, out_n, ins[i], in_n[i])) return ESR_ERR_BAD_ARG;
    k.w = static_cast<const char*>(d->wpacked);
    k.npix = (long long)d->n * d->h * d->w;
    k.ngroups = (int)((k.npix + 15) / 16);
    k.t_pitch = d->in.pitch; k.t_coff = d->in.coff;
    k.s_pitch = d->res.pitch; k.s_coff = d->res.coff;
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    k.c = d->cin; k.cp = cp; k.cout_store = d->cout;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (d->storage == ESR_STORE_BF16) return launch_pa_gate<ESR_STORE_BF16>(k, st);
    if (d->storage == ESR_STORE_F16) return launch_pa_gate<ESR_STORE_F16>(k, st);
    return launch_pa_gate<ESR_STORE_F32>(k, st);
}

int esr_pa_tail_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->ksize != 3 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->cin <= 32 || d->cin > PA_CMAX) return 0;
    if ((d->cout & 7) || d->cout < d->cin || d->cout > esr_round_up(d->cin, 16)) return 0;
    if (d->act != ESR_ACT_NONE || (d->res_mode != ESR_RES_NONE && d->res_mode != ESR_RES_POST_ACT)) return 0;
    if (d->split || d->tail_cat.ptr || d->tail_cat_c || d->post_wpacked || d->post2_wpacked || d->border_bias || d->blocked8 || d->in_seg_stride || d->wino_wpacked) return 0;
    if (d->hilo & ~(ESR_HILO_RES | ESR_HILO_OUT)) return 0;
    if (d->hilo && (d->hilo_stride <= 0 || (d->hilo_stride & 15))) return 0;
    if ((d->hilo & ESR_HILO_RES) && d->res_mode == ESR_RES_NONE) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, PT_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_pa_tail(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->wpacked || !d->tail_wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_pa_tail_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int cp = esr_round_up(d->cin, 8);
    const bool has_s = d->res_mode != ESR_RES_NONE;
    if (has_s && !d->res.ptr) return ESR_ERR_BAD_ARG;
    if (!esr_view_fits(d->in, 8, cp) || !esr_view_fits(d->out0, 8, d->cout) || (has_s && !esr_view_fits(d->res, 8, cp))) return ESR_ERR_BAD_ARG;
    PtK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.s = has_s ? static_cast<const char*>(d->res.ptr) : nullptr;
    k.s_lo = (has_s && (d->hilo & ESR_HILO_RES)) ? k.s + d->hilo_stride : nullptr;
    k.y = static_cast<char*>(d->out0.ptr);
    k.y_lo = (d->hilo & ESR_HILO_OUT) ? k.y + d->hilo_stride : nullptr;
    // y's bytes meet neither x's (neighbouring tiles read its halo) nor s's
    const size_t npx = (size_t)d->n * d->h * d->w;
    const size_t in_n[3] = {npx * d->in.pitch * 2, npx * d->res.pitch * 2, npx * d->res.pitch * 2}, out_n = npx * d->out0.pitch * 2;
    const char* ins[3] = {k.x, k.s, k.s_lo};
    const char* outs[2] = {k.y, k.y_lo};
    for (const char* o : outs)
        for (int i = 0; i < 3; ++i)
            if (esr_bytes_overlap(o, out_n, ins[i], in_n[i])) return ESR_ERR_BAD_ARG;
    k.w3 = static_cast<const char*>(d->wpacked);
    k.wg = static_cast<const char*>(d->tail_wpacked);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.s_pitch = d->res.pitch; k.s_coff = d->res.coff;
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    k.c = d->cin; k.cout_store = d->cout;
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, PT_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const bool bf16 = d->storage == ESR_STORE_BF16;
    if (d->cin > 48) return bf16 ? launch_pa_tail<true, 4>(k, st) : launch_pa_tail<false, 4>(k, st);
    return bf16 ? launch_pa_tail<true, 3>(k, st) : launch_pa_tail<false, 3>(k, st);
}

}  // extern "C"
