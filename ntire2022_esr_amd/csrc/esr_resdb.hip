// esr_resdb.hip -- ResDN's block (models/team43_resdn.py:48-111): its per-channel PReLU as a streaming op in every storage (esr_prelu,
// prelu_kernel: this comment), and one whole step of the block as ONE launch on 16-bit storage (esr_resdb_step, resdb_step_kernel: the
// comment in front of it, further down), which applies the same PReLU where it loads its matrix operands.
//
// Every convolution of a ResDB is PRE-activated by an nn.PReLU with one slope per channel, and the raw tensor is still needed (the residual,
// later layers with slopes of their own): the activation belongs to the consumer, not to a producer's epilogue.  esr_prelu is that consumer
// side as ONE launch per layer: it gathers up to four NHWC source views (the torch.cat in front of the expansion 1x1s never runs) into one
// dense tensor,
//
//     out[c] = store(in[c] >= 0 ? in[c] : a[c] * in[c])            c over the sources' channels, one behind the other
//
// The checkpoint's slopes span -1.82 .. +3.62 (352 of 1 728 negative, 89 above 1), so the kernels' usual max(v, slope v) is NOT this function:
// it is for 0 <= a <= 1 only.  Slopes are fp32.  A non-negative value passes through bit for bit (-0 included); the product of a negative one is
// rounded ONCE to the storage type (fp64 -> fp32 -> 16-bit would round twice): prelu16 rounds the product to odd in fp32 with one fma's exact
// residual and lets the conversion round that to nearest even; tiny products take fp64, where a 16-bit value times an fp32 slope is exact
// (11 + 24 bits) and prelu_round16 rounds it to nearest even itself.  fp32 storage: one fp32 multiplication.
// The output's pad slots up to the 16-byte granule are written as zeros, nothing behind them; a source's pad slots are never read into the
// output: where every source's channel count is whole granules a thread moves one 16-byte piece (VEC), else it gathers its channels one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_internal.h"
#include "esr_s16_dev.h"

namespace {

constexpr int PR_MAXSRC = 4;
constexpr int PR_THREADS = 256;
constexpr int PR_MAX_BLOCKS = 16384;

struct PreluK {
    const char* src[PR_MAXSRC];
    int pitch[PR_MAXSRC], coff[PR_MAXSRC];
    int cend[PR_MAXSRC];      // first output channel BEHIND source s (cend[nsrc - 1] == ctot); sources beyond nsrc: ctot
    const float* a;           // ctot slopes
    char* y;
    int y_pitch, y_coff;
    int ctot, cstore;         // channels, channels written (round_up(ctot, granule))
    long long npix;
};

// (prelu_round16 -- fp64 -> 16-bit with ONE rounding -- lives in esr_s16_dev.h: esr_mdsa.hip's epilogue rounds its products the same way)
template <int ST>
__device__ __forceinline__ unsigned prelu16(unsigned bits, float a)
{
    float v;
    if (ST == ESR_STORE_BF16) {
        v = __builtin_bit_cast(float, bits << 16);
    } else {
        v = (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
    }
    if (v >= 0.f) return bits;                             // bit for bit
    // One rounding without fp64 on the common path: p = RN(a v) and the exact residual e = a v - p (one fma) give the product ROUNDED TO ODD
    // in fp32 -- of the two fp32 neighbours of an inexact product the one with an odd significand --, and rounding that to nearest even
    // into a type with at least two bits less (8 or 11 of 24) equals rounding the exact product once.  The residual is exact while the
    // product's 35 bits lie above 2^-149: for |p| >= 2^-100; below that (and for a NaN or an Inf) the fp64 path takes over.
    const float p = a * v;
    const float ap = fabsf(p);
    if (!(ap >= 0x1p-100f && ap < __builtin_inff())) {
        const double pd = (double)a * (double)v;           // exact
        return ST == ESR_STORE_BF16 ? prelu_round16<7, 8>(pd) : prelu_round16<10, 5>(pd);
    }
    const float e = fmaf(a, v, -p);
    unsigned pb = __builtin_bit_cast(unsigned, p);
    if (e != 0.f) {
        if ((e < 0.f) == (p > 0.f)) pb -= 1u;              // the exact product lies below |p|: its truncation is p's predecessor
        pb |= 1u;
    }
    const float po = __builtin_bit_cast(float, pb);
    if (ST == ESR_STORE_BF16) return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)po);
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)po);
}

__device__ __forceinline__ float prelu32(float v, float a) { return v >= 0.f ? v : a * v; }

// the source of output channel c and the channel's element offset inside a pixel of it
__device__ __forceinline__ int prelu_source(const PreluK& p, int c, int& ch)
{
    int s = 0, c0 = 0;
#pragma unroll
    for (int i = 0; i < PR_MAXSRC - 1; ++i)
        if (c >= p.cend[i]) { s = i + 1; c0 = p.cend[i]; }
    ch = p.coff[s] + (c - c0);
    return s;
}

// ST: esr_storage; VEC: every source's channel count is whole granules (a granule never spans two sources, none holds a pad slot)
template <int ST, bool VEC>
__global__ __launch_bounds__(PR_THREADS) void prelu_kernel(const PreluK p)
{
    constexpr int G = ST == ESR_STORE_F32 ? 4 : 8;         // channels per 16-byte granule
    constexpr int ES = 16 / G;
    const int ng = p.cstore / G;
    const long long total = p.npix * ng;
    for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PR_THREADS) {
        const long long pix = i / ng;
        const int c = (int)(i - pix * ng) * G;
        uint4 out;
        if (VEC) {
            int ch;
            const int s = prelu_source(p, c, ch);
            const uint4 in = *reinterpret_cast<const uint4*>(p.src[s] + ((size_t)pix * p.pitch[s] + ch) * ES);
            const float4 a0 = *reinterpret_cast<const float4*>(p.a + c);
            if (ST == ESR_STORE_F32) {
                out.x = __builtin_bit_cast(unsigned, prelu32(__builtin_bit_cast(float, in.x), a0.x));
                out.y = __builtin_bit_cast(unsigned, prelu32(__builtin_bit_cast(float, in.y), a0.y));
                out.z = __builtin_bit_cast(unsigned, prelu32(__builtin_bit_cast(float, in.z), a0.z));
                out.w = __builtin_bit_cast(unsigned, prelu32(__builtin_bit_cast(float, in.w), a0.w));
            } else {
                const float4 a1 = *reinterpret_cast<const float4*>(p.a + c + 4);
                out.x = prelu16<ST>(in.x & 0xffffu, a0.x) | (prelu16<ST>(in.x >> 16, a0.y) << 16);
                out.y = prelu16<ST>(in.y & 0xffffu, a0.z) | (prelu16<ST>(in.y >> 16, a0.w) << 16);
                out.z = prelu16<ST>(in.z & 0xffffu, a1.x) | (prelu16<ST>(in.z >> 16, a1.y) << 16);
                out.w = prelu16<ST>(in.w & 0xffffu, a1.z) | (prelu16<ST>(in.w >> 16, a1.w) << 16);
            }
        } else {
            unsigned e[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                e[j] = 0u;                                 // the output's pad slots: zeros
                if (c + j < p.ctot) {
                    int ch;
                    const int s = prelu_source(p, c + j, ch);
                    const char* at = p.src[s] + ((size_t)pix * p.pitch[s] + ch) * ES;
                    const float a = p.a[c + j];
                    if (ST == ESR_STORE_F32) e[j] = __builtin_bit_cast(unsigned, prelu32(*reinterpret_cast<const float*>(at), a));
                    else e[j] = prelu16<ST>(*reinterpret_cast<const unsigned short*>(at), a);
                }
            }
            if (ST == ESR_STORE_F32) {
                out.x = e[0]; out.y = e[1]; out.z = e[2]; out.w = e[3];
            } else {
                out.x = e[0] | (e[1 % G] << 16); out.y = e[2 % G] | (e[3 % G] << 16);
                out.z = e[4 % G] | (e[5 % G] << 16); out.w = e[6 % G] | (e[7 % G] << 16);
            }
        }
        *reinterpret_cast<uint4*>(p.y + ((size_t)pix * p.y_pitch + p.y_coff + c) * ES) = out;
    }
}

template <int ST, bool VEC>
int launch_prelu(const PreluK& k, hipStream_t st)
{
    const long long total = k.npix * (k.cstore / (ST == ESR_STORE_F32 ? 4 : 8));
    const long long blocks = (total + PR_THREADS - 1) / PR_THREADS;
    esr_note_kernel("prelu_kernel<%d, %s>", ST, esr_tf(VEC));
    hipLaunchKernelGGL((prelu_kernel<ST, VEC>), dim3((unsigned)(blocks < PR_MAX_BLOCKS ? blocks : PR_MAX_BLOCKS)), dim3(PR_THREADS), 0, st, k);
    return esr_check_launch("prelu_kernel launch");
}

inline int pr_granule(int storage) { return storage == ESR_STORE_F32 ? 4 : 8; }

// the sources of a descriptor in order: (view, channels); a count of zero ends the list (the predicate does not look at pointers)
int pr_sources(const esr_conv_desc* d, const esr_view* v[PR_MAXSRC], int c[PR_MAXSRC])
{
    const esr_view* views[PR_MAXSRC] = {&d->in, &d->res, &d->tail_cat, &d->out1};
    const int counts[PR_MAXSRC] = {d->cin, d->split, d->tail_cat_c, d->tail_cout};
    int n = 0;
    while (n < PR_MAXSRC && counts[n] > 0) { v[n] = views[n]; c[n] = counts[n]; ++n; }
    for (int i = n; i < PR_MAXSRC; ++i)
        if (views[i]->ptr || counts[i] != 0) return -1;   // a source behind a gap
    return n;
}

// ---- esr_resdb_step: one ResDB step (team43_resdn.py:93-106) as ONE launch on 16-bit storage ---------------------------------------------------
//
//     u = (prelu(in, a_e))~          in = cat(x, e0, e1): 48 + 16 NX channels             e = W_e . u + b_e (fp32)
//     dists = e[48:]~  (stored)      r = e[:48]~     t = (prelu(r, a_c))~, and t = 0 outside the image (the 3x3's zero padding, not prelu(b_e))
//     y = (x + W_c (*) t + b_c)~     (stored)
//
// `~`: rounded once (RNE) to the storage type, as a stored tensor holds it.  A block owns one 16 x 16 output tile at a time (persistent over
// the tiles).  LDS, all as [16-channel chunk][pixel][32 B] (conv_s16_kernel's stage layout: a B fragment is 16 B of one pixel):
//     in  18 x 18 pixels, RAW, staged once with a one-pixel halo (zeros outside the image); the PReLU is applied where a B fragment is
//         loaded -- the consumer's operand load -- once per (pixel group, chunk) for all output tiles; x's centre is the residual
//     t   18 x 18: the 1x1's `res` rows on every staged pixel (21 groups of 16), rounded, activated, rounded
// and both weight images as esr_pack_conv_s16 lays them out -- the 1x1's [hi | lo] K pairs as the stand-alone launch multiplies by them, the
// 3x3's tap pairs with its diffused rounding -- (30 + 45 KB), biases and slopes.  The distilled rows run on the tile's own pixels only.
constexpr int RS_T = 16, RS_R = 18, RS_PIX = RS_R * RS_R, RS_NW = 4;
constexpr int RS_XCH = RS_PIX * 32;                        // bytes of one staged 16-channel chunk
constexpr int RS_GROUPS = (RS_PIX + 15) / 16;              // pixel groups of the staged region (the last one partial)
constexpr int RS_OFF_W1 = 0;                               // up to 5 chunks x 6 output tiles
constexpr int RS_OFF_W3 = RS_OFF_W1 + 5 * 6 * 1024;        // 3 chunks x 5 tap pairs x 3 output tiles
constexpr int RS_OFF_X = RS_OFF_W3 + 3 * 5 * 3 * 1024;
constexpr int RS_OFF_T = RS_OFF_X + 5 * RS_XCH;
constexpr int RS_OFF_BE = RS_OFF_T + 3 * RS_XCH;           // 96 fp32
constexpr int RS_OFF_BC = RS_OFF_BE + 96 * 4;              // 48 fp32
constexpr int RS_OFF_AE = RS_OFF_BC + 48 * 4;              // 80 fp32
constexpr int RS_OFF_AC = RS_OFF_AE + 80 * 4;              // 48 fp32
constexpr int RS_LDS = RS_OFF_AC + 48 * 4;
static_assert(RS_LDS <= LDS_LIMIT && RS_OFF_X % 16 == 0 && RS_OFF_T % 16 == 0 && RS_OFF_BE % 16 == 0, "LDS plan");

struct ResdbK {
    const char* x;            // the step's running x (48 channels), then the earlier distilled maps it reads next to it (16 each)
    const char* e0;
    const char* e1;
    const char* w1;           // esr_pack_conv_s16 blob of the expansion 1x1 (48 + 16 NX -> 48 + 16 ND)
    const char* w3;           // esr_pack_conv_s16 blob of the compression 3x3 (48 -> 48)
    const float* a;           // esr_pack_prelu blob: a_e (48 + 16 NX), then a_c (48)
    char* d;                  // the step's distilled maps (16 ND channels)
    char* y;
    int N, H, W;
    int x_pitch, x_coff, e0_pitch, e0_coff, e1_pitch, e1_coff, d_pitch, d_coff, y_pitch, y_coff;
    int tiles_x, tiles_y, ntiles;
};

template <int ST>
__device__ __forceinline__ i32x4 rs_prelu8(i32x4 v, const float* a)
{
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + 4);
    i32x4 o;
    o.x = (int)(prelu16<ST>((unsigned)v.x & 0xffffu, a0.x) | (prelu16<ST>((unsigned)v.x >> 16, a0.y) << 16));
    o.y = (int)(prelu16<ST>((unsigned)v.y & 0xffffu, a0.z) | (prelu16<ST>((unsigned)v.y >> 16, a0.w) << 16));
    o.z = (int)(prelu16<ST>((unsigned)v.z & 0xffffu, a1.x) | (prelu16<ST>((unsigned)v.z >> 16, a1.y) << 16));
    o.w = (int)(prelu16<ST>((unsigned)v.w & 0xffffu, a1.z) | (prelu16<ST>((unsigned)v.w >> 16, a1.w) << 16));
    return o;
}

// NX: extra inputs (0..2), ND: distilled outputs (1..3)
template <bool BF16, int NX, int ND>
__global__ __launch_bounds__(64 * RS_NW, 1) void resdb_step_kernel(const ResdbK p)
{
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    constexpr int ST = BF16 ? ESR_STORE_BF16 : ESR_STORE_F16;
    constexpr int NCH = 3 + NX, NT1 = 3 + ND;
    constexpr int W1B = NCH * NT1 * 1024, W3B = 3 * 5 * 3 * 1024;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;

    // weights, biases and slopes into LDS: once per block
    for (int i = tid * 16; i < W1B; i += 64 * RS_NW * 16)
        *reinterpret_cast<i32x4*>(smem + RS_OFF_W1 + i) = *reinterpret_cast<const i32x4*>(p.w1 + i);
    for (int i = tid * 16; i < W3B; i += 64 * RS_NW * 16)
        *reinterpret_cast<i32x4*>(smem + RS_OFF_W3 + i) = *reinterpret_cast<const i32x4*>(p.w3 + i);
    for (int i = tid; i < NT1 * 16; i += 64 * RS_NW) reinterpret_cast<float*>(smem + RS_OFF_BE)[i] = reinterpret_cast<const float*>(p.w1 + W1B)[i];
    for (int i = tid; i < 48; i += 64 * RS_NW) reinterpret_cast<float*>(smem + RS_OFF_BC)[i] = reinterpret_cast<const float*>(p.w3 + W3B)[i];
    for (int i = tid; i < NCH * 16; i += 64 * RS_NW) reinterpret_cast<float*>(smem + RS_OFF_AE)[i] = p.a[i];
    for (int i = tid; i < 48; i += 64 * RS_NW) reinterpret_cast<float*>(smem + RS_OFF_AC)[i] = p.a[NCH * 16 + i];
    const float* const be = reinterpret_cast<const float*>(smem + RS_OFF_BE);
    const float* const bc = reinterpret_cast<const float*>(smem + RS_OFF_BC);
    const float* const ae = reinterpret_cast<const float*>(smem + RS_OFF_AE);
    const float* const ac = reinterpret_cast<const float*>(smem + RS_OFF_AC);

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * RS_T, x0 = (rem % p.tiles_x) * RS_T;
        __syncthreads();                                  // the previous tile's readers are done (and the weights are in place)

        // ---- in with a one-pixel halo: piece (chunk c, pixel, half h) -> LDS byte RS_OFF_X + c * RS_XCH + pixel * 32 + h * 16 ----------------
        for (int item = tid; item < NCH * RS_PIX * 2; item += 64 * RS_NW) {
            const int c = item / (RS_PIX * 2), pr = item - c * (RS_PIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 1 + pix / RS_R, gx = x0 - 1 + pix % RS_R;
            i32x4 v = {0, 0, 0, 0};
            if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
                const size_t pixel = ((size_t)n * p.H + gy) * p.W + gx;
                const char* src = c < 3 ? p.x + (pixel * p.x_pitch + p.x_coff + c * 16 + h * 8) * 2
                                : c == 3 ? p.e0 + (pixel * p.e0_pitch + p.e0_coff + h * 8) * 2
                                         : p.e1 + (pixel * p.e1_pitch + p.e1_coff + h * 8) * 2;
                v = *reinterpret_cast<const i32x4*>(src);
            }
            *reinterpret_cast<i32x4*>(smem + RS_OFF_X + c * RS_XCH + pix * 32 + h * 16) = v;
        }
        __syncthreads();

        // ---- t on the staged 18 x 18 pixels: groups of 16 pixels in staged order -------------------------------------------------------
        for (int g = wv; g < RS_GROUPS; g += RS_NW) {
            const int pq = g * 16 + px;
            const int pc = pq < RS_PIX ? pq : RS_PIX - 1;
            f32x4 acc[3];
            static_for<3>([&](auto o_) { constexpr int o = decltype(o_)::value; acc[o] = *reinterpret_cast<const f32x4*>(be + o * 16 + kq * 4); });
            static_for<NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                const i32x4 raw = *reinterpret_cast<const i32x4*>(smem + RS_OFF_X + c * RS_XCH + pc * 32 + (kq & 1) * 16);
                const i32x4 b = rs_prelu8<ST>(raw, ae + c * 16 + (kq & 1) * 8);
                static_for<3>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    const i32x4 a = *reinterpret_cast<const i32x4*>(smem + RS_OFF_W1 + (c * NT1 + o) * 1024 + lane * 16);
                    acc[o] = mfma32<BF16>(a, b, acc[o]);
                });
            });
            const int gy = y0 - 1 + pc / RS_R, gx = x0 - 1 + pc % RS_R;
            const bool inside = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            static_for<3>([&](auto o_) {
                constexpr int o = decltype(o_)::value;
                const unsigned r0 = pack2<BF16>(acc[o].x, acc[o].y), r1 = pack2<BF16>(acc[o].z, acc[o].w);
                const f32x4 s = *reinterpret_cast<const f32x4*>(ac + o * 16 + kq * 4);
                uint2 tk;
                tk.x = prelu16<ST>(r0 & 0xffffu, s.x) | (prelu16<ST>(r0 >> 16, s.y) << 16);
                tk.y = prelu16<ST>(r1 & 0xffffu, s.z) | (prelu16<ST>(r1 >> 16, s.w) << 16);
                if (!inside) tk = make_uint2(0u, 0u);
                if (pq < RS_PIX) *reinterpret_cast<uint2*>(smem + RS_OFF_T + o * RS_XCH + pq * 32 + kq * 8) = tk;
            });
        }
        // ---- the distilled rows on the tile's own pixels: one image row of the tile per job --------------------------------------------
        for (int row = wv; row < RS_T; row += RS_NW) {
            const int pc = (row + 1) * RS_R + px + 1;
            f32x4 acc[ND];
            static_for<ND>([&](auto o_) { constexpr int o = decltype(o_)::value; acc[o] = *reinterpret_cast<const f32x4*>(be + (3 + o) * 16 + kq * 4); });
            static_for<NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                const i32x4 raw = *reinterpret_cast<const i32x4*>(smem + RS_OFF_X + c * RS_XCH + pc * 32 + (kq & 1) * 16);
                const i32x4 b = rs_prelu8<ST>(raw, ae + c * 16 + (kq & 1) * 8);
                static_for<ND>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    const i32x4 a = *reinterpret_cast<const i32x4*>(smem + RS_OFF_W1 + (c * NT1 + 3 + o) * 1024 + lane * 16);
                    acc[o] = mfma32<BF16>(a, b, acc[o]);
                });
            });
            const int gy = y0 + row, gx = x0 + px;
            if (gy < p.H && gx < p.W) {
                char* const dp = p.d + ((((size_t)n * p.H + gy) * p.W + gx) * p.d_pitch + p.d_coff) * 2;
                static_for<ND>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    uint2 pk;
                    pk.x = pack2<BF16>(acc[o].x, acc[o].y);
                    pk.y = pack2<BF16>(acc[o].z, acc[o].w);
                    *reinterpret_cast<uint2*>(dp + (o * 16 + kq * 4) * 2) = pk;
                });
            }
        }
        __syncthreads();                                  // t is complete

        // ---- y = x + W_c (*) t + b_c: K = 32 is a tap pair x the chunk's 16 channels (the tenth tap's weights are zeros) ----------------
        for (int row = wv; row < RS_T; row += RS_NW) {
            f32x4 acc[3];
            static_for<3>([&](auto o_) { constexpr int o = decltype(o_)::value; acc[o] = *reinterpret_cast<const f32x4*>(bc + o * 16 + kq * 4); });
            static_for<3>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                static_for<5>([&](auto q_) {
                    constexpr int q = decltype(q_)::value;
                    int tap = 2 * q + (kq >> 1);
                    tap = tap > 8 ? 8 : tap;
                    const int pix = (row + tap / 3) * RS_R + px + tap % 3;
                    const i32x4 b = *reinterpret_cast<const i32x4*>(smem + RS_OFF_T + c * RS_XCH + pix * 32 + (kq & 1) * 16);
                    static_for<3>([&](auto o_) {
                        constexpr int o = decltype(o_)::value;
                        const i32x4 a = *reinterpret_cast<const i32x4*>(smem + RS_OFF_W3 + ((c * 5 + q) * 3 + o) * 1024 + lane * 16);
                        acc[o] = mfma32<BF16>(a, b, acc[o]);
                    });
                });
            });
            const int gy = y0 + row, gx = x0 + px;
            if (gy < p.H && gx < p.W) {
                char* const yp = p.y + ((((size_t)n * p.H + gy) * p.W + gx) * p.y_pitch + p.y_coff) * 2;
                const int pc = (row + 1) * RS_R + px + 1;
                static_for<3>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    const f32x4 xr = unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + RS_OFF_X + o * RS_XCH + pc * 32 + kq * 8));
                    uint2 pk;
                    pk.x = pack2<BF16>(acc[o].x + xr.x, acc[o].y + xr.y);
                    pk.y = pack2<BF16>(acc[o].z + xr.z, acc[o].w + xr.w);
                    *reinterpret_cast<uint2*>(yp + (o * 16 + kq * 4) * 2) = pk;
                });
            }
        }
    }
}

template <bool BF16, int NX, int ND>
int launch_resdb(const ResdbK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&resdb_step_kernel<BF16, NX, ND>), RS_LDS, "resdb_step_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (LDS), persistent over the tiles
    esr_note_kernel("resdb_step_kernel<%s, %d, %d>", esr_tf(BF16), NX, ND);
    hipLaunchKernelGGL((resdb_step_kernel<BF16, NX, ND>), dim3(grid), dim3(64 * RS_NW), RS_LDS, st, k);
    return esr_check_launch("resdb_step_kernel launch");
}

template <bool BF16, int NX>
int launch_resdb_nd(const ResdbK& k, int nd, hipStream_t st)
{
    return nd == 1 ? launch_resdb<BF16, NX, 1>(k, st) : nd == 2 ? launch_resdb<BF16, NX, 2>(k, st) : launch_resdb<BF16, NX, 3>(k, st);
}

template <bool BF16>
int launch_resdb_nx(const ResdbK& k, int nx, int nd, hipStream_t st)
{
    return nx == 0 ? launch_resdb_nd<BF16, 0>(k, nd, st) : nx == 1 ? launch_resdb_nd<BF16, 1>(k, nd, st) : launch_resdb_nd<BF16, 2>(k, nd, st);
}

}  // namespace

extern "C" {

size_t esr_packed_prelu_bytes(int c)
{
    if (c < 1 || c > 512) return 0;
    return (size_t)esr_round_up(c, 8) * 4;
}

// nn.PReLU(c).weight [c] (or the slopes of several, one behind the other) -> c fp32 slopes, zeros up to round_up(c, 8)
int esr_pack_prelu(const float* slopes, int c, void* out, size_t out_bytes)
{
    const size_t need = esr_packed_prelu_bytes(c);
    if (!slopes || !out || !need || out_bytes < need) return ESR_ERR_BAD_ARG;
    memset(out, 0, need);
    memcpy(out, slopes, (size_t)c * 4);
    return ESR_OK;
}

int esr_unpack_prelu(const void* packed, size_t packed_bytes, int c, float* slopes)
{
    const size_t need = esr_packed_prelu_bytes(c);
    if (!packed || !slopes || !need || packed_bytes < need) return ESR_ERR_BAD_ARG;
    memcpy(slopes, packed, (size_t)c * 4);
    return ESR_OK;
}

int esr_prelu_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (d->storage != ESR_STORE_F32 && d->storage != ESR_STORE_BF16 && d->storage != ESR_STORE_F16) return 0;
    if (d->compute != d->storage) return 0;
    if (d->ksize != 1 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->act != ESR_ACT_NONE || d->res_mode != ESR_RES_NONE) return 0;
    const esr_view* v[PR_MAXSRC];
    int c[PR_MAXSRC];
    const int n = pr_sources(d, v, c);
    if (n < 1) return 0;
    int ctot = 0;
    for (int i = 0; i < n; ++i) ctot += c[i];
    if (d->cout != ctot || ctot > 512) return 0;
    if (d->tail_wpacked || d->tail_mid_act || d->tail_seg_stride16 || d->post_wpacked || d->post_out.ptr || d->post_cout || d->post_act || d->post2_wpacked ||
        d->post2_out.ptr || d->post2_cout || d->border_bias || d->blocked8 || d->in_seg_stride || d->in_seg_chunks || d->wino_wpacked || d->hilo || d->hilo_stride) return 0;
    return 1;
}

int esr_prelu(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_prelu_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int g = pr_granule(d->storage), es = 16 / g;
    const esr_view* v[PR_MAXSRC];
    int c[PR_MAXSRC];
    const int n = pr_sources(d, v, c);
    const int cstore = esr_round_up(d->cout, g);
    if (!esr_view_fits(d->out0, g, cstore)) return ESR_ERR_BAD_ARG;
    const size_t npx = (size_t)d->n * d->h * d->w;
    bool vec = true;
    for (int i = 0; i < n; ++i) {
        if (!v[i]->ptr || !esr_view_fits(*v[i], g, c[i])) return ESR_ERR_BAD_ARG;           // (only the c[i] channels are read: never a pad slot)
        if (esr_views_meet(d->out0, cstore, *v[i], c[i], npx, es)) return ESR_ERR_BAD_ARG;
        vec = vec && c[i] % g == 0;
    }
    PreluK k;
    memset(&k, 0, sizeof(k));
    int end = 0;
    for (int i = 0; i < PR_MAXSRC; ++i) {
        if (i < n) {
            k.src[i] = static_cast<const char*>(v[i]->ptr);
            k.pitch[i] = v[i]->pitch; k.coff[i] = v[i]->coff;
            end += c[i];
        } else {
            k.src[i] = k.src[0];
        }
        k.cend[i] = end;
    }
    k.a = static_cast<const float*>(d->wpacked);
    k.y = static_cast<char*>(d->out0.ptr);
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    k.ctot = d->cout; k.cstore = cstore;
    k.npix = (long long)npx;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    switch (d->storage) {
        case ESR_STORE_F32: return vec ? launch_prelu<ESR_STORE_F32, true>(k, st) : launch_prelu<ESR_STORE_F32, false>(k, st);
        case ESR_STORE_BF16: return vec ? launch_prelu<ESR_STORE_BF16, true>(k, st) : launch_prelu<ESR_STORE_BF16, false>(k, st);
        default: return vec ? launch_prelu<ESR_STORE_F16, true>(k, st) : launch_prelu<ESR_STORE_F16, false>(k, st);
    }
}

/* d = 16: how many distilled outputs / extra inputs a descriptor asks for, or -1 */
static int rs_count16(int channels, int lo, int hi)
{
    return (channels % 16 == 0 && channels / 16 >= lo && channels / 16 <= hi) ? channels / 16 : -1;
}

int esr_resdb_step_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->ksize != 3 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    if (d->cin != 48 || d->cout != 48) return 0;                                                  // n = 48
    if (rs_count16(d->post_cout, 1, 3) < 0 || rs_count16(d->tail_cat_c, 0, 2) < 0) return 0;        // d = 16: 1..3 distilled outputs, 0..2 extra inputs
    if (d->act != ESR_ACT_NONE || d->post_act != ESR_ACT_NONE || d->res_mode != ESR_RES_NONE) return 0;
    if (d->split || d->tail_cout || d->tail_mid_act || d->tail_seg_stride16 || d->post2_wpacked || d->post2_out.ptr || d->post2_cout || d->out1.ptr ||
        d->border_bias || d->blocked8 || d->in_seg_stride || d->in_seg_chunks || d->wino_wpacked || d->hilo || d->hilo_stride) return 0;
    if (esr_tiles(d->n, d->h, d->w, RS_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_resdb_step(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->post_out.ptr || !d->wpacked || !d->post_wpacked || !d->tail_wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_resdb_step_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int nd = d->post_cout / 16, nx = d->tail_cat_c / 16;
    if ((nx >= 1) != (d->res.ptr != nullptr) || (nx >= 2) != (d->tail_cat.ptr != nullptr)) return ESR_ERR_BAD_ARG;
    if (!esr_view_fits(d->in, 8, 48) || !esr_view_fits(d->out0, 8, 48) || !esr_view_fits(d->post_out, 8, 16 * nd)) return ESR_ERR_BAD_ARG;
    if ((nx >= 1 && !esr_view_fits(d->res, 8, 16)) || (nx >= 2 && !esr_view_fits(d->tail_cat, 8, 16))) return ESR_ERR_BAD_ARG;
    // neither output's bytes meet x (the neighbouring tiles read its halo), an extra input, or the other output
    const size_t npx = (size_t)d->n * d->h * d->w;
    const esr_view* ins[3] = {&d->in, &d->res, &d->tail_cat};
    const int in_c[3] = {48, 16, 16};
    for (int i = 0; i <= nx; ++i)
        if (esr_views_meet(d->out0, 48, *ins[i], in_c[i], npx, 2) || esr_views_meet(d->post_out, 16 * nd, *ins[i], in_c[i], npx, 2)) return ESR_ERR_BAD_ARG;
    if (esr_views_meet(d->out0, 48, d->post_out, 16 * nd, npx, 2)) return ESR_ERR_BAD_ARG;
    ResdbK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.e0 = static_cast<const char*>(d->res.ptr);
    k.e1 = static_cast<const char*>(d->tail_cat.ptr);
    k.w1 = static_cast<const char*>(d->post_wpacked);
    k.w3 = static_cast<const char*>(d->wpacked);
    k.a = static_cast<const float*>(d->tail_wpacked);
    k.d = static_cast<char*>(d->post_out.ptr);
    k.y = static_cast<char*>(d->out0.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.x_pitch = d->in.pitch; k.x_coff = d->in.coff;
    k.e0_pitch = d->res.pitch; k.e0_coff = d->res.coff;
    k.e1_pitch = d->tail_cat.pitch; k.e1_coff = d->tail_cat.coff;
    k.d_pitch = d->post_out.pitch; k.d_coff = d->post_out.coff;
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, RS_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return d->storage == ESR_STORE_BF16 ? launch_resdb_nx<true>(k, nx, nd, st) : launch_resdb_nx<false>(k, nx, nd, st);
}

}  // extern "C"
