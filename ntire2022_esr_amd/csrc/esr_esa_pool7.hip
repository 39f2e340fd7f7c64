// esr_esa_pool7.hip -- EFDN's ESA low-resolution branch (models/team05_efdn/plainblock.py:124-150).  Interfaces: esr_esa_lowres_f32 with
// w_s2 == NULL (dispatched here from esr_esa_lowres.hip) and esr_maxpool7s7_f32 (include/esr_hip.h).
//
//     v   = max_pool2d(c1_, 7, stride 7, padding 1)          straight on the FULL-RESOLUTION conv1 map: no stride-2 conv
//     c23 = cat(relu(conv_2(v)), relu(conv_3(v)))           two parallel 3x3 f -> f
//     c3  = conv_23(c23)                                    3x3 2f -> f, no activation
//
// Two launches, only the pooled map in between (as esr_esa_lowres.hip does for RFDN's branch):
//   esa_pool7_kernel         one thread per (pooled pixel, 4 channels): the 7x7 window, padding never wins (its -inf); the windows do not
//                            overlap, so the conv1 map is read at most once.  The per-op form (esr_maxpool7s7_f32) launches the same kernel.
//   esa_pool7_branch_kernel  one block = a 6x6 tile of conv_23's output: the 10x10 pooled patch in LDS, the pair's 8x8 outputs in two LDS
//                            maps (positions outside the map written as zeros: conv_23's zero padding), conv_23 over them as two K = 16
//                            halves -- the 2f-channel concat never exists.  Every convolution on v_mfma_f32_16x16x4_f32 (exact fp32) with its
//                            weights in registers, as esa_chain_kernel.
#include <hip/hip_runtime.h>
#include <math.h>

#include "esr_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int FP = ESR_ESA_FP;                 // 16: channel pitch of every map here
constexpr int OT = 6;                          // conv_23 output tile edge (339x510 -> 48 x 73: 8 x 13 tiles)
constexpr int MT = OT + 2;                     // pair outputs per edge: 64 pixels = one 16-pixel group per wave
constexpr int VT = OT + 4;                     // pooled patch per edge
constexpr int BP = 20;                         // floats per pixel of the LDS maps (16 + 4: adjacent pixels on different banks)

// blocks dealt to the 8 XCDs in raster eighths, so neighbouring tiles (which share their halo) meet in the same L2
__device__ __forceinline__ int p7_xcd_tile()
{
    const int G8 = (int)gridDim.x & ~7, b = (int)blockIdx.x;
    return b < G8 ? (b & 7) * (G8 >> 3) + (b >> 3) : b;
}

template <int ST>
__device__ __forceinline__ f32x4 p7_ld4(const void* base, size_t idx)
{
    if (ST == ESR_STORE_F32) return *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + idx);
    const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(base) + idx);
    f32x4 v;
    if (ST == ESR_STORE_BF16) {
        v.x = __builtin_bit_cast(float, u.x << 16); v.y = __builtin_bit_cast(float, u.x & 0xffff0000u);
        v.z = __builtin_bit_cast(float, u.y << 16); v.w = __builtin_bit_cast(float, u.y & 0xffff0000u);
    } else {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 a = __builtin_bit_cast(h2, u.x), b = __builtin_bit_cast(h2, u.y);
        v.x = (float)a[0]; v.y = (float)a[1]; v.z = (float)b[0]; v.w = (float)b[1];
    }
    return v;
}

// ---- max_pool2d(7, 7, padding 1) ------------------------------------------------------------------------------------------------
// Window of pooled row oy: rows 7 oy - 1 .. 7 oy + 5.  It always holds at least one image row (h7 = (h - 5) / 7 + 1), so a coordinate
// clamped into the image is a row of the SAME window: the max is unchanged, and all 49 loads are unconditional and in flight at once.
template <int ST>
__global__ __launch_bounds__(256) void esa_pool7_kernel(const void* __restrict__ x, float* __restrict__ y, int N, int H, int W, int H7, int W7)
{
    const int q = threadIdx.x & 3;
    const long long pix = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
    if (pix >= (long long)N * H7 * W7) return;
    const int ox = (int)(pix % W7);
    const int oy = (int)((pix / W7) % H7);
    const int n = (int)(pix / ((long long)W7 * H7));
    int xs[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) xs[k] = min(max(7 * ox - 1 + k, 0), W - 1);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
        const size_t row = ((size_t)n * H + min(max(7 * oy - 1 + ky, 0), H - 1)) * W;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const f32x4 v = p7_ld4<ST>(x, (row + xs[kx]) * FP + 4 * q);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    *reinterpret_cast<f32x4*>(y + (size_t)pix * FP + 4 * q) = m;
}

// ---- the pair and conv_23 -------------------------------------------------------------------------------------------------------
// D[cout][pixel] += W[cout][cin] X[cin][pixel] per tap, 16 pixels per group.  Lane (j = l & 15, g = l >> 4): A = W[cout j][cin 4g + s],
// B = X[pixel j][cin 4g + s] for the four K steps s of a tap; D: lane (j, g) holds output channels 4g .. 4g + 3 of pixel j.
// Weights: esr_pack_dense_f32 [tap][ROWS][16] + bias[16]; rows row0 .. row0 + 15 of every tap (conv_23: 0 = conv_2's half, 16 = conv_3's).
template <int ROWS>
__device__ __forceinline__ void p7_load_weights(const float* __restrict__ wp, int row0, f32x4 (&wr)[9], int lane)
{
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float* r = wp + (t * ROWS + row0 + 4 * g) * FP + j;
        f32x4 v;
        v.x = r[0]; v.y = r[FP]; v.z = r[2 * FP]; v.w = r[3 * FP];
        wr[t] = v;
    }
}

__device__ __forceinline__ f32x4 p7_mfma4(f32x4 a, f32x4 b, f32x4 acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ f32x4 p7_act(f32x4 v, int act)
{
    if (act == ESR_ACT_RELU) return f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
    if (act == ESR_ACT_LRELU) return f32x4{fmaxf(v.x, 0.05f * v.x), fmaxf(v.y, 0.05f * v.y), fmaxf(v.z, 0.05f * v.z), fmaxf(v.w, 0.05f * v.w)};
    return v;
}

struct Pool7K {
    const float* x;            // pooled map [n][H7][W7][16]
    float* y;                  // conv_23's output [n][H7][W7][16]
    const float* w2;           // conv_2: dense [9][16][16] + bias
    const float* w3;           // conv_3: likewise
    const float* w23;          // conv_23: dense [9][32][16] + bias (rows 0 .. 15: conv_2's channels, 16 .. 31: conv_3's)
    int H7, W7, tiles_x, tiles_y;
    int act_pair, act_out;
};

__global__ __launch_bounds__(256) void esa_pool7_branch_kernel(const Pool7K p)
{
    __shared__ __attribute__((aligned(16))) float sv[VT * VT * BP];
    __shared__ __attribute__((aligned(16))) float s2[MT * MT * BP];
    __shared__ __attribute__((aligned(16))) float s3[MT * MT * BP];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    int t = p7_xcd_tile();
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int n = t / p.tiles_y;
    const int vy = OT * ty - 2, vx = OT * tx - 2;                  // map coordinates of the patch's (0, 0)
    for (int it = threadIdx.x; it < VT * VT * 4; it += 256) {
        const int qq = it & 3, pl = it >> 2;
        const int ly = pl / VT, lx = pl - ly * VT;
        const int gy = vy + ly, gx = vx + lx;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};                            // outside the map: the pair's zero padding
        if (gy >= 0 && gy < p.H7 && gx >= 0 && gx < p.W7) v = *reinterpret_cast<const f32x4*>(p.x + (((size_t)n * p.H7 + gy) * p.W7 + gx) * FP + qq * 4);
        *reinterpret_cast<f32x4*>(sv + pl * BP + qq * 4) = v;
    }
    f32x4 wa[9], wb[9];
    p7_load_weights<FP>(p.w2, 0, wa, lane);
    p7_load_weights<FP>(p.w3, 0, wb, lane);
    const f32x4 ba = *reinterpret_cast<const f32x4*>(p.w2 + 9 * FP * FP + 4 * g);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(p.w3 + 9 * FP * FP + 4 * g);
    __syncthreads();
    // conv_2 and conv_3 on the same staged inputs: MT x MT outputs, one 16-pixel group per wave
    for (int grp = wv; grp * 16 < MT * MT; grp += 4) {
        const int pl = grp * 16 + j;
        const int ly = pl / MT, lx = pl - ly * MT;
        const float* in = sv + (ly * VT + lx) * BP + 4 * g;
        f32x4 a2 = ba, a3 = bb;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(in + (ky * VT + kx) * BP);
                a2 = p7_mfma4(wa[ky * 3 + kx], b, a2);
                a3 = p7_mfma4(wb[ky * 3 + kx], b, a3);
            }
        const int gy = vy + 1 + ly, gx = vx + 1 + lx;
        const bool inside = gy >= 0 && gy < p.H7 && gx >= 0 && gx < p.W7;
        a2 = p7_act(a2, p.act_pair);
        a3 = p7_act(a3, p.act_pair);
        if (!inside) a2 = a3 = f32x4{0.f, 0.f, 0.f, 0.f};          // conv_23's zero padding
        *reinterpret_cast<f32x4*>(s2 + pl * BP + 4 * g) = a2;
        *reinterpret_cast<f32x4*>(s3 + pl * BP + 4 * g) = a3;
    }
    f32x4 wc[9], wd[9];
    p7_load_weights<2 * FP>(p.w23, 0, wc, lane);
    p7_load_weights<2 * FP>(p.w23, FP, wd, lane);
    const f32x4 bc = *reinterpret_cast<const f32x4*>(p.w23 + 9 * 2 * FP * FP + 4 * g);
    __syncthreads();
    // conv_23 = W[:, :16] * c2 + W[:, 16:] * c3: two K = 16 halves into one accumulator
    for (int grp = wv; grp * 16 < OT * OT; grp += 4) {
        const int pl = grp * 16 + j;
        const bool live = pl < OT * OT;
        const int plc = live ? pl : 0;
        const int ly = plc / OT, lx = plc - ly * OT;
        const int base = (ly * MT + lx) * BP + 4 * g;
        f32x4 acc = bc;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int o = base + (ky * MT + kx) * BP;
                acc = p7_mfma4(wc[ky * 3 + kx], *reinterpret_cast<const f32x4*>(s2 + o), acc);
                acc = p7_mfma4(wd[ky * 3 + kx], *reinterpret_cast<const f32x4*>(s3 + o), acc);
            }
        acc = p7_act(acc, p.act_out);
        const int gy = OT * ty + ly, gx = OT * tx + lx;
        if (live && gy < p.H7 && gx < p.W7) *reinterpret_cast<f32x4*>(p.y + (((size_t)n * p.H7 + gy) * p.W7 + gx) * FP + 4 * g) = acc;
    }
}

bool act_ok(int a) { return a == ESR_ACT_NONE || a == ESR_ACT_RELU || a == ESR_ACT_LRELU; }

int launch_pool7(const void* x, float* y, int storage, int n, int h, int w, int h7, int w7, hipStream_t st)
{
    const long long npix = (long long)n * h7 * w7;
    if ((npix + 63) / 64 >= ESR_INDEX_LIMIT) return ESR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((npix + 63) / 64));
    switch (storage) {
        case ESR_STORE_F32: esr_note_kernel("esa_pool7_kernel<0>"); hipLaunchKernelGGL(esa_pool7_kernel<ESR_STORE_F32>, grid, dim3(256), 0, st, x, y, n, h, w, h7, w7); break;
        case ESR_STORE_BF16: esr_note_kernel("esa_pool7_kernel<1>"); hipLaunchKernelGGL(esa_pool7_kernel<ESR_STORE_BF16>, grid, dim3(256), 0, st, x, y, n, h, w, h7, w7); break;
        case ESR_STORE_F16: esr_note_kernel("esa_pool7_kernel<2>"); hipLaunchKernelGGL(esa_pool7_kernel<ESR_STORE_F16>, grid, dim3(256), 0, st, x, y, n, h, w, h7, w7); break;
        default: return ESR_ERR_BAD_ARG;
    }
    return esr_check_launch("esa_pool7_kernel launch");
}

}  // namespace

int esr_esa_pool7_lowres(const esr_esa_lowres_desc* d, void* hip_stream)
{
    if (!d || d->w_s2 || !d->x.ptr || !d->pooled || !d->y) return ESR_ERR_BAD_ARG;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->f <= 0 || d->f > FP) return ESR_ERR_BAD_ARG;
    if (d->x.pitch != FP || d->x.coff) return ESR_ERR_BAD_ARG;
    if (d->storage != ESR_STORE_F32 && d->storage != ESR_STORE_BF16 && d->storage != ESR_STORE_F16) return ESR_ERR_BAD_ARG;
    const esr_esa_layer& a = d->layer[0];
    const esr_esa_layer& b = d->layer[1];
    if (d->n_layers != 2 || a.kind != 2 || b.kind != 3 || !a.w || !a.w_dw || !b.w || !act_ok(a.act) || !act_ok(b.act)) return ESR_ERR_BAD_ARG;
    if (d->h < 5 || d->w < 5) return ESR_ERR_TOO_SMALL;                            // (5 + 2 - 7) / 7 + 1 = 1: one pooling window
    const int H7 = (d->h - 5) / 7 + 1, W7 = (d->w - 5) / 7 + 1;
    Pool7K k;
    k.H7 = H7; k.W7 = W7;
    k.tiles_x = (W7 + OT - 1) / OT; k.tiles_y = (H7 + OT - 1) / OT;
    if ((long long)d->n * k.tiles_x * k.tiles_y >= ESR_INDEX_LIMIT) return ESR_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    float* pooled = static_cast<float*>(d->pooled);
    int rc = launch_pool7(d->x.ptr, pooled, d->storage, d->n, d->h, d->w, H7, W7, st);
    if (rc != ESR_OK) return rc;
    k.x = pooled; k.y = static_cast<float*>(d->y);
    k.w2 = static_cast<const float*>(a.w); k.w3 = static_cast<const float*>(a.w_dw); k.w23 = static_cast<const float*>(b.w);
    k.act_pair = a.act; k.act_out = b.act;
    esr_note_kernel("esa_pool7_branch_kernel");
    hipLaunchKernelGGL(esa_pool7_branch_kernel, dim3((unsigned)(d->n * k.tiles_x * k.tiles_y)), dim3(256), 0, st, k);
    return esr_check_launch("esa_pool7_branch_kernel launch");
}

extern "C" int esr_maxpool7s7_f32(const esr_esa_desc* d, void* hip_stream)
{
    if (!d || !d->x.ptr || !d->y.ptr) return ESR_ERR_BAD_ARG;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return ESR_ERR_BAD_ARG;
    if (d->x.pitch != FP || d->y.pitch != FP || d->x.coff || d->y.coff) return ESR_ERR_BAD_ARG;
    if (d->h < 5 || d->w < 5) return ESR_ERR_TOO_SMALL;
    const int H7 = (d->h - 5) / 7 + 1, W7 = (d->w - 5) / 7 + 1;
    if (d->h_lo != H7 || d->w_lo != W7) return ESR_ERR_BAD_ARG;
    return launch_pool7(d->x.ptr, static_cast<float*>(d->y.ptr), d->storage, d->n, d->h, d->w, H7, W7, static_cast<hipStream_t>(hip_stream));
}
