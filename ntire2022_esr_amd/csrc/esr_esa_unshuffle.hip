// esr_esa_unshuffle.hip -- the low-resolution branch of team 35's ESA (models/team35_rfdn/rmsrb1.py:137-144).  Interface:
// esr_esa_unshuffle_f32 (include/esr_hip.h).
//
//     u  = pixel_unshuffle(c1_, 2)                            4 f channels at half resolution; a stride-2 convolution: odd H, W floored
//     p  = relu(max_pool2d(u, 7, stride 3))                   h3 = (h / 2 - 7) / 3 + 1
//     c3 = relu(con_(p))                                      nn.Conv2d(4 f, f, 1, padding 1): (h3 + 2) x (w3 + 2), the ring = relu(bias)
//
// Unshuffled channel 4 c + 2 dy + dx is channel c of c1_ at (2 y + dy, 2 x + dx), so pooled pixel (py, px) of that channel is the max of
// c1_[2 (3 py + i) + dy][2 (3 px + j) + dx][c] over i, j < 7: the unshuffled tensor and the pooled one never exist.
//
// esa_unshuffle_kernel<ST>: one 64-thread block per output pixel, ring included.  Thread u < 4 f owns unshuffled channel u and its 49 window
// values (a max is a selection: exact in every storage), relu, into LDS; thread o < 16 then sums bias + W[o][u] p[u] with fmaf in ascending
// u, relu, and stores -- the pad channels f .. 15 as zeros (zero weight columns and bias in the esr_pack_dense_f32 blob).  A ring pixel
// skips the window: relu(bias).  A few KB per image; no tuning.
#include <hip/hip_runtime.h>
#include <math.h>

#include "esr_internal.h"

namespace {

constexpr int FP = ESR_ESA_FP;                 // 16: channel pitch of the conv1 map and of c3
constexpr int UC = 4 * FP;                     // unshuffled channels at most

template <int ST>
__device__ __forceinline__ float un_ld(const void* base, size_t idx)
{
    if (ST == ESR_STORE_F32) return static_cast<const float*>(base)[idx];
    const unsigned short u = static_cast<const unsigned short*>(base)[idx];
    if (ST == ESR_STORE_BF16) return __builtin_bit_cast(float, (unsigned)u << 16);
    return (float)__builtin_bit_cast(_Float16, u);
}

struct UnK {
    const void* x;             // conv1 map [n][H][W][x_pitch] in the plan's storage
    const float* wp;           // esr_pack_dense_f32(k = 1, cin_p = 4 f, cout_p = 16): [4 f][16] + bias[16]
    float* y;                  // [n][H3 + 2][W3 + 2][y_pitch] fp32
    int H, W, H3, W3, f;
    int x_pitch, x_coff, y_pitch, y_coff;
};

template <int ST>
__global__ __launch_bounds__(64) void esa_unshuffle_kernel(const UnK p)
{
    __shared__ float sp[UC];
    const int ho = p.H3 + 2, wo = p.W3 + 2;
    int t = (int)blockIdx.x;
    const int ox = t % wo; t /= wo;
    const int oy = t % ho;
    const int n = t / ho;
    const int py = oy - 1, px = ox - 1;
    const bool ring = py < 0 || py >= p.H3 || px < 0 || px >= p.W3;       // block-uniform
    const int u = threadIdx.x, uc = 4 * p.f;
    if (!ring) {
        if (u < uc) {
            const int c = u >> 2, dy = (u >> 1) & 1, dx = u & 1;
            float m = -INFINITY;
            for (int i = 0; i < 7; ++i) {
                const size_t row = ((size_t)n * p.H + 2 * (3 * py + i) + dy) * p.W;
#pragma unroll
                for (int j = 0; j < 7; ++j) m = fmaxf(m, un_ld<ST>(p.x, (row + 2 * (3 * px + j) + dx) * p.x_pitch + p.x_coff + c));
            }
            sp[u] = fmaxf(m, 0.f);
        }
        __syncthreads();
    }
    if (u < FP) {
        float acc = p.wp[uc * FP + u];
        if (!ring)
            for (int k = 0; k < uc; ++k) acc = fmaf(p.wp[k * FP + u], sp[k], acc);
        p.y[(((size_t)n * ho + oy) * wo + ox) * p.y_pitch + p.y_coff + u] = fmaxf(acc, 0.f);
    }
}

}  // namespace

extern "C" int esr_esa_unshuffle_f32(const esr_esa_desc* d, void* hip_stream)
{
    if (!d || !d->x.ptr || !d->y.ptr || !d->w0) return ESR_ERR_BAD_ARG;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->f <= 0 || d->f > FP) return ESR_ERR_BAD_ARG;
    if (d->storage != ESR_STORE_F32 && d->storage != ESR_STORE_BF16 && d->storage != ESR_STORE_F16) return ESR_ERR_BAD_ARG;
    if (d->x.pitch <= 0 || d->x.coff < 0 || d->x.coff + d->f > d->x.pitch) return ESR_ERR_BAD_ARG;
    if (!esr_view_fits(d->y, 4, FP)) return ESR_ERR_BAD_ARG;
    if (d->h < 14 || d->w < 14) return ESR_ERR_TOO_SMALL;                          // (14 / 2 - 7) / 3 + 1 = 1: one pooling window
    const int H3 = (d->h / 2 - 7) / 3 + 1, W3 = (d->w / 2 - 7) / 3 + 1;
    if (d->h_lo != H3 + 2 || d->w_lo != W3 + 2) return ESR_ERR_BAD_ARG;
    if (!esr_fits_raw((double)d->n * d->h * d->w, d->x.pitch, 1)) return ESR_ERR_UNSUPPORTED;
    const long long nblk = (long long)d->n * d->h_lo * d->w_lo;
    if (nblk >= ESR_INDEX_LIMIT) return ESR_ERR_UNSUPPORTED;
    UnK k;
    k.x = d->x.ptr; k.wp = static_cast<const float*>(d->w0); k.y = static_cast<float*>(d->y.ptr);
    k.H = d->h; k.W = d->w; k.H3 = H3; k.W3 = W3; k.f = d->f;
    k.x_pitch = d->x.pitch; k.x_coff = d->x.coff; k.y_pitch = d->y.pitch; k.y_coff = d->y.coff;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((unsigned)nblk);
    switch (d->storage) {
        case ESR_STORE_F32: esr_note_kernel("esa_unshuffle_kernel<0>"); hipLaunchKernelGGL(esa_unshuffle_kernel<ESR_STORE_F32>, grid, dim3(64), 0, st, k); break;
        case ESR_STORE_BF16: esr_note_kernel("esa_unshuffle_kernel<1>"); hipLaunchKernelGGL(esa_unshuffle_kernel<ESR_STORE_BF16>, grid, dim3(64), 0, st, k); break;
        default: esr_note_kernel("esa_unshuffle_kernel<2>"); hipLaunchKernelGGL(esa_unshuffle_kernel<ESR_STORE_F16>, grid, dim3(64), 0, st, k); break;
    }
    return esr_check_launch("esa_unshuffle_kernel launch");
}
