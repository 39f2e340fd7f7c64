// esr_asym.hip -- one step of ARFDN's block (team14_arfdn/block.py:233-254) as ONE launch (esr_asym_step; 16-bit storage).
//
//     d   = act(W_d . in + b_d)                                       1x1, cin (17..64) -> cmid (17..32), stored 16-bit (post_out)
//     a_l = act(W_l1 (3x1) in + b_l1)    a_m = act(W_m1 (1x3) in + b_m1)          cin -> cmid each; never stored
//     out = act(W_l2 (1x3) a_l~ + W_m2 (3x1) a_m~ + (b_l2 + b_m2) [+ in] + d~ + p1 + p2)                                     (out0)
//
// act = max(v, slope v).  d~, a_l~, a_m~ are the maps AS A STORED TENSOR WOULD HOLD THEM: rounded once to the storage type, and a_l~ / a_m~ are
// 0 outside the image -- the reference zero-pads the input of the second convolution of a pair, so a halo pixel outside the image is 0,
// not act(b_l1) (esr_distill_step_s16's rule).  p1 / p2 (res / tail_cat; either may be absent) are the earlier steps' distilled maps as
// stored; `+ in` (ESR_RES_PRE_ACT) needs cin == cmid.  Every sum is fp32.  Layer by layer a pixel of a cin = 25 step moves 64 (in, three
// times) + 2 x 64 (d, out) + 2 x 128 (a_l | a_m written and read) + the p reads through HBM; here `in` is read once and d and out are written once.
//
// A block owns one 16 x 16 output tile at a time (persistent over the tiles) and keeps in LDS, all as [16-channel chunk][pixel][32 B]
// (conv_s16_kernel's stage layout: a B fragment is 16 B of one pixel)
//
//     in   18 x 18 pixels   staged ONCE with a one-pixel halo by LDS-DMA; pieces outside the image arrive as zeros (the corners are staged
//                           with the rest -- whole DMA instructions -- and never read)
//     d    16 x 16          the 1x1 on the tile's own pixels, rounded; also stored to post_out
//     a_l  16 rows x 18 columns   the 3x1 (vertical taps) wherever the 1x3 behind it reads;   a_m  18 rows x 16 columns likewise
//
// The MFMA K dimension is channels x THREE taps: one v_mfma_f32_16x16x32 step is one tap over 32 channels (lane quarter kq: chunk kq >> 1,
// half kq & 1), so a 3-tap convolution over 32 channels is 3 steps where a zero-padded 3x3 would be 5 tap pairs.  The 3-tap images
// (esr_pack_asym_s16: 36 fragments at cin > 32, 24 else) live in registers for the block's lifetime, the 1x1's esr_pack_conv_s16 image (hi + lo
// weights, as the stand-alone 1x1 launch multiplies by) in LDS.  Per accumulator: bias as the first MFMA's C, taps in order, l before m.
// `in`'s channels at and beyond cin are zero in LDS (distill_step_kernel's masking): a tensor's pad slots and the bytes behind it never reach
// an MFMA or the residual; p1 / p2 are read for the tile's own pixels only and masked beyond cmid.
// LDS: 8 KB + 41 KB in + 16 KB d + 2 x 18 KB = 101 KB; one 4-wave block per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "esr_s16_dev.h"

namespace {

constexpr int AS_T = 16;                                   // output tile (pixels per side)
constexpr int AS_NW = 4;
constexpr int AS_R = AS_T + 2;                             // staged region (pixels per side)
constexpr int AS_PIX = AS_R * AS_R;
constexpr int AS_APIX = AS_T * AS_R;                       // pixels of a_l (16 x 18) and of a_m (18 x 16)
constexpr int AS_NT = 2;                                   // output tiles of every layer (cmid in 17..32)
constexpr int AS_MAXCH = 4;                                // chunks of `in` (cin <= 64)
constexpr int AS_XCH = AS_PIX * 32;                        // bytes of one 16-channel chunk of the staged input
constexpr int AS_DCH = AS_T * AS_T * 32;                   // ... of d
constexpr int AS_ACH = AS_APIX * 32;                       // ... of a_l / a_m
constexpr int as_x_bytes(int nch) { return (nch * AS_PIX * 2 + 63) / 64 * 64 * 16; }      // whole DMA instructions (64 pieces of 16 bytes)
constexpr int AS_OFF_W1 = 0;
constexpr int AS_OFF_X = AS_MAXCH * AS_NT * 1024;
constexpr int AS_OFF_D = AS_OFF_X + as_x_bytes(AS_MAXCH);
constexpr int AS_OFF_AL = AS_OFF_D + AS_NT * AS_DCH;
constexpr int AS_OFF_AM = AS_OFF_AL + AS_NT * AS_ACH;
constexpr int AS_LDS = AS_OFF_AM + AS_NT * AS_ACH;
constexpr int AS_GROUPS_A = AS_APIX / 16;                  // groups of 16 pixels of a_l and of a_m
constexpr int AS_JOBS = AS_T + 2 * AS_GROUPS_A;            // d's 16 rows, then a_l's groups, then a_m's
static_assert(AS_LDS <= LDS_LIMIT && AS_OFF_X % 1024 == 0 && AS_OFF_D % 16 == 0 && AS_APIX % 16 == 0, "LDS plan");

struct AsymK {
    const char* x;            // NHWC 16-bit input (cin channels from in_coff)
    const char* w1;           // esr_pack_conv_s16 blob of the 1x1 (cin -> cmid; hi + lo)
    const char* wa;           // esr_pack_asym_s16 blob
    const char* p1;           // earlier distilled maps added before the activation, or NULL
    const char* p2;
    char* d;                  // NHWC 16-bit distilled map
    char* y;                  // NHWC 16-bit step result
    int N, H, W;
    int in_pitch, in_coff, d_pitch, d_coff, y_pitch, y_coff, p1_pitch, p1_coff, p2_pitch, p2_coff;
    int cin, cmid;            // logical channels: nothing at or beyond them is read
    int nch1;                 // chunks of the 1x1's image: round_up(cin, 16) / 16
    int d_cout8, y_cout8;     // channels stored
    float slope;              // max(v, slope v)
    int tiles_x, tiles_y, ntiles;
};

__device__ __forceinline__ f32x4 as_act(f32x4 v, float s)
{
    v.x = act1(v.x, s); v.y = act1(v.y, s); v.z = act1(v.z, s); v.w = act1(v.w, s);
    return v;
}

// a distilled map's channels ch .. ch + 3 of one pixel, those at and beyond cmid as zeros
template <bool BF16>
__device__ __forceinline__ f32x4 as_load_p(const char* p, int ch, int cmid)
{
    f32x4 v = unpack4<BF16>(*reinterpret_cast<const uint2*>(p + ch * 2));
    v.x = ch + 0 < cmid ? v.x : 0.f; v.y = ch + 1 < cmid ? v.y : 0.f; v.z = ch + 2 < cmid ? v.z : 0.f; v.w = ch + 3 < cmid ? v.w : 0.f;
    return v;
}

// NKP: 32-channel K pairs of `in` (2: cin 33..64, 1: 17..32); RES: + in before the activation (cin == cmid: NKP == 1)
template <bool BF16, int NKP, bool RES>
__global__ __launch_bounds__(64 * AS_NW, 1) void asym_step_kernel(const AsymK p)
{
    static_assert(!RES || NKP == 1, "the residual is the input: as many channels as outputs");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 15, kq = lane >> 4;
    constexpr int NCH = 2 * NKP;                           // 16-channel chunks staged
    constexpr int F1 = 3 * NKP * AS_NT, F2 = 3 * AS_NT;    // fragments of a first / second convolution of a pair
    const int W1B = p.nch1 * AS_NT * 1024;
    constexpr int WAB = (2 * F1 + 2 * F2) * 1024;

    // the 1x1's image into LDS, the 3-tap images into registers: once per block
    for (int i = tid * 16; i < W1B; i += 64 * AS_NW * 16)
        *reinterpret_cast<i32x4*>(smem + AS_OFF_W1 + i) = *reinterpret_cast<const i32x4*>(p.w1 + i);
    i32x4 al1[3][NKP][AS_NT], am1[3][NKP][AS_NT], al2[3][AS_NT], am2[3][AS_NT];
    static_for<3>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        static_for<AS_NT>([&](auto o_) {
            constexpr int o = decltype(o_)::value;
            static_for<NKP>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                al1[t][k][o] = *reinterpret_cast<const i32x4*>(p.wa + ((t * NKP + k) * AS_NT + o) * 1024 + lane * 16);
                am1[t][k][o] = *reinterpret_cast<const i32x4*>(p.wa + (F1 + (t * NKP + k) * AS_NT + o) * 1024 + lane * 16);
            });
            al2[t][o] = *reinterpret_cast<const i32x4*>(p.wa + (2 * F1 + t * AS_NT + o) * 1024 + lane * 16);
            am2[t][o] = *reinterpret_cast<const i32x4*>(p.wa + (2 * F1 + F2 + t * AS_NT + o) * 1024 + lane * 16);
        });
    });
    f32x4 bia1[AS_NT], bial[AS_NT], biam[AS_NT], bia2[AS_NT];
    static_for<AS_NT>([&](auto o_) {
        constexpr int o = decltype(o_)::value;
        bia1[o] = *reinterpret_cast<const f32x4*>(p.w1 + W1B + (o * 16 + kq * 4) * 4);
        bial[o] = *reinterpret_cast<const f32x4*>(p.wa + WAB + (0 * 32 + o * 16 + kq * 4) * 4);
        biam[o] = *reinterpret_cast<const f32x4*>(p.wa + WAB + (1 * 32 + o * 16 + kq * 4) * 4);
        bia2[o] = *reinterpret_cast<const f32x4*>(p.wa + WAB + (2 * 32 + o * 16 + kq * 4) * 4);
    });
    const float slope = p.slope;
    const int boff = (kq >> 1) * AS_XCH + (kq & 1) * 16;   // a lane's 16 bytes inside a staged pixel: chunk kq >> 1 of the K pair, half kq & 1
    const int aoff = (kq >> 1) * AS_ACH + (kq & 1) * 16;   // ... inside a pixel of a_l / a_m

    const size_t img_bytes = (size_t)p.H * p.W * p.in_pitch * 2;
    const int cvalid8 = (p.cin + 7) & ~7;                 // channels moved per pixel: whole 16-byte pieces up to round_up(cin, 8)
    constexpr int ITEMS = NCH * AS_PIX * 2;               // 16-byte pieces of the staged input
    constexpr int NINST = (ITEMS + 63) / 64;              // (the last instruction's pieces beyond ITEMS: zeros behind the last chunk)

    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int per = p.tiles_x * p.tiles_y;
        const int n = t / per, rem = t - n * per;
        const int y0 = (rem / p.tiles_x) * AS_T, x0 = (rem % p.tiles_x) * AS_T;

        // ---- in with a one-pixel halo: piece (chunk c, pixel, half h) -> LDS byte AS_OFF_X + c * AS_XCH + pixel * 32 + h * 16 -----------------
        const i32x4 rs = make_rsrc(p.x + (size_t)n * img_bytes, img_bytes);
        for (int i = wv; i < NINST; i += AS_NW) {
            const int item = i * 64 + lane;
            const int c = item / (AS_PIX * 2), pr = item - c * (AS_PIX * 2);
            const int pix = pr >> 1, h = pr & 1;
            const int gy = y0 - 1 + pix / AS_R, gx = x0 - 1 + pix % AS_R;
            const int ch = c * 16 + h * 8;
            const bool ok = item < ITEMS && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W && ch < cvalid8;
            const unsigned voff = ok ? (unsigned)(((gy * p.W + gx) * p.in_pitch + p.in_coff + ch) * 2) : OOB;
            dma_buf16(smem_lds + (unsigned)(AS_OFF_X + i * 1024), voff, rs, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (p.cin & 7) {
            // the last piece holds channels cvalid8 - 8 .. cvalid8 - 1, of which those >= cin are pad slots of the tensor: zero
            const int cl = cvalid8 - 8, keep = p.cin - cl;
            const int base = AS_OFF_X + (cl >> 4) * AS_XCH + ((cl >> 3) & 1) * 16;
            for (int pix = tid; pix < AS_PIX; pix += 64 * AS_NW) {
                i32x4 v = *reinterpret_cast<const i32x4*>(smem + base + pix * 32);
                v.x = keep >= 2 ? v.x : (keep == 1 ? (v.x & 0xffff) : 0);
                v.y = keep >= 4 ? v.y : (keep == 3 ? (v.y & 0xffff) : 0);
                v.z = keep >= 6 ? v.z : (keep == 5 ? (v.z & 0xffff) : 0);
                v.w = keep == 7 ? (v.w & 0xffff) : 0;
                *reinterpret_cast<i32x4*>(smem + base + pix * 32) = v;
            }
            __syncthreads();
        }

        // a_l (ISL: the 3x1 -- vertical taps, staged rows r, r + 1, r + 2 of column c -- on 16 rows x 18 columns) or a_m (the 1x3 -- horizontal
        // taps, staged columns c, c + 1, c + 2 of row r -- on 18 rows x 16 columns): group g of 16 pixels
        auto first_of_pair = [&](auto isl_, int g) {
            constexpr bool ISL = decltype(isl_)::value;
            const int pp = g * 16 + px;
            const int r = ISL ? pp / AS_R : pp / AS_T, c = ISL ? pp - r * AS_R : pp - r * AS_T;
            const int s0 = r * AS_R + c;
            constexpr int SSTEP = ISL ? AS_R : 1;
            const int gy = ISL ? y0 + r : y0 - 1 + r, gx = ISL ? x0 - 1 + c : x0 + c;
            const bool inside = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            f32x4 acc[AS_NT];
            static_for<3>([&](auto t_) {
                constexpr int tp = decltype(t_)::value;
                static_for<NKP>([&](auto k_) {
                    constexpr int k = decltype(k_)::value;
                    const i32x4 b = *reinterpret_cast<const i32x4*>(smem + AS_OFF_X + 2 * k * AS_XCH + (s0 + tp * SSTEP) * 32 + boff);
                    static_for<AS_NT>([&](auto o_) {
                        constexpr int o = decltype(o_)::value;
                        const f32x4 c0 = (tp == 0 && k == 0) ? (ISL ? bial[o] : biam[o]) : acc[o];
                        acc[o] = mfma32<BF16>(ISL ? al1[tp][k][o] : am1[tp][k][o], b, c0);
                    });
                });
            });
            static_for<AS_NT>([&](auto o_) {
                constexpr int o = decltype(o_)::value;
                const f32x4 v = as_act(acc[o], slope);
                uint2 pk;
                pk.x = inside ? pack2<BF16>(v.x, v.y) : 0u;           // outside the image: the second convolution's zero padding
                pk.y = inside ? pack2<BF16>(v.z, v.w) : 0u;
                *reinterpret_cast<uint2*>(smem + (ISL ? AS_OFF_AL : AS_OFF_AM) + o * AS_ACH + pp * 32 + kq * 8) = pk;
            });
        };

        // ---- d on the tile's pixels, a_l on 16 x 18, a_m on 18 x 16: 52 groups of 16 pixels dealt to the waves ------------------------------
        for (int job = wv; job < AS_JOBS; job += AS_NW) {
            if (job < AS_T) {
                // d = act(1x1(in)): K = 32 is [hi | lo] weights x the chunk's 16 channels twice
                const int row = job;
                const int sp = ((row + 1) * AS_R + px + 1) * 32 + (kq & 1) * 16;
                f32x4 acc[AS_NT];
                static_for<NCH>([&](auto c_) {
                    constexpr int c = decltype(c_)::value;
                    if (c < 2 || c < p.nch1) {             // (cin 33..48: three chunks; the staged fourth one is zeros and has no image)
                        const i32x4 b = *reinterpret_cast<const i32x4*>(smem + AS_OFF_X + c * AS_XCH + sp);
                        static_for<AS_NT>([&](auto o_) {
                            constexpr int o = decltype(o_)::value;
                            const i32x4 a = *reinterpret_cast<const i32x4*>(smem + AS_OFF_W1 + (c * AS_NT + o) * 1024 + lane * 16);
                            acc[o] = mfma32<BF16>(a, b, c == 0 ? bia1[o] : acc[o]);
                        });
                    }
                });
                const int gy = y0 + row, gx = x0 + px;
                const bool inside = gy < p.H && gx < p.W;
                char* const dp = p.d + (((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0)) * p.d_pitch * 2 + (size_t)p.d_coff * 2;
                static_for<AS_NT>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    const f32x4 v = as_act(acc[o], slope);
                    uint2 pk;
                    pk.x = pack2<BF16>(v.x, v.y);
                    pk.y = pack2<BF16>(v.z, v.w);
                    *reinterpret_cast<uint2*>(smem + AS_OFF_D + o * AS_DCH + (row * AS_T + px) * 32 + kq * 8) = pk;
                    const int ch = o * 16 + kq * 4;
                    if (inside && ch < p.d_cout8) *reinterpret_cast<uint2*>(dp + ch * 2) = pk;
                });
            } else if (job < AS_T + AS_GROUPS_A) {
                first_of_pair(std::true_type{}, job - AS_T);
            } else {
                first_of_pair(std::false_type{}, job - AS_T - AS_GROUPS_A);
            }
        }
        __syncthreads();

        // ---- out = act(1x3(a_l) + 3x1(a_m) + b (+ in) + d + p1 + p2): four image rows of the tile per wave -----------------------------------
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = wv * 4 + j;
            f32x4 acc[AS_NT];
            static_for<3>([&](auto t_) {
                constexpr int tp = decltype(t_)::value;
                const i32x4 b = *reinterpret_cast<const i32x4*>(smem + AS_OFF_AL + (row * AS_R + px + tp) * 32 + aoff);
                static_for<AS_NT>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    acc[o] = mfma32<BF16>(al2[tp][o], b, tp == 0 ? bia2[o] : acc[o]);
                });
            });
            static_for<3>([&](auto t_) {
                constexpr int tp = decltype(t_)::value;
                const i32x4 b = *reinterpret_cast<const i32x4*>(smem + AS_OFF_AM + ((row + tp) * AS_T + px) * 32 + aoff);
                static_for<AS_NT>([&](auto o_) {
                    constexpr int o = decltype(o_)::value;
                    acc[o] = mfma32<BF16>(am2[tp][o], b, acc[o]);
                });
            });
            const int gy = y0 + row, gx = x0 + px;
            const bool inside = gy < p.H && gx < p.W;
            const size_t pixel = ((size_t)n * p.H + (inside ? gy : 0)) * p.W + (inside ? gx : 0);
            char* const yp = p.y + pixel * p.y_pitch * 2 + (size_t)p.y_coff * 2;
            static_for<AS_NT>([&](auto o_) {
                constexpr int o = decltype(o_)::value;
                f32x4 v = acc[o];
                const int ch = o * 16 + kq * 4;
                if constexpr (RES) {
                    // + in: channels 16 o + 4 kq .. + 3 of the staged tile's pixel (row + 1, px + 1)
                    const f32x4 xf = unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + AS_OFF_X + o * AS_XCH + ((row + 1) * AS_R + px + 1) * 32 + kq * 8));
                    v.x += xf.x; v.y += xf.y; v.z += xf.z; v.w += xf.w;
                }
                const f32x4 df = unpack4<BF16>(*reinterpret_cast<const uint2*>(smem + AS_OFF_D + o * AS_DCH + (row * AS_T + px) * 32 + kq * 8));
                v.x += df.x; v.y += df.y; v.z += df.z; v.w += df.w;
                if (inside && ch < p.y_cout8) {
                    if (p.p1 && ch < p.d_cout8) {
                        const f32x4 q = as_load_p<BF16>(p.p1 + pixel * p.p1_pitch * 2 + (size_t)p.p1_coff * 2, ch, p.cmid);
                        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                    }
                    if (p.p2 && ch < p.d_cout8) {
                        const f32x4 q = as_load_p<BF16>(p.p2 + pixel * p.p2_pitch * 2 + (size_t)p.p2_coff * 2, ch, p.cmid);
                        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                    }
                    v = as_act(v, slope);
                    uint2 pk;
                    pk.x = pack2<BF16>(v.x, v.y);
                    pk.y = pack2<BF16>(v.z, v.w);
                    *reinterpret_cast<uint2*>(yp + ch * 2) = pk;
                }
            });
        }
        __syncthreads();                                  // in, d, a_l and a_m are read: the next tile's DMA and first phase may overwrite them
    }
}

template <bool BF16, int NKP, bool RES>
int launch_asym(const AsymK& k, hipStream_t st)
{
    static esr_lds_optin_flags optin;
    if (const int rc = esr_lds_optin(optin, reinterpret_cast<const void*>(&asym_step_kernel<BF16, NKP, RES>), AS_LDS, "asym_step_kernel")) return rc;
    const int grid = esr_persistent_grid(k.ntiles, ESR_BLOCKS_1_PER_CU);      // one block per CU (LDS), persistent over the tiles
    esr_note_kernel("asym_step_kernel<%s, %d, %s>", esr_tf(BF16), NKP, esr_tf(RES));
    hipLaunchKernelGGL((asym_step_kernel<BF16, NKP, RES>), dim3(grid), dim3(64 * AS_NW), AS_LDS, st, k);
    return esr_check_launch("asym_step_kernel launch");
}

inline int as_nkp(int cin) { return cin > 32 ? 2 : 1; }
inline int as_frags(int cin) { return 2 * 3 * as_nkp(cin) * AS_NT + 2 * 3 * AS_NT; }

}  // namespace

extern "C" {

size_t esr_packed_asym_s16_bytes(int cin, int cmid)
{
    if (cin < 17 || cin > 64 || cmid < 17 || cmid > 32) return 0;
    return (size_t)as_frags(cin) * 1024 + 3 * 32 * 4;
}

// element e of lane `lane` of fragment (tap, K pair kp, output tile o): W[16 o + (lane & 15)][32 kp + 8 (lane >> 4) + e][tap]
int esr_pack_asym_s16(const float* w_l1, const float* b_l1, const float* w_m1, const float* b_m1, const float* w_l2, const float* b_l2,
                      const float* w_m2, const float* b_m2, int cin, int cmid, int compute, void* out, size_t out_bytes)
{
    const size_t need = esr_packed_asym_s16_bytes(cin, cmid);
    if (!w_l1 || !w_m1 || !w_l2 || !w_m2 || !out || !need || out_bytes < need) return ESR_ERR_BAD_ARG;
    if (!esr_is_s16(compute)) return ESR_ERR_BAD_ARG;
    memset(out, 0, need);
    char* o = static_cast<char*>(out);
    const int nkp = as_nkp(cin);
    size_t frag = 0;
    auto image = [&](const float* w, int ci, int kps) {
        for (int tap = 0; tap < 3; ++tap)
            for (int kp = 0; kp < kps; ++kp)
                for (int ot = 0; ot < AS_NT; ++ot, ++frag)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const int co = ot * 16 + (lane & 15), ch = kp * 32 + (lane >> 4) * 8 + e;
                            const float v = (co < cmid && ch < ci) ? w[((size_t)co * ci + ch) * 3 + tap] : 0.f;
                            const uint16_t h = esr_host_to16(v, compute);
                            memcpy(o + (frag * 64 + lane) * 16 + e * 2, &h, 2);
                        }
    };
    image(w_l1, cin, nkp);
    image(w_m1, cin, nkp);
    image(w_l2, cmid, 1);
    image(w_m2, cmid, 1);
    float* b = reinterpret_cast<float*>(o + frag * 1024);
    for (int i = 0; i < cmid; ++i) {
        b[i] = b_l1 ? b_l1[i] : 0.f;
        b[32 + i] = b_m1 ? b_m1[i] : 0.f;
        b[64 + i] = (b_l2 ? b_l2[i] : 0.f) + (b_m2 ? b_m2[i] : 0.f);
    }
    return ESR_OK;
}

// the EFFECTIVE weights [cmid][c][3] of the four convolutions (what the kernel multiplies by) and the three bias rows b_l1, b_m1, b_l2 + b_m2
int esr_unpack_asym_s16(const void* packed, size_t packed_bytes, int cin, int cmid, int compute, float* w_l1, float* w_m1, float* w_l2, float* w_m2,
                        float* bias3)
{
    const size_t need = esr_packed_asym_s16_bytes(cin, cmid);
    if (!packed || !need || packed_bytes < need || !w_l1 || !w_m1 || !w_l2 || !w_m2 || !bias3) return ESR_ERR_BAD_ARG;
    if (!esr_is_s16(compute)) return ESR_ERR_BAD_ARG;
    const char* o = static_cast<const char*>(packed);
    const int nkp = as_nkp(cin);
    size_t frag = 0;
    auto image = [&](float* w, int ci, int kps) {
        for (int tap = 0; tap < 3; ++tap)
            for (int kp = 0; kp < kps; ++kp)
                for (int ot = 0; ot < AS_NT; ++ot, ++frag)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const int co = ot * 16 + (lane & 15), ch = kp * 32 + (lane >> 4) * 8 + e;
                            if (co >= cmid || ch >= ci) continue;
                            uint16_t h;
                            memcpy(&h, o + (frag * 64 + lane) * 16 + e * 2, 2);
                            w[((size_t)co * ci + ch) * 3 + tap] = esr_host_from16(h, compute);
                        }
    };
    image(w_l1, cin, nkp);
    image(w_m1, cin, nkp);
    image(w_l2, cmid, 1);
    image(w_m2, cmid, 1);
    const float* b = reinterpret_cast<const float*>(o + frag * 1024);
    for (int r = 0; r < 3; ++r)
        for (int i = 0; i < cmid; ++i) bias3[r * cmid + i] = b[r * 32 + i];
    return ESR_OK;
}

int esr_asym_step_supported(const esr_conv_desc* d)
{
    if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0) return 0;
    if (!esr_s16_pair(d->storage, d->compute)) return 0;
    if (d->ksize != 3 || d->in_layout != ESR_NHWC || d->out_layout != ESR_NHWC) return 0;
    const int cmid = d->post_cout;                                                // logical channels of d, a_l, a_m and out
    if (cmid < 17 || cmid > 32 || d->cin < 17 || d->cin > 64) return 0;
    if (d->cout < cmid || d->cout > esr_round_up(cmid, 16)) return 0;             // channels of out stored, as esr_conv2d_f32's cout
    if (d->res_mode != ESR_RES_NONE && d->res_mode != ESR_RES_PRE_ACT) return 0;
    if (d->res_mode == ESR_RES_PRE_ACT && d->cin != cmid) return 0;               // the residual is the input
    if (d->act != ESR_ACT_NONE && d->act != ESR_ACT_LRELU && d->act != ESR_ACT_RELU) return 0;
    if (d->post_act != d->act) return 0;                                          // one activation for d, a_l, a_m and out
    if (d->split || d->tail_wpacked || d->tail_cat_c || d->tail_cout || d->tail_mid_act || d->tail_seg_stride16 || d->post2_wpacked || d->post2_out.ptr ||
        d->post2_cout || d->out1.ptr || d->border_bias || d->blocked8 || d->in_seg_stride || d->in_seg_chunks || d->wino_wpacked || d->hilo || d->hilo_stride) return 0;
    if (!esr_image_below_1g((double)d->h * d->w, d->in.pitch, 2)) return 0;
    if (esr_tiles(d->n, d->h, d->w, AS_T).count >= (double)ESR_INDEX_LIMIT) return 0;
    return 1;
}

int esr_asym_step(const esr_conv_desc* d, void* hip_stream)
{
    if (!d || !d->in.ptr || !d->out0.ptr || !d->post_out.ptr || !d->wpacked || !d->post_wpacked) return ESR_ERR_BAD_ARG;
    if (!esr_asym_step_supported(d)) return ESR_ERR_UNSUPPORTED;
    const int cmid = d->post_cout, c8 = esr_round_up(cmid, 8), y8 = esr_round_up(d->cout, 8);
    if (!esr_view_fits(d->in, 8, esr_round_up(d->cin, 8)) || !esr_view_fits(d->post_out, 8, c8) || !esr_view_fits(d->out0, 8, y8)) return ESR_ERR_BAD_ARG;
    if ((d->res.ptr && !esr_view_fits(d->res, 8, c8)) || (d->tail_cat.ptr && !esr_view_fits(d->tail_cat, 8, c8))) return ESR_ERR_BAD_ARG;
    // neither output's bytes meet `in` (the neighbouring tiles read its halo), p1 or p2 (an absent one: a null view meets nothing), or the other output
    const size_t npx = (size_t)d->n * d->h * d->w;
    const esr_view* ins[3] = {&d->in, &d->res, &d->tail_cat};
    const int in_c[3] = {esr_round_up(d->cin, 8), c8, c8};
    for (int i = 0; i < 3; ++i)
        if (esr_views_meet(d->out0, y8, *ins[i], in_c[i], npx, 2) || esr_views_meet(d->post_out, c8, *ins[i], in_c[i], npx, 2)) return ESR_ERR_BAD_ARG;
    if (esr_views_meet(d->out0, y8, d->post_out, c8, npx, 2)) return ESR_ERR_BAD_ARG;
    AsymK k;
    memset(&k, 0, sizeof(k));
    k.x = static_cast<const char*>(d->in.ptr);
    k.w1 = static_cast<const char*>(d->post_wpacked);
    k.wa = static_cast<const char*>(d->wpacked);
    k.p1 = static_cast<const char*>(d->res.ptr);
    k.p2 = static_cast<const char*>(d->tail_cat.ptr);
    k.d = static_cast<char*>(d->post_out.ptr);
    k.y = static_cast<char*>(d->out0.ptr);
    k.N = d->n; k.H = d->h; k.W = d->w;
    k.in_pitch = d->in.pitch; k.in_coff = d->in.coff;
    k.d_pitch = d->post_out.pitch; k.d_coff = d->post_out.coff;
    k.y_pitch = d->out0.pitch; k.y_coff = d->out0.coff;
    k.p1_pitch = d->res.pitch; k.p1_coff = d->res.coff;
    k.p2_pitch = d->tail_cat.pitch; k.p2_coff = d->tail_cat.coff;
    k.cin = d->cin; k.cmid = cmid;
    k.nch1 = esr_round_up(d->cin, 16) / 16;
    k.d_cout8 = c8; k.y_cout8 = y8;
    k.slope = esr_act_slope(d->act, d->slope);
    const esr_tile_grid tg = esr_tiles(d->n, d->h, d->w, AS_T);
    k.tiles_x = tg.tiles_x; k.tiles_y = tg.tiles_y; k.ntiles = (int)tg.count;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const bool bf16 = d->storage == ESR_STORE_BF16;
    if (d->res_mode == ESR_RES_PRE_ACT) return bf16 ? launch_asym<true, 1, true>(k, st) : launch_asym<false, 1, true>(k, st);
    if (d->cin > 32) return bf16 ? launch_asym<true, 2, false>(k, st) : launch_asym<false, 2, false>(k, st);
    return bf16 ? launch_asym<true, 1, false>(k, st) : launch_asym<false, 1, false>(k, st);
}

}  // extern "C"
