// shared by the translation units of libesr_hip.so (not part of the public ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "esr_hip.h"

void esr_set_err(const char* what, hipError_t e);
int esr_check_launch(const char* what);

// Opt-in of one kernel instantiation to more than 64 KB of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize).  The attribute
// belongs to the (device, instantiation) pair: one process may drive several GPUs (engine contexts are keyed by device), so a launcher
// keeps one `static esr_lds_optin_flags` per instantiation and calls esr_lds_optin before it launches.  Relaxed atomics: a racing
// thread at worst sets the same value twice.  A failure is recorded as "hipFuncSetAttribute(<name>, MaxDynamicSharedMemorySize)"
// and returns ESR_ERR_LAUNCH.
constexpr int MAX_DEVICES = 64;
struct esr_lds_optin_flags { std::atomic<unsigned> set[MAX_DEVICES]; };
int esr_lds_optin(esr_lds_optin_flags& flags, const void* kernel, int bytes, const char* name);

// Persistent launches: min(work items, resident blocks).  The LDS footprint of a kernel decides how many of its blocks a CU holds.
constexpr int ESR_BLOCKS_1_PER_CU = 256, ESR_BLOCKS_2_PER_CU = 512;      // 256 CUs
static inline int esr_persistent_grid(int ntiles, int cap) { return ntiles < cap ? ntiles : cap; }

// fp32 -> bf16 / fp16 and back on the host, as the kernels' conversions: round to nearest even, a NaN is quietened.  THE rounding of
// every weight packer (a fused kernel is bit-identical to the launches it replaces only if their packers round alike).  `fmt` is an
// ESR_COMPUTE_* or an ESR_STORE_* value: the two enums agree on the 16-bit formats.
static_assert((int)ESR_COMPUTE_BF16 == (int)ESR_STORE_BF16 && (int)ESR_COMPUTE_F16 == (int)ESR_STORE_F16, "esr_host_to16: one fmt for both enums");
static inline uint16_t esr_host_to16(float f, int fmt)
{
    uint16_t r;
    if (fmt == ESR_COMPUTE_BF16) {
        uint32_t u;
        memcpy(&u, &f, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);       // NaN
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
    const _Float16 h = (_Float16)f;        // host compiler: IEEE RNE
    memcpy(&r, &h, 2);
    return r;
}
static inline float esr_host_from16(uint16_t h, int fmt)
{
    if (fmt == ESR_COMPUTE_BF16) {
        const uint32_t u = (uint32_t)h << 16;
        float f;
        memcpy(&f, &u, 4);
        return f;
    }
    _Float16 v;
    memcpy(&v, &h, 2);
    return (float)v;
}
// Records the device symbol of the launch that follows, as rocprofv3 prints it -- only while esr_run_ops_profiled runs (a bench /
// profile leg names its kernels by the symbol that really ran: esr_prof_kernel_symbol).  printf-style.
void esr_note_kernel(const char* fmt, ...);
static inline const char* esr_tf(bool b) { return b ? "true" : "false"; }
static inline int esr_round_up(int v, int m) { return (v + m - 1) / m * m; }

// THE acceptance tests of a declared tensor view (tests/test_view_validation.py sweeps every launcher's).  `granule` is 4 channels for
// fp32 views (16-byte lanes) and 8 for 16-bit ones, a power of two; `channels` is what the kernel touches from coff on -- the stored
// count rounded up to the granule, or less than the K chunks under the tight pitch (esr_conv2d_s16).  _aligned: pitch and coff are whole
// granules; _fits: and the slice lies inside the pixel; _ok: and the pointer is set (where no earlier check has looked at it)
static inline bool esr_view_aligned(const esr_view& v, int granule) { return !(v.pitch & (granule - 1)) && !(v.coff & (granule - 1)); }
static inline bool esr_view_fits(const esr_view& v, int granule, int channels) { return esr_view_aligned(v, granule) && v.coff + channels <= v.pitch; }
static inline bool esr_view_ok(const esr_view& v, int granule, int channels) { return v.ptr && esr_view_fits(v, granule, channels); }

// Raw buffers address 2 GiB: the byte size of ONE IMAGE of a view the kernel reads or writes through a buffer resource
// (pixels x pitch x element size) stays below it, as does whatever a kernel holds in a 32-bit int -- element offsets over the whole
// batch (esr_fits_raw with elem_bytes = 1), tile, job and pixel counts (ESR_INDEX_LIMIT)
constexpr double ESR_RAW_LIMIT = 2147483647.0;
constexpr long long ESR_INDEX_LIMIT = 2147483647LL;
static inline bool esr_fits_raw(double pixels, int pitch, int elem_bytes) { return pixels * pitch * elem_bytes < ESR_RAW_LIMIT; }

// The fused 16-bit kernels address a tiled view with 32-bit BYTE offsets inside one image and ADD an out-of-range marker (0x80000000,
// esr_chain also 0x40000000) to the offset of a lane or a row that lies outside the image: one image of such a view (pixels x pitch x
// element size) stays below 1 GiB, not 2, so that no sum with a marker in it wraps to a valid offset
constexpr double ESR_IMAGE_LIMIT = 1073741824.0;
static inline bool esr_image_below_1g(double pixels, int pitch, int elem_bytes) { return pixels * pitch * elem_bytes < ESR_IMAGE_LIMIT; }

// The T x T output tiles of a launch: a predicate holds `count` below ESR_INDEX_LIMIT, after which its launcher's ntiles is (int)count
struct esr_tile_grid { int tiles_x, tiles_y; double count; };
static inline esr_tile_grid esr_tiles(int n, int h, int w, int T)
{
    const int tx = (w + T - 1) / T, ty = (h + T - 1) / T;
    return {tx, ty, (double)n * tx * ty};
}

// 16-bit storage (`fmt` is an ESR_STORE_* or an ESR_COMPUTE_* value: the two enums agree on the 16-bit formats, static_assert above), and
// the rule of the fused 16-bit kernels: 16-bit storage, and the MFMA operand type is the storage type
static inline bool esr_is_s16(int fmt) { return fmt == ESR_STORE_BF16 || fmt == ESR_STORE_F16; }
static inline bool esr_s16_pair(int storage, int compute) { return esr_is_s16(storage) && compute == storage; }

// Do the byte ranges [a, a + an) and [b, b + bn) meet?  A null pointer meets nothing.
static inline bool esr_bytes_overlap(const char* a, size_t an, const char* b, size_t bn) { return a && b && a < b + bn && b < a + an; }

// Does a byte that a launch WRITES through view `o` (channels [coff, coff + oc) of each of `npx` pixels, pad slots up to the granule included)
// belong to what it READS through view `i` (channels [coff, coff + ic))?  A view's ptr is its tensor's base (coff lies inside the pitch), so a
// tensor is the npx * pitch elements behind it.  Two views of one pixel grid -- the same pitch, their first pixels a whole number of pixels
// apart -- meet only where their channel ranges do (slices of one concat tensor); any other pair meets wherever the tensors' byte ranges
// do.  A null pointer on either side meets nothing.
static inline bool esr_views_meet(const esr_view& o, int oc, const esr_view& i, int ic, size_t npx, int elem_bytes)
{
    const char* ob = static_cast<const char*>(o.ptr);
    const char* ib = static_cast<const char*>(i.ptr);
    if (!esr_bytes_overlap(ob, npx * o.pitch * elem_bytes, ib, npx * i.pitch * elem_bytes)) return false;
    if (o.pitch != i.pitch || ((ob - ib) % ((ptrdiff_t)o.pitch * elem_bytes)) != 0) return true;
    return o.coff < i.coff + ic && i.coff < o.coff + oc;
}

// "the residual is the input": a pre-activation residual over the view the conv reads, which the kernel then adds from its staged input
// tile.  `chunk`: the channel counts agree after rounding up to it -- 16 for the 16-bit kernels (K chunks), 1 for the fp32 ones
static inline bool esr_res_is_input(const esr_conv_desc* d, int chunk)
{
    return d->res_mode == ESR_RES_PRE_ACT && esr_round_up(d->cin, chunk) == esr_round_up(d->cout, chunk) && d->res.ptr == d->in.ptr &&
           d->res.pitch == d->in.pitch && d->res.coff == d->in.coff;
}

// the slope a kernel's max(v, slope * v) epilogue takes: LeakyReLU's own, 0 for ReLU, 1 for every other activation (identity)
static inline float esr_act_slope(int act, float slope) { return act == ESR_ACT_LRELU ? slope : (act == ESR_ACT_RELU ? 0.f : 1.f); }

// esr_s16.hip: NHWC convolution on 16-bit storage (called by esr_conv2d_f32 when d->storage != ESR_STORE_F32)
int esr_conv2d_s16(const esr_conv_desc* d, void* hip_stream);
int esr_s16_block_waves(const esr_conv_desc* d);      // 4: two 4-wave blocks per CU (16 x 16 tiles), 8: one 8-wave block (16 x 32)

// esr_hfab.hip: FMEN's HFAB as one launch (esr_conv_chain_s16 with res_mode ESR_RES_GATE; esr_conv_chain_supported asks the first)
int esr_hfab_supported(const esr_chain_desc* d);
int esr_hfab_s16(const esr_chain_desc* d, void* hip_stream);

// esr_esa_pool7.hip: EFDN's ESA branch -- esr_esa_lowres_f32 with w_s2 == NULL (max_pool2d(7, 7, padding 1) + the parallel pair + conv_23)
int esr_esa_pool7_lowres(const esr_esa_lowres_desc* d, void* hip_stream);

// esr_wino.hip: Winograd F(2x2, 3x3) fp32 convolution (called by esr_conv2d_f32 when d->wino_wpacked is set and the shape qualifies)
int esr_conv2d_wino(const esr_conv_desc* d, void* hip_stream);

// esr_graph.hip: while esr_graph_create captures an op list, a launcher whose kernel can read the network input or write the network
// output reports the launch it has JUST enqueued on `st`: the pointer values it passed and their byte offsets inside the kernel's first
// argument (offsetof in the parameter struct; 0 for a leading scalar pointer argument).  No-op outside a capture.
void esr_graph_note_io(hipStream_t st, const void* in_ptr, size_t in_off, const void* out_ptr, size_t out_off);

#ifdef __HIPCC__
// gfx950 erratum found in round 4 (LAB_NOTES.md "packed fp32 op_sel"; tools/dbg/pk_opsel_probe.hip reproduces it in isolation): a
// packed fp32 VALU instruction whose op_sel makes a result half read the HIGH dword of a 64-bit source pair (v_pk_mul_f32 ...
// op_sel:[0,1]) returns 0 in lanes 48..63 when a wave of ANOTHER kernel issues MFMAs on the same SIMD -- forwards overlapping on
// several HIP streams differed from serial ones.  hipcc picks that encoding when a scalar factor happens to live in the odd
// register of a pair (an .y / .w element of a loaded vector, or lx next to ly in a struct).  esr_lone() gives the factor a register
// of its own, so the broadcast is encoded with op_sel_hi (both halves read the LOW dword: the form that never failed);
// tools/lint_isa.py (a CPU test) fails the build if the bad encoding shows up in any kernel of the library.
__device__ __forceinline__ float esr_lone(float v)
{
    asm("" : "+v"(v));
    return v;
}

// ESR_RES_GATE: y = sigmoid(v) * r.  The ONE expression of the sigmoid: every kernel that implements the gate (conv_f32_kernel,
// conv_s16_kernel, hfab_kernel) calls this, so the fused HFAB is bit-identical to its per-layer launches
__device__ __forceinline__ float esr_sigmoid(float v)
{
    return 1.f / (1.f + expf(-v));
}

// GELU of the 16-bit storage modes (the scalar definition conv_s16_kernel's packed version follows bit for bit -- held by
// tests/test_gpu_value_sweep.py over every 16-bit value; accuracy and derivation: esr_s16_dev.h, tools/fit_gelu.py: |error| <= 1.3e-4 on
// [-4, 4], 5.33e-5 x above, 2.13e-4 below -4)
__device__ __forceinline__ float esr_gelu16(float x)
{
    const float xc = fminf(fmaxf(x, -4.f), 4.f);
    const float t = xc * xc;
    float p = -1.580786198e-09f;
    p = fmaf(p, t, 1.217111051e-07f);
    p = fmaf(p, t, -4.100866386e-06f);
    p = fmaf(p, t, 8.066739505e-05f);
    p = fmaf(p, t, -1.048204400e-03f);
    p = fmaf(p, t, 9.664874174e-03f);
    p = fmaf(p, t, -6.617537882e-02f);
    p = fmaf(p, t, 3.988475079e-01f);
    return fmaxf(x, -4.f) * fmaf(xc, p, 0.5f);
}
#endif
