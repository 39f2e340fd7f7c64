"""Byte patterns for the "a plan's result does not depend on what its workspace held before" tests (tests/test_gpu_stale_workspace.py;
DESIGN.md 2c).

The engine keeps ONE grow-only workspace per stream and never re-zeroes it between the plans of different shapes
(engine.HipSRModel.rezero_on_switch): a plan's pad channels, halo rows and not-yet-written buffers hold whatever another shape's forward
left there -- FINITE values of the SAME element type, because the fp32 low-resolution maps of all plans live in an arena of their own in
front of the full-resolution buffers.  The patterns here are the hostile version of such leftovers, written over the WHOLE workspace:

  * constant bytes (BYTES), finite in every element type, so they need no knowledge of the arena boundary:
        0x3C   fp16 1.0586       bf16 / fp32 ~ 0.0115
        0x77   fp16 30576        bf16 / fp32 ~ 5.0e33
        0xF7   fp16 -32624       bf16 / fp32 ~ -1.0e34      (0x77 with the sign bit set in every byte)
  * typed noise: fp32 values in the low-resolution arena (the first `lo_cap` bytes), values of the plan's storage type behind it, both
    randn * 100 rounded to the type, seeded.

Everything is built on the CPU as a uint8 tensor of the workspace's size; the device may stay out of it (tests/test_poison_helper.py)."""
import torch

BYTES = (0x3C, 0x77, 0xF7)
NOISE_SCALE = 100.0
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PATTERNS = tuple(f"0x{b:02X}" for b in BYTES) + ("noise",)


def constant_bytes(nbytes, byte):
    """`nbytes` copies of `byte`"""
    assert 0 <= byte <= 255
    return torch.full((nbytes,), byte, dtype=torch.uint8)


def typed_noise(nbytes, lo_cap, store, seed=0):
    """fp32 randn * 100 in bytes [0, lo_cap), randn * 100 rounded to `store` behind them; a tail shorter than one element holds BYTES[0]"""
    dt = DTYPES[store]
    es = torch.empty(0, dtype=dt).element_size()
    lo_cap = min(lo_cap, nbytes)
    assert lo_cap % 4 == 0, lo_cap
    g = torch.Generator().manual_seed(seed)
    out = torch.full((nbytes,), BYTES[0], dtype=torch.uint8)
    out[:lo_cap] = (torch.randn(lo_cap // 4, generator=g) * NOISE_SCALE).view(torch.uint8)
    n_hi = (nbytes - lo_cap) // es
    out[lo_cap:lo_cap + n_hi * es] = (torch.randn(n_hi, generator=g) * NOISE_SCALE).to(dt).view(torch.uint8)
    return out


def pattern(name, nbytes, lo_cap, store, seed=0):
    """one of PATTERNS as `nbytes` bytes"""
    if name == "noise":
        return typed_noise(nbytes, lo_cap, store, seed)
    return constant_bytes(nbytes, int(name, 16))


def typed_views(data, lo_cap, store):
    """(fp32 view of the low-resolution arena's bytes, `store` view of the whole elements behind it) of a byte pattern"""
    dt = DTYPES[store]
    es = torch.empty(0, dtype=dt).element_size()
    lo_cap = min(lo_cap, data.numel())
    n_hi = (data.numel() - lo_cap) // es
    return data[:lo_cap].view(torch.float32), data[lo_cap:lo_cap + n_hi * es].view(dt)


def buffer_ranges(plan, lo_cap):
    """[(buffer name, first byte, bytes)] of a Plan's buffers inside a workspace whose low-resolution arena is `lo_cap` bytes: what
    engine._addr resolves, with the 256-byte rounding of Plan.buffer.  For locating which buffer lets stale content through."""
    out = []
    for b in plan.buffers:
        size = (plan.n * b.h * b.w * b.pitch * b.esize + 255) // 256 * 256
        out.append((b.name, b.offset if b.arena == 1 else lo_cap + b.offset, size))
    return out


def poison_range(ws, data, start, nbytes):
    """copy bytes [start, start + nbytes) of the pattern `data` into the workspace `ws` (a uint8 tensor on any device), nothing else"""
    ws[start:start + nbytes].copy_(data[start:start + nbytes])
