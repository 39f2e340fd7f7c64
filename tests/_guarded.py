"""A guarded arena for the "stays inside its declared views" tests (tests/test_gpu_bounds.py; DESIGN.md "Bounds").

The kernels get zero padding and edge clipping from buffer resources whose size is one image's bytes, tensors live back to back in the
engine's workspace, and a test that lets every op allocate fresh tensors cannot see a read or a write that leaves its tensor: the memory
behind a fresh tensor is usually zero.  The arena carves every tensor of one launch out of ONE flat allocation per dtype,

    [guard | tensor | guard  guard | tensor | guard  guard | ...]         (every tensor owns the guard before and the guard behind it)

so that what lies next to a tensor is chosen by the test:
  * the guards of an INPUT hold the arena's `fill`: "nan", "big" (3e4: finite in f16 and bf16) or "noise" (seeded, finite);
  * the guards of an OUTPUT hold a fixed bit pattern (SENTINEL bytes), and so does every byte of the output buffer itself; the caller
    declares which part of the buffer the launch may write (`writable`), everything else must keep its bits.
check_untouched() compares every byte the launch may not write -- guards, inputs, the undeclared parts of outputs -- bit for bit through
a uint8 view with a snapshot taken before the launch, and names the first byte that changed as (tensor, image, row, column, channel).

Tensor starts are 256-byte aligned (what the caching allocator gives the kernels); a guard is at least 18 rows of its tensor (one 16-row
tile plus its halo) and at least 64 KiB.  The device may be "cpu": the helper's own tests run without a GPU."""
import torch

ALIGN = 256
GUARD_ROWS = 18
GUARD_MIN_BYTES = 64 * 1024
SENTINEL = 0xA5                  # every byte of an output buffer and of its guards before the launch (a finite value in every float type)
FILLS = ("nan", "big", "noise")
BIG = 3.0e4


def _round_up(v, m):
    return (v + m - 1) // m * m


class Untouched(AssertionError):
    """a byte outside the declared views changed; .where = (tensor name, image, row, column, channel), .region = 'guard before' | ..."""

    def __init__(self, msg, where, region):
        super().__init__(msg)
        self.where, self.region = where, region


class _Slot:
    def __init__(self, name, shape, dtype, kind, data, writable, row=None):
        self.name, self.shape, self.dtype, self.kind, self.data, self.writable = name, tuple(shape), dtype, kind, data, writable
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.numel = 1
        for s in self.shape:
            self.numel *= s
        if row is None:                                     # one image row: w * pitch elements
            row = (self.shape[-2] if len(self.shape) >= 2 else 1) * self.shape[-1]
        self.guard = _round_up(max(GUARD_ROWS * row * self.es, GUARD_MIN_BYTES), ALIGN)          # bytes
        self.start = None                                   # byte offset of the tensor inside its dtype's allocation

    @property
    def nbytes(self):
        return self.numel * self.es

    def coords(self, lin):
        """element offset from the tensor's start (negative: in the guard before it; >= numel: behind it) -> (image, row, column, channel);
        the last three dims are (h, w, pitch), everything in front of them counts images (an NCHW tensor: image = n, then plane, row,
        column)"""
        h, w, p = ((1, 1, 1) + self.shape)[-3:]
        img, rem = divmod(lin, h * w * p)
        row, rem = divmod(rem, w * p)
        col, ch = divmod(rem, p)
        return img, row, col, ch


class Arena:
    def __init__(self, device="cpu", fill="nan", seed=0):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}")
        self.device, self.fill, self.seed = torch.device(device), fill, seed
        self.slots, self.tensors, self._bufs = [], {}, {}

    # ---- declaration -----------------------------------------------------------------------------------------------------------
    def add_input(self, name, data, row=None):
        """`data`: the whole buffer (a CPU tensor, pitch and foreign channels included) as the launch will see it.  row: elements of one
        image row (w * pitch) where the last two dims are not (w, pitch) -- a channel-blocked [N, C/8, H, W, 8] tensor: w * C"""
        self._add(_Slot(name, data.shape, data.dtype, "in", data, None, row))

    def add_output(self, name, shape, dtype, writable="all", row=None):
        """row: as add_input.  writable: "all" | None (the launch stores nothing here) | (dim, start, length): the index range of ONE dim the launch may write
        (an NHWC view: (-1, coff, round_up(cout, granule)))"""
        if writable not in ("all", None):
            dim, start, length = writable
            dim %= len(shape)
            if not (0 <= start and length > 0 and start + length <= shape[dim]):
                raise ValueError(f"{name}: writable range [{start}, {start + length}) outside dim {dim} of {tuple(shape)}")
            writable = (dim, start, length)
        self._add(_Slot(name, shape, dtype, "out", None, writable, row))

    def _add(self, slot):
        if self.tensors:
            raise RuntimeError("the arena is built")
        if any(s.name == slot.name for s in self.slots):
            raise ValueError(f"two tensors named {slot.name}")
        self.slots.append(slot)

    # ---- layout ----------------------------------------------------------------------------------------------------------------
    def build(self):
        by_dtype = {}
        for s in self.slots:
            by_dtype.setdefault(s.dtype, []).append(s)
        for k, (dtype, slots) in enumerate(by_dtype.items()):
            es = slots[0].es
            off = 0
            for s in slots:
                s.start = off + s.guard                                       # guard before | tensor | guard behind, up to the next 256
                off = _round_up(s.start + s.nbytes + s.guard, ALIGN)
                s.end_guard = off                                             # byte offset where the guard behind the tensor ends
            raw = torch.empty(off + ALIGN, dtype=torch.uint8, device=self.device)
            shift = (-raw.data_ptr()) % ALIGN                                 # (the CPU allocator aligns to 64 bytes only)
            buf = raw[shift:shift + off]
            expect = torch.empty(off, dtype=torch.uint8)
            g = torch.Generator().manual_seed(1000 * self.seed + k)
            for s in slots:
                lo, hi = s.start - s.guard, s.end_guard
                if s.kind == "out":
                    expect[lo:hi] = SENTINEL
                else:
                    expect[lo:hi] = self._guard_bytes(dtype, (hi - lo) // es, g)
                    expect[s.start:s.start + s.nbytes] = s.data.contiguous().reshape(-1).view(torch.uint8)
            buf.copy_(expect)
            mask = torch.ones(off, dtype=torch.bool)                          # True: the launch may not change this byte
            for s in slots:
                if s.kind == "out" and s.writable is not None:
                    m = torch.ones(s.shape, dtype=torch.bool)
                    if s.writable == "all":
                        m[...] = False
                    else:
                        dim, start, length = s.writable
                        m.narrow(dim, start, length).fill_(False)
                    mask[s.start:s.start + s.nbytes] = m.reshape(-1).repeat_interleave(es)
                self.tensors[s.name] = buf[s.start:s.start + s.nbytes].view(dtype).view(s.shape)
            self._bufs[dtype] = (raw, buf, expect, mask, slots)
        return self

    def _guard_bytes(self, dtype, n, g):
        if dtype.is_floating_point:
            if self.fill == "nan":
                t = torch.full((n,), float("nan"), dtype=dtype)
            elif self.fill == "big":
                t = torch.full((n,), BIG, dtype=dtype)
            else:
                t = (torch.randn(n, generator=g) * 3.0).to(dtype)
        else:                                               # integer storage (uint8 images): there is no NaN; the extremes and noise
            info = torch.iinfo(dtype)
            if self.fill == "nan":
                t = torch.full((n,), info.max, dtype=dtype)
            elif self.fill == "big":
                t = torch.full((n,), info.max // 2 + 1, dtype=dtype)
            else:
                t = torch.randint(0, 256, (n,), generator=g).to(dtype)
        return t.view(torch.uint8)

    def __getitem__(self, name):
        return self.tensors[name]

    def written(self, name):
        """a copy of the declared writable part of an output"""
        s = next(s for s in self.slots if s.name == name)
        t = self.tensors[name]
        if s.writable is None:
            raise KeyError(f"{name} is declared as not stored")
        return (t if s.writable == "all" else t.narrow(*s.writable)).clone()

    # ---- the check -------------------------------------------------------------------------------------------------------------
    def check_untouched(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for dtype, (_, buf, expect, mask, slots) in self._bufs.items():
            bad = (buf.cpu() != expect) & mask
            if not bool(bad.any()):
                continue
            at = int(torch.nonzero(bad.view(-1))[0])
            s = next(s for s in slots if at < s.end_guard)
            lin = (at - s.start) // s.es                    # floor: a byte of the guard before the tensor has a negative element offset
            region = "guard before" if at < s.start else ("guard behind" if at >= s.start + s.nbytes else
                                                          ("input" if s.kind == "in" else "outside the declared view"))
            where = (s.name,) + s.coords(lin)
            raise Untouched(f"{s.name} ({s.kind}put {tuple(s.shape)} {dtype}): byte {at - s.start:+d} from the tensor's start changed "
                            f"({region}): image {where[1]}, row {where[2]}, column {where[3]}, channel {where[4]}; "
                            f"{int(bad.sum())} bytes changed in this allocation", where, region)
