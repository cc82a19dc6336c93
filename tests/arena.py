"""One allocation, filled with a byte pattern, from which the operands of a call are carved (tests of the buffer contract
of include/flm.h: a call's result depends on nothing its buffers, or the memory beside them, held before).

    a = Arena(0xFF, [("x", nbytes, 16, True), ("ws", ws_bytes, 256), ("out", out_bytes, 16)], device="cuda")
    a.put("x", crops)                                   # the data of a read-only operand; kept for check_guards()
    model.forward_device(a.view("x", torch.uint8, crops.shape), ..., workspace=a.region("ws"), out_tensor=a.view("out", ...))
    a.check_guards()                                    # every byte outside the regions still holds the fill; "x" unchanged

A region is (name, bytes, alignment[, read_only]).  Its start lies at an offset that is `alignment` modulo twice the
alignment -- the alignment the header promises for the operand and no better, so that a kernel which quietly assumes more
(a 512-byte workspace, a 32-byte row) runs on an address it does not get for free from an allocator.  Every region has
GUARD bytes of fill on both sides: 4 MiB, more than one 128-row x 4096-column float32 tile, the largest single over-run a
tile kernel of this library could make.  Works on CPU tensors too (tests/test_arena_host.py).

The fills: 0x00, what a fresh page reads as; 0xFF, NaN as float32 and as bfloat16 and all ones as an integer; 0x4B, 1.33e7
as float32 and as bfloat16 -- fmaxf and the v_max forms swallow a NaN, so a NaN that leaks in before a ReLU comes out as
the 0 a fresh page gives, and only a large finite stray value shows there.
"""
import torch

FILLS = (0x00, 0x4B, 0xFF)   # the order of the cases: the fresh-page run first, it is the reference of the other two
GUARD = 4 << 20
_BASE_ALIGN = 512            # the arena's own start: twice the largest alignment a region may ask for


class Arena:
    def __init__(self, fill, regions, device="cpu", guard=GUARD):
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill is one byte")
        self.fill = int(fill)
        self.guard = int(guard)
        self._off = {}        # name -> (start, bytes)
        self._readonly = {}   # name -> copy of the data put() there (None until then)
        cur = self.guard
        for spec in regions:
            name, nbytes, align = spec[0], int(spec[1]), int(spec[2])
            if name in self._off:
                raise ValueError("region %r twice" % name)
            if nbytes < 1 or align < 1 or align & (align - 1) or 2 * align > _BASE_ALIGN:
                raise ValueError("region %r: %d bytes at alignment %d (a power of two up to %d)"
                                 % (name, nbytes, align, _BASE_ALIGN // 2))
            start = cur + (align - cur) % (2 * align)     # the first offset >= cur that is `align` modulo 2 * align
            self._off[name] = (start, nbytes)
            if len(spec) > 3 and spec[3]:
                self._readonly[name] = None
            cur = start + nbytes + self.guard
        self.nbytes = cur
        raw = torch.empty(self.nbytes + _BASE_ALIGN, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % _BASE_ALIGN
        self._raw = raw                                   # (keeps the allocation alive)
        self.buf = raw[skip:skip + self.nbytes]
        self.buf.fill_(self.fill)

    def offset(self, name):
        return self._off[name][0]

    def region(self, name):
        """The region as a uint8 view of the arena."""
        start, nbytes = self._off[name]
        return self.buf[start:start + nbytes]

    def view(self, name, dtype, shape):
        """The region's first bytes as a contiguous tensor of `dtype` and `shape`."""
        numel = 1
        for s in shape:
            numel *= int(s)
        nb = numel * torch.empty((), dtype=dtype).element_size()
        if nb > self._off[name][1]:
            raise ValueError("region %r holds %d bytes, %s %s needs %d" % (name, self._off[name][1], dtype, tuple(shape), nb))
        return self.region(name)[:nb].view(dtype).view(tuple(shape))

    def put(self, name, data):
        """Copy `data` (a tensor or a numpy array) to the start of the region; returns the view that now holds it.  A
        read-only region remembers the bytes for check_guards()."""
        t = data if isinstance(data, torch.Tensor) else torch.from_numpy(data)
        t = t.contiguous()
        v = self.view(name, t.dtype, t.shape)
        v.copy_(t)
        if name in self._readonly:
            self._readonly[name] = self.region(name).clone()
        return v

    def gaps(self):
        """The (start, end) byte ranges that belong to no region: the guards and the alignment slack."""
        out, cur = [], 0
        for start, nbytes in sorted(self._off.values()):
            out.append((cur, start))
            cur = start + nbytes
        out.append((cur, self.nbytes))
        return out

    def check_guards(self):
        """Every byte outside the regions still holds the fill, and every read-only region the bytes put() there."""
        for lo, hi in self.gaps():
            g = self.buf[lo:hi]
            if not torch.equal(g, torch.full_like(g, self.fill)):
                bad = torch.nonzero(g != self.fill).flatten()
                first, last = lo + int(bad[0]), lo + int(bad[-1])
                near = min(self._off.items(), key=lambda kv: min(abs(first - kv[1][0]), abs(first - kv[1][0] - kv[1][1])))
                raise AssertionError("fill 0x%02X: %d guard bytes changed, arena offsets %d .. %d (nearest region %r at %d .. %d)"
                                     % (self.fill, bad.numel(), first, last, near[0], near[1][0], near[1][0] + near[1][1]))
        for name, snap in self._readonly.items():
            if snap is not None and not torch.equal(self.region(name), snap):
                raise AssertionError("fill 0x%02X: read-only region %r changed" % (self.fill, name))


def same_bits(a, b):
    """Equality of two tensors bit for bit (so NaN equals the same NaN, and -0.0 differs from 0.0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
