"""Write-footprint helpers: poisoned buffers with guard bands around them.

A kernel test that only compares the values inside the declared output cannot see a store that never happened (the
buffer already held the answer), a store outside the output, a result that depends on memory outside the declared
operands, or a modified input.  ``Guarded`` allocates ``[front guard | rows x ld elements | back guard]`` in ONE flat
byte buffer the test owns, fills all of it -- the guards and the ``ld - cols`` gap of every row included -- with a
poison pattern, and afterwards compares every byte outside the payload with that pattern, bit for bit.  Nothing here
reads or writes outside an allocation.  Works on CPU and CUDA tensors alike; plain module, no pytest configuration.
"""
import contextlib

import torch

ALIGN = 4096          # the payload's base alignment (the C ABI wants 16-byte bases)

# Two poison patterns per element size / kind.  Floats: NaNs with distinct payloads; integers: two fixed constants.
_POISON_BITS = {
    torch.float32: (0x7FC0DEAD, 0x7FE0BEEF),
    torch.bfloat16: (0x7FDE, 0x7FBE),
    torch.float16: (0x7DAD, 0x7EEF),
    torch.float64: (0x7FF8DEADDEADDEAD, 0x7FFCBEEFBEEFBEEF),
    torch.int16: (0x6B5A, 0x1C2D),
    torch.int32: (0x6B5A3C1D, 0x1C2D4E7F),
    torch.int64: (0x6B5A3C1D2E4F7081, 0x1C2D4E7F50617283),
    torch.uint8: (0xA5, 0x5A),
    torch.int8: (0x65, 0x5A),
}
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
N_PATTERNS = 2


def poison_bits(dtype, pattern):
    """The poison element of ``dtype`` for pattern 0 | 1, as an unsigned integer."""
    return _POISON_BITS[dtype][pattern]


def _signed(bits, size):
    return bits - (1 << (8 * size)) if size > 1 and bits >= 1 << (8 * size - 1) else bits


def bits_of(t):
    """``t`` (any strides) as a contiguous integer tensor of the same element size: the view bit comparisons go through."""
    t = t.detach()
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    return t.contiguous().view(_INT_OF_SIZE[t.element_size()])


def poison_scalar(dtype, pattern):
    """The poison element as a value of the integer view ``bits_of`` gives for ``dtype``."""
    return _signed(poison_bits(dtype, pattern), torch.empty((), dtype=dtype).element_size())


class Guarded:
    """One flat byte buffer ``[front guard | rows x ld elements | back guard]``, the payload base ALIGN-byte aligned.

    ``shape`` = (rows, cols) or (n,) (one row).  ``mask`` (optional, bool [rows, cols]): which elements of the view are
    payload -- the rest (plane gaps, rows a contract leaves untouched) count as gap and must keep the poison.
    ``.view`` is the [rows, cols] strided view (or the [n] vector) to hand to the kernels; ``.flat`` the rows x ld
    elements behind it."""

    def __init__(self, shape, dtype, device, ld=None, guard_bytes=4096, pattern=0, mask=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.one_d = len(shape) == 1
        self.rows, self.cols = (1, shape[0]) if self.one_d else shape
        self.dtype, self.device = dtype, torch.device(device)
        self.ld = self.cols if ld is None else int(ld)
        if self.ld < self.cols or self.rows < 1 or self.cols < 1:
            raise ValueError("Guarded: need rows, cols >= 1 and ld >= cols")
        self.es = torch.empty((), dtype=dtype).element_size()
        if guard_bytes < 16 or guard_bytes % 16:
            raise ValueError("Guarded: guard_bytes must be a positive multiple of 16")
        self.guard_bytes = int(guard_bytes)
        self.payload_bytes = self.rows * self.ld * self.es
        total = self.guard_bytes + self.payload_bytes + self.guard_bytes + ALIGN
        self.raw = torch.empty(total, dtype=torch.uint8, device=self.device)
        base = self.raw.data_ptr()
        self.start = (base + self.guard_bytes + ALIGN - 1) // ALIGN * ALIGN - base       # byte offset of the payload
        self.end = self.start + self.payload_bytes
        # (everything in front of the payload is front guard: the alignment slack too -- it is ours, and it is checked)
        self.lo = self.start % self.es                       # element-aligned window of the raw buffer
        n_el = (total - self.lo) // self.es
        self.elems = self.raw[self.lo:self.lo + n_el * self.es].view(dtype)
        e0 = (self.start - self.lo) // self.es
        self.flat = self.elems[e0:e0 + self.rows * self.ld].view(self.rows, self.ld)
        v = self.flat[:, :self.cols]
        self.view = v[0] if self.one_d else v
        assert self.view.data_ptr() % ALIGN == 0
        # outside[b]: byte b of the raw buffer is NOT payload
        inside = torch.zeros((self.rows, self.ld), dtype=torch.bool, device=self.device)
        if mask is None:
            inside[:, :self.cols] = True
        else:
            mask = torch.as_tensor(mask, dtype=torch.bool, device=self.device).reshape(self.rows, self.cols)
            inside[:, :self.cols] = mask
        self.inside = inside
        self.rect = mask is None
        outside = torch.ones(total, dtype=torch.bool, device=self.device)
        outside[self.start:self.end] = ~inside.reshape(-1).repeat_interleave(self.es)
        self.outside = outside
        self.pattern = None
        self.rearm(pattern)

    # ---- poison --------------------------------------------------------------------------------------------------
    def _expected(self, pattern):
        """the raw buffer's bytes if every element held the poison (phase-locked to the payload base)"""
        b = poison_bits(self.dtype, pattern)
        el = torch.tensor([(b >> (8 * i)) & 0xFF for i in range(self.es)], dtype=torch.uint8, device=self.device)
        n = self.raw.numel()
        rep = el.repeat(n // self.es + 2)
        off = (self.es - self.lo) % self.es
        return rep[off:off + n]

    def rearm(self, pattern):
        """Re-poison everything, the payload too, for the next launch."""
        self.pattern = int(pattern) % N_PATTERNS
        self.raw.copy_(self._expected(self.pattern))
        return self

    def fill_from(self, t):
        """Copy operand data into the payload only (``t`` of the view's shape; with a mask: the masked elements)."""
        t = torch.as_tensor(t).to(device=self.device, dtype=self.dtype).reshape(self.rows, self.cols)
        tgt = self.flat[:, :self.cols]
        if self.rect:
            tgt.copy_(t)
        else:
            m = self.inside[:, :self.cols]
            tgt[m] = t[m]
        return self

    # ---- checks --------------------------------------------------------------------------------------------------
    def payload(self):
        """A copy of the payload: [rows, cols] (or [n]); with a mask, the masked elements as a vector."""
        v = self.flat[:, :self.cols]
        if not self.rect:
            return v[self.inside[:, :self.cols]].clone()
        return (v[0] if self.one_d else v).clone()

    def locate(self, byte):
        """(zone, description) of a byte offset of the raw buffer."""
        if byte < self.start:
            return "front guard", "%d bytes before the payload (element %d before it)" % (
                self.start - byte, (self.start - byte + self.es - 1) // self.es)
        if byte >= self.end:
            return "back guard", "%d bytes past the payload's end (element %d after it)" % (
                byte - self.end, (byte - self.end) // self.es)
        e = (byte - self.start) // self.es
        r, c = divmod(e, self.ld)
        zone = "row gap" if c >= self.cols else "masked-out element"
        return zone, "row %d, column %d (cols %d, ld %d)" % (r, c, self.cols, self.ld)

    def assert_guards_intact(self, name="buffer"):
        """Every byte outside the payload still holds the poison: front, back and row gaps, bit for bit."""
        bad = (self.raw != self._expected(self.pattern)) & self.outside
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0].item())
            zone, where = self.locate(first)
            raise AssertionError("%s: write outside the payload in the %s: byte offset %d, %s; %d bytes differ in all"
                                 % (name, zone, first - self.start, where, int(bad.sum().item())))


def poison_(t, pattern):
    """Fill a plain tensor (any dtype of the table above, unit inner stride) with poison pattern 0 | 1 in place: the ``rearm``
    of an output that needs no guard band (one fill per relaunch)."""
    v = t.detach()
    if v.dtype not in _INT_OF_SIZE.values() or v.dtype == torch.int8:
        v = v.view(_INT_OF_SIZE[v.element_size()])
    v.fill_(poison_scalar(t.dtype, int(pattern) % N_PATTERNS))
    return t


def poisoned(*size, dtype=None, device=None, pattern=0):
    """``torch.empty`` whose contents are the poison of ``pattern``: a kernel output that no launch stored into cannot hold
    an earlier result the caching allocator left in the block."""
    t = torch.empty(*size, dtype=dtype, device=device)
    return poison_(t, pattern) if t.dtype in _POISON_BITS and t.numel() else t


def poisoned_like(t, pattern=0):
    return poisoned(t.shape, dtype=t.dtype, device=t.device, pattern=pattern)


def _as_dict(p):
    if isinstance(p, dict):
        return p
    if isinstance(p, torch.Tensor):
        return {"out": p}
    return {"out%d" % i: t for i, t in enumerate(p)}


def assert_fully_written(run):
    """``run(pattern)`` launches into outputs armed with poison pattern ``pattern`` (0 | 1) and returns their payloads (a
    tensor, a sequence or a dict of tensors).  Requires the two runs' payloads bit-identical through an integer view (a
    NaN the kernel wrote on purpose compares equal; an element the launch did not store holds two different poisons; a
    result that depends on poisoned memory differs as well) and no float payload element equal to its own poison bits.
    (Arithmetic that canonicalises NaNs turns both poisons into the same NaN: that dependence shows in the caller's
    reference comparison, which meets a NaN.)  Returns the payloads of the second run."""
    got = [_as_dict(run(p)) for p in range(N_PATTERNS)]
    if got[0].keys() != got[1].keys():
        raise AssertionError("the two runs returned different outputs: %s / %s" % (sorted(got[0]), sorted(got[1])))
    for name in got[0]:
        a, b = got[0][name], got[1][name]
        if a.shape != b.shape or a.dtype != b.dtype:
            raise AssertionError("%s: the two runs returned different shapes or types" % name)
        ia, ib = bits_of(a).reshape(-1), bits_of(b).reshape(-1)
        if a.dtype.is_floating_point:
            for p, i in ((0, ia), (1, ib)):
                hit = i == poison_scalar(a.dtype, p)
                if bool(hit.any()):
                    k = int(torch.nonzero(hit)[0].item())
                    raise AssertionError("%s: payload element %d %s still holds the poison of pattern %d: never written "
                                         "(%d such elements)" % (name, k, _index(a, k), p, int(hit.sum().item())))
        diff = ia != ib
        if bool(diff.any()):
            k = int(torch.nonzero(diff)[0].item())
            pa, pb = poison_scalar(a.dtype, 0), poison_scalar(a.dtype, 1)
            what = "never written" if (int(ia[k]) == pa and int(ib[k]) == pb) else "depends on the poisoned memory"
            raise AssertionError("%s: payload element %d %s differs between the two poison patterns (%s): bits %#x / %#x; "
                                 "%d elements differ" % (name, k, _index(a, k), what, int(ia[k]) & ((1 << 64) - 1),
                                                         int(ib[k]) & ((1 << 64) - 1), int(diff.sum().item())))
    return got[1]


def _index(t, k):
    if t.dim() < 2:
        return ""
    idx = []
    for s in reversed(t.shape):
        k, r = divmod(k, s)
        idx.append(r)
    return "(index %s)" % (tuple(reversed(idx)),)


@contextlib.contextmanager
def frozen(*tensors, names=None):
    """Clone the inputs, run the body, assert they come back bit-identical."""
    keep = [bits_of(t).clone() for t in tensors]
    yield
    for i, (t, k) in enumerate(zip(tensors, keep)):
        now = bits_of(t)
        diff = now != k
        if bool(diff.any()):
            j = int(torch.nonzero(diff.reshape(-1))[0].item())
            name = names[i] if names else "input %d" % i
            raise AssertionError("%s was modified: element %d %s, bits %#x -> %#x; %d elements differ"
                                 % (name, j, _index(t, j), int(k.reshape(-1)[j]) & ((1 << 64) - 1),
                                    int(now.reshape(-1)[j]) & ((1 << 64) - 1), int(diff.sum().item())))
