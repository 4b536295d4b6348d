"""Guarded arenas: what a call does to the caller's memory outside its output values.

One allocation per call under test, laid out

    [guard][operand][guard][operand] ... [guard]

* Everything is prefilled with the sentinel, all bits of the word set.  The sentinel is >= every
  modulus of its word class (q <= 0xFFF00001 on 32-bit words, q < 2^62 on 64-bit words), so a
  canonical result is never the sentinel, an output word that was never written is visible, and a
  guard word read as an operand is out of range (NTTMUL_FLAG_VALIDATE turns it into
  NTTMUL_ERANGE).
* A guard is at least `guard` words wide, and `guard_words` never gives less than GUARD_MIN =
  8192 words, the span of one block of the widest kernel (32 polynomials x 256 words, or
  2 x 4096), nor less than one whole batch entry of the widest operand.
* Each operand starts at an address aligned to its word and to nothing larger:
  addr % 16 == 4 for 32-bit words, == 8 for 64-bit words (asserted on every view handed out).

`check()` asserts that every guard word still holds the sentinel, that every input is bit-identical
to the copy taken at placement, and that no output word is the sentinel; a violation raises
GuardError naming the kind, the operand, the word offset relative to that operand's start
(-1 = the word before it, len = the word after its last) and the value found.

HostArena lives in a numpy array (or in a page-locked nttmul.host_empty block), DeviceArena in one
torch tensor; both share the layout and the check, which runs on a host image of the whole
allocation.  Importing this module needs neither a GPU nor the library.
"""
import numpy as np

GUARD_MIN = 8192
_ALIGN_SLACK = 4            # words a guard may grow by to reach the wanted misalignment


def sentinel(bits):
    return (1 << bits) - 1


def dtype_of(bits):
    assert bits in (32, 64)
    return np.uint32 if bits == 32 else np.uint64


def guard_words(*entry_words):
    """The guard width for a call whose operands have batch entries of these many words
    (limbs * n, terms * n, (K + L) * n or n): one whole entry of the widest, at least GUARD_MIN."""
    return max((GUARD_MIN,) + tuple(int(w) for w in entry_words))


class GuardError(AssertionError):
    def __init__(self, kind, operand, offset, value):
        self.kind, self.operand, self.offset, self.value = kind, operand, int(offset), int(value)
        super().__init__(f"{kind}: {operand}[{self.offset}] = {self.value:#x}")


class _Arena:
    """Layout and check.  Operands are given as name=value keywords in layout order: a numpy array
    is an input (copied in, must be unchanged after the call), an integer is an output of that
    many words.  Names listed in `inplace` are inputs the call also writes (out == in): they are
    held to the output rule instead of the input rule."""

    def __init__(self, bits, guard, inplace=(), **operands):
        self.bits, self.guard = bits, int(guard)
        self.dtype = dtype_of(bits)
        self.sentinel = self.dtype(sentinel(bits))
        assert self.guard >= 1 and operands
        self._spec = []
        for name, v in operands.items():
            if isinstance(v, (int, np.integer)):
                assert name not in inplace
                self._spec.append((name, int(v), None))
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype).reshape(-1)
                self._spec.append((name, v.size, v.copy()))
        self._inplace = tuple(inplace)
        assert all(any(n == s[0] for s in self._spec) for n in self._inplace)
        self.total = (sum(s[1] for s in self._spec)
                      + (len(self._spec) + 1) * (self.guard + _ALIGN_SLACK))

    def _layout(self, base_addr):
        """Word offsets of the operands for an allocation at base_addr: each guard is self.guard
        words, widened by up to three so that the operand after it starts at addr % 16 == word."""
        wb = self.bits // 8
        assert base_addr % wb == 0
        self.base_addr = base_addr
        self.spans, pos = {}, 0
        for name, words, _ in self._spec:
            pos += self.guard
            while (base_addr + pos * wb) % 16 != wb:
                pos += 1
            self.spans[name] = (pos, words)
            pos += words
        assert pos + self.guard <= self.total
        self.inputs = {name: data for name, _, data in self._spec
                       if data is not None and name not in self._inplace}
        self.outputs = [name for name, _, data in self._spec
                        if data is None or name in self._inplace]

    def _image(self):
        """The prefilled host image of the whole allocation."""
        img = np.full(self.total, self.sentinel, dtype=self.dtype)
        for name, words, data in self._spec:
            if data is not None:
                start = self.spans[name][0]
                img[start:start + words] = data
        return img

    def addr(self, name):
        return self.base_addr + self.spans[name][0] * (self.bits // 8)

    def _assert_aligned(self, name, ptr):
        wb = self.bits // 8
        assert ptr == self.addr(name) and ptr % 16 == wb, (name, hex(ptr))

    def snapshot(self):
        raise NotImplementedError

    def get(self, name, shape=None):
        """The operand's words now, as a numpy copy."""
        start, words = self.spans[name]
        out = self.snapshot()[start:start + words].copy()
        return out if shape is None else out.reshape(shape)

    def _nearest(self, g):
        """(operand, offset relative to its start) for guard word g."""
        best = None
        for name, (start, words) in self.spans.items():
            off = g - start
            dist = -off if off < 0 else off - words + 1
            if best is None or dist < best[0]:
                best = (dist, name, off)
        return best[1], best[2]

    def check(self):
        img = self.snapshot()
        assert img.dtype == self.dtype and img.size == self.total
        mask = np.ones(self.total, dtype=bool)
        for start, words in self.spans.values():
            mask[start:start + words] = False
        bad = np.flatnonzero(mask & (img != self.sentinel))
        if bad.size:
            name, off = self._nearest(int(bad[0]))
            raise GuardError("guard overwritten", name, off, img[bad[0]])
        for name, data in self.inputs.items():
            start, words = self.spans[name]
            diff = np.flatnonzero(img[start:start + words] != data)
            if diff.size:
                raise GuardError("input changed", name, diff[0], img[start + diff[0]])
        for name in self.outputs:
            start, words = self.spans[name]
            left = np.flatnonzero(img[start:start + words] == self.sentinel)
            if left.size:
                raise GuardError("output not written", name, left[0], self.sentinel)


class HostArena(_Arena):
    """The arena in host memory: a numpy array, or with pinned=True a page-locked block of
    nttmul.host_empty (the direct-DMA path of the host-buffer calls).  self[name] is a contiguous
    1-D numpy view."""

    def __init__(self, bits, guard, inplace=(), pinned=False, **operands):
        super().__init__(bits, guard, inplace, **operands)
        if pinned:
            import nttmul
            self.buf = nttmul.host_empty((self.total,), self.dtype)
        else:
            self.buf = np.empty(self.total, dtype=self.dtype)
        self._layout(self.buf.ctypes.data)
        self.buf[...] = self._image()

    def __getitem__(self, name):
        start, words = self.spans[name]
        view = self.buf[start:start + words]
        assert view.flags.c_contiguous
        self._assert_aligned(name, view.ctypes.data)
        return view

    def snapshot(self):
        return self.buf


class DeviceArena(_Arena):
    """The arena in one torch tensor on the current HIP device.  self[name] is a contiguous 1-D
    tensor view (int32 / int64) that nttmul._dev_arg accepts unchanged.  The image goes up in one
    copy; snapshot() brings the whole allocation back in one copy and keeps it until sync()."""

    def __init__(self, torch, bits, guard, inplace=(), **operands):
        super().__init__(bits, guard, inplace, **operands)
        self._tdtype = torch.int32 if bits == 32 else torch.int64
        self.buf = torch.empty(self.total, dtype=self._tdtype, device="cuda")
        self._layout(self.buf.data_ptr())
        signed = self._image().view(np.int32 if bits == 32 else np.int64)
        self.buf.copy_(torch.from_numpy(signed))
        self._snap = None

    def __getitem__(self, name):
        start, words = self.spans[name]
        view = self.buf[start:start + words]
        assert view.is_contiguous()
        self._assert_aligned(name, view.data_ptr())
        return view

    def sync(self):
        """Forget the host image: the next snapshot() reads the device again."""
        self._snap = None

    def snapshot(self):
        if self._snap is None:
            self._snap = self.buf.cpu().numpy().view(self.dtype)
        return self._snap
