"""Guarded buffers for the memory-contract tests (test infrastructure, no GPU needed; tests/test_memory_contract.py).

A `Guarded` is `n` elements of a dtype inside one larger byte tensor, with at least GUARD_WORDS 32-bit guard words before
and after, so an overrun of a whole tile of rows lands in memory the test owns instead of in the allocator's slack.  The
guards hold a chosen 32-bit pattern; the inner part a pattern, given data, or "leavings" (the bytes another run left in
another buffer, repeated to length).  Everything is compared BITWISE through integer views: a NaN pattern never compares
equal as a float, and -0.0 equals +0.0 as one.

  intact()     the guards hold what they were given; on failure the first and last damaged offset, in bytes and in 4-byte
               words relative to the inner buffer (negative: before it; >= its length: behind it)
  unchanged()  the inner part holds the data it was given (a read-only input)
  bits()       the inner part as a numpy integer array (what two runs are compared by)

The inner start is 256-byte aligned by default; `shift` moves it by that many bytes (4: the natural alignment of a float).
"""
import ctypes

import numpy as np
import torch

ZERO, NAN, HUGE = 0x00000000, 0xFFFFFFFF, 0x7F7FFFFF          # all-zero; a NaN (quiet, negative); the largest finite fp32
PATTERNS = {"zero": ZERO, "nan": NAN, "huge": HUGE}
GUARD_WORDS = 8192
ALIGN = 256


def _i32(pattern):
    return int(np.array([pattern], np.uint32).view(np.int32)[0])


def _bytes_of(src):
    """a tensor or numpy array as a flat uint8 tensor (a copy is made only for numpy input)"""
    if isinstance(src, np.ndarray):
        src = torch.from_numpy(np.ascontiguousarray(src))
    return src.contiguous().reshape(-1).view(torch.uint8)


class Guarded:
    def __init__(self, n, dtype=torch.float32, device="cpu", fill=ZERO, data=None, leavings=None, guard_fill=NAN,
                 guard_words=GUARD_WORDS, shift=0, name="buffer"):
        assert guard_words >= GUARD_WORDS and shift >= 0 and shift % 4 == 0
        self.n, self.dtype, self.name = int(n), dtype, name
        item = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = self.n * item
        inner_room = (self.nbytes + 3) // 4 * 4                      # the guards are whole 32-bit words
        total = 4 * guard_words + ALIGN + shift + inner_room + 4 * guard_words
        self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 4 == 0
        self.start = 4 * guard_words + (-(self.raw.data_ptr() + 4 * guard_words)) % ALIGN + shift
        self.raw.view(torch.int32).fill_(_i32(guard_fill))
        self.view = self.raw[self.start:self.start + self.nbytes].view(dtype)
        assert self.view.data_ptr() % ALIGN == shift % ALIGN and self.view.numel() == self.n
        self.data = None
        self.refill(fill=fill, data=data, leavings=leavings)
        self._front = self.raw[:self.start].clone()
        self._back = self.raw[self.start + self.nbytes:].clone()
        assert self._front.numel() >= 4 * guard_words and self._back.numel() >= 4 * guard_words

    # ---- contents ----------------------------------------------------------------------------------------------------
    def refill(self, fill=ZERO, data=None, leavings=None):
        """inner part <- `data` (n elements, kept for unchanged()), or `leavings` (any tensor: its bytes, repeated to
        length), or the 32-bit pattern `fill`"""
        inner = self.raw[self.start:self.start + self.nbytes]
        self.data = None
        if data is not None:
            src = _bytes_of(data if isinstance(data, torch.Tensor) else np.asarray(data)).to(self.raw.device)
            assert src.numel() == self.nbytes, f"{self.name}: {src.numel()} bytes of data for {self.nbytes}"
            inner.copy_(src)
            self.data = inner.clone()
        elif leavings is not None:
            src = _bytes_of(leavings).to(self.raw.device)
            assert src.numel() > 0
            reps = -(-self.nbytes // src.numel())
            inner.copy_(src.repeat(reps)[:self.nbytes])
        else:
            words = torch.full(((self.nbytes + 3) // 4,), _i32(fill), dtype=torch.int32, device=self.raw.device)
            inner.copy_(words.view(torch.uint8)[:self.nbytes])
        return self

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def bits(self):
        """the inner part as numpy integers of the element's width"""
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.view.element_size()]
        return self.view.view(it).cpu().numpy().copy()

    def numpy(self):
        return self.view.cpu().numpy().copy()

    # ---- checks ------------------------------------------------------------------------------------------------------
    def damage(self):
        """None, or (first, last) damaged byte offset relative to the inner buffer's first byte"""
        bad = []
        for now, was, off in ((self.raw[:self.start], self._front, -self.start),
                              (self.raw[self.start + self.nbytes:], self._back, self.nbytes)):
            d = torch.nonzero(now != was).reshape(-1)
            if d.numel():
                bad += [int(d[0]) + off, int(d[-1]) + off]
        return (min(bad), max(bad)) if bad else None

    def intact(self):
        d = self.damage()
        assert d is None, (f"{self.name}: guard words overwritten, first damaged byte {d[0]} (word {d[0] // 4}), last {d[1]} "
                           f"(word {d[1] // 4}) relative to the inner buffer of {self.nbytes} bytes ({self.nbytes // 4} words)")
        return True

    def unchanged(self):
        assert self.data is not None, f"{self.name}: holds no given data"
        d = torch.nonzero(self.raw[self.start:self.start + self.nbytes] != self.data).reshape(-1)
        assert d.numel() == 0, (f"{self.name}: read-only input written, {d.numel()} bytes differ, first at byte {int(d[0])} "
                                f"(word {int(d[0]) // 4}), last at byte {int(d[-1])}")
        return True

    def check(self):
        self.intact()
        if self.data is not None:
            self.unchanged()
        return True


def same_bits(got, want, what):
    """two dicts name -> numpy integer array (Guarded.bits()) are equal element by element"""
    assert set(got) == set(want), what
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} has another shape or type"
        d = np.flatnonzero(a != b)
        assert d.size == 0, f"{what}: {k} differs in {d.size} of {a.size} elements, first at {int(d[0])}, last at {int(d[-1])}"
