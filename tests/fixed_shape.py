"""What the tests of the fixed-shape calls share (collate, windows, their spans): the tm_collate struct, its constants and an output in page-locked
memory behind sentinels.  Imports nothing of the package until an output is made, so that a module may import this one before it picks its device."""
import ctypes as C

import numpy as np

NONE = 0xFFFFFF                      # TM_NONE (include/tokenmonster_hip.h)
PAD_LEFT, KEEP_TAIL = 1, 2           # TM_COLLATE_*
DT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
FILL = 0xA5


class Collate(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("first_doc", "ndocs", "row_len", "id_bytes", "pad_id", "bos_id", "eos_id", "flags")]


def spec(x):
    return NONE if x is None else x


class Out:
    """n elements of `elem` bytes in page-locked memory, `shift` elements behind a 16-byte boundary, every byte around them a sentinel"""

    def __init__(self, n, elem, shift=0):
        from tokenmonster_amd.vocab import PinnedBuffer
        self.n, self.elem = n, elem
        self.buf = PinnedBuffer(n * elem + 64)
        a = self.buf.array
        a[:] = FILL
        self.off = (-a.ctypes.data) % 16 + 16 + shift * elem
        self.ptr = a.ctypes.data + self.off

    def view(self, dtype):
        return self.buf.array[self.off:self.off + self.n * self.elem].view(dtype)

    def sentinels_intact(self):
        a = self.buf.array
        return bool((a[:self.off] == FILL).all() and (a[self.off + self.n * self.elem:] == FILL).all())

    def untouched(self):
        return bool((self.buf.array == FILL).all())
