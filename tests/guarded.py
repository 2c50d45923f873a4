"""Guarded buffers: how a test owns every byte a kernel may touch.  Importing this module needs no GPU and no library; every helper works
on `cpu` tensors as well (tests/test_guarded_cpu.py plants writes by hand and checks that they are reported).

Buffers follow tests/gemm_ref.py (same GUARD and SENTINEL): a tensor the kernel READS sits between guard bands, so a read outside it
reaches the result; a tensor the kernel WRITES (outputs, and workspaces of exactly the bytes their *_workspace_bytes query answers) starts
poisoned between bands of the sentinel bit pattern, so an element the kernel leaves out, or a workspace word it reads without having
written it, shows in the result and a store outside shows as a touched band.

The fills:
  fp32 / fp16, read      bands of NaN in the tensor's own format.
  fp32 / fp16, written   the tensor starts as NaN (has_nan()), bands of SENTINEL.
  int32 / uint8, written the tensor starts as POISON in every 32-bit word (has_unwritten()), bands of SENTINEL.  POISON is 0xA5A5A5A5:
                         as an int32 it is -1515870811, and every integer output of include/vocr.h is a frame, a label, a length, a count
                         or a distance - never below -1; as four bytes it is 165 four times, and an operation code of vocr_edit_stats'
                         out_ops is 0 .. 4.  No contract can produce it, so a word that still holds it was not written.
  int32, read            bands of `band`, the caller's choice of a value the operand may legally hold (default 0: an empty line, the first
                         state, the blank), so that a kernel which reads outside and indexes with what it found stays inside the test's
                         own allocations.  Never a huge or a negative word.
Rows with a stride (labels[B][n][label_stride], queries[nq][query_stride]): pack_labels / pack_rows fill every slot past a row's own length,
and every column past the width the kernel is told, with `fill` - the callers pass V, one past the alphabet: a kernel that looks at such a
slot meets an invalid label (its score turns -inf and the comparison fails), one that gathers through it reads logits[..][V], inside the
test's allocation."""
import numpy as np
import torch

from tests.gemm_ref import GUARD, SENTINEL

_NAN_WORD = {torch.float32: 0x7FC00000, torch.float16: 0x7E007E00}          # one 32-bit word of NaN in the tensor's own format
POISON = 0xA5A5A5A5 - (1 << 32)                                             # as an int32: -1515870811
_INTS = (torch.int32, torch.uint8)


class Guarded(object):
    """A contiguous tensor of `shape` behind GUARD 32-bit words and in front of GUARD more, in one allocation (the tensor starts 256
    bytes into it: every alignment a kernel asks for holds).
    data given: an operand - the bands hold NaN of the tensor's format, or `band` for an integer tensor.  data None: an output or a
    workspace - the tensor starts as NaN (integers: POISON) and the bands hold SENTINEL."""

    def __init__(self, shape, dev, data=None, dtype=torch.float32, name="", band=0):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = torch.empty(0, dtype=dtype).element_size()
        assert numel > 0 and numel * item % 4 == 0, (shape, dtype)
        self.words, self.name, self.dtype = numel * item // 4, name, dtype
        if data is None:
            self.band = SENTINEL
        else:
            self.band = int(band) if dtype in _INTS else _NAN_WORD[dtype]
        self.buf = torch.full((GUARD + self.words + GUARD,), self.band, dtype=torch.int32, device=dev)
        body = self.buf[GUARD:GUARD + self.words]
        self.t = body.view(dtype).view(shape)
        if data is None:
            if dtype in _INTS:
                body.fill_(POISON)
            else:
                self.t.fill_(float("nan"))
        else:
            assert tuple(data.shape) == shape, (tuple(data.shape), shape)
            self.t.copy_(data.to(dev))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def outside_untouched(self):
        """both bands still hold their fill, bit for bit"""
        front, back = self.buf[:GUARD], self.buf[GUARD + self.words:]
        return bool((front == self.band).all()) and bool((back == self.band).all())

    def has_nan(self):
        return bool(torch.isnan(self.t).any())

    def has_unwritten(self):
        """an element still holds its initial fill: NaN, or POISON in an integer tensor (has_nan's counterpart)"""
        if self.dtype == torch.int32:
            return bool((self.t == POISON).any())
        if self.dtype == torch.uint8:
            return bool((self.t == (POISON & 0xFF)).any())
        return self.has_nan()

    def all_unwritten(self):
        """every element still holds its initial fill (a refused call launched nothing)"""
        if self.dtype in _INTS:
            return bool((self.bits() == POISON).all())
        return bool(torch.isnan(self.t).all())

    def bits(self):
        return self.buf[GUARD:GUARD + self.words]


def workspace(nbytes, dev, name="workspace"):
    """a workspace of exactly `nbytes` (what the library's size query answered), NaN-filled, a sentinel band behind it; None for 0 bytes"""
    assert nbytes % 4 == 0
    return Guarded((nbytes // 4,), dev, name=name) if nbytes else None


def pack_rows(seqs, stride, fill):
    """seqs (lists of ints, or None) as (rows int32 [len(seqs), stride] with every slot past a row's own content = fill, lens int32
    [len(seqs)]; None: length -1); a row longer than the stride keeps its length and loses its tail"""
    rows = np.full((len(seqs), max(int(stride), 1)), int(fill), dtype=np.int32)
    lens = np.zeros((len(seqs),), dtype=np.int32)
    for i, s in enumerate(seqs):
        if s is None:
            lens[i] = -1
        else:
            lens[i] = len(s)
            k = min(len(s), rows.shape[1])
            rows[i, :k] = s[:k]
    return torch.from_numpy(rows), torch.from_numpy(lens)


def pack_labels(hyps, stride, fill):
    """hyps[b][q] (lists or None) as (labels int32 [B,n,stride], label_lens int32 [B,n]) by pack_rows"""
    B, n = len(hyps), len(hyps[0])
    rows, lens = pack_rows([h for row in hyps for h in row], stride, fill)
    return rows.view(B, n, -1), lens.view(B, n)
