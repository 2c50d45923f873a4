"""What the guarded CTC suites (tests/test_ctc_guarded_gpu.py, tests/test_ctc_guarded_search_gpu.py) share: one call of a C entry point
of include/vocr.h with every byte it may touch owned by the test (tests/guarded.py), the checks every case makes of such a call, and
the table the suites print.  Importing this module needs no GPU; calling into it does."""
import time

import pytest
import torch

from tests import guarded as gd

DEV = "cuda"
ROWS = []                      # (entry, case, branch, error over bar, workspace bytes)
T0 = [None]


class Call(object):
    """One call of `entry`.  ins: name -> None, an fp32 tensor (bands of NaN) or (int32 tensor, band value); outs: name -> None or
    (shape, dtype): poisoned, bands of SENTINEL; nbytes: the workspace handed over, exactly (NaN-filled, a SENTINEL band behind it);
    args(p, ws, nbytes): the entry's argument list from the pointers p[name] (None for an absent tensor), the workspace pointer and its
    size.  inout: the names in `ins` the call may write (an accumulator the caller zeroes).  refuse: the call must fail with VOCR_EINVAL
    (-1); otherwise it must succeed.  The stream is synchronised before returning."""

    def __init__(self, entry, ins, outs, nbytes, args, refuse=False, inout=()):
        from vistaocr_amd import _lib
        self.entry, self.data, self.ins, self.outs, self.inout = entry, {}, {}, {}, tuple(inout)
        for k, v in ins.items():
            if v is None:
                self.ins[k] = None
                continue
            t, band = v if isinstance(v, tuple) else (v, 0)
            t = t.contiguous()
            self.data[k] = t.to(DEV)
            self.ins[k] = gd.Guarded(t.shape, DEV, data=t, dtype=t.dtype, name=k, band=band)
        for k, v in outs.items():
            self.outs[k] = None if v is None else gd.Guarded(v[0], DEV, dtype=v[1], name=k)
        self.ws = gd.workspace(nbytes, DEV)
        p = {k: (None if g is None else g.ptr) for k, g in list(self.ins.items()) + list(self.outs.items())}
        a = args(p, None if self.ws is None else self.ws.ptr, nbytes)
        self.refused = bool(refuse)
        if refuse:
            with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
                _lib.call(entry, *a)
        else:
            _lib.call(entry, *a)
        torch.cuda.synchronize()

    def out(self, name):
        g = self.outs[name]
        return None if g is None else g.t

    def host(self, name):
        g = self.outs[name]
        return None if g is None else g.t.cpu().numpy()

    def assert_guards_intact(self, case):
        """every band of every operand, every output and the workspace bit for bit as it was; no operand changed"""
        for k, g in list(self.ins.items()) + list(self.outs.items()) + [("workspace", self.ws)]:
            if g is not None:
                assert g.outside_untouched(), (self.entry, case, "a band of %s was written" % k)
        for k, g in self.ins.items():
            if g is not None and (k not in self.inout or self.refused):
                a, b = g.t, self.data[k]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (self.entry, case, "operand %s was written" % k)

    def assert_written(self, case):
        """no output element still holds its poison, and no NaN came out of the NaN-filled workspace or the NaN bands"""
        for k, g in self.outs.items():
            if g is not None:
                assert not g.has_unwritten(), (self.entry, case, "output %s has unwritten elements or NaN" % k)

    def assert_nothing_launched(self, case):
        """a refused call: every output still fully poisoned, the workspace untouched, every band intact"""
        for k, g in self.outs.items():
            if g is not None:
                assert g.all_unwritten(), (self.entry, case, "a refused call wrote output %s" % k)
        assert self.ws is None or self.ws.all_unwritten(), (self.entry, case, "a refused call wrote the workspace")
        self.assert_guards_intact(case)

    def assert_same_bits(self, other, case):
        for k, g in list(self.outs.items()) + [(k, self.ins[k]) for k in self.inout]:
            if g is not None:
                h = other.outs[k] if k in other.outs else other.ins[k]
                assert torch.equal(g.bits(), h.bits()), (self.entry, case, "output %s differs between two runs" % k)


def same_bits(a, b):
    """two tensors of one shape and dtype hold the same bits (NaN-safe)"""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.contiguous(), b.contiguous()
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


def guarded_runs(entry, case, ins, outs, nbytes, args, takes_size=True, inout=()):
    """The part of a case that is the same for every entry: the call into poisoned buffers (every output element written, no NaN, every
    band intact), a second call into fresh ones (the same bits), and - where the entry takes workspace_bytes - the refusal of a truly
    smaller workspace, 16 bytes short, with its true size (nothing launched).  Returns the first call."""
    run = Call(entry, ins, outs, nbytes, args, inout=inout)
    run.assert_guards_intact(case)
    run.assert_written(case)
    again = Call(entry, ins, outs, nbytes, args, inout=inout)
    again.assert_guards_intact(case)
    run.assert_same_bits(again, case)
    if takes_size:
        assert nbytes >= 16 and nbytes % 4 == 0, (entry, case, nbytes)
        Call(entry, ins, outs, nbytes - 16, args, refuse=True, inout=inout).assert_nothing_launched(case)
    return run


def row(entry, case, branch, frac, nbytes):
    ROWS.append((entry, case, branch, float(frac), int(nbytes)))


def print_table(title):
    if ROWS:
        print("\n%s\n%-28s %-22s %-58s %10s %12s" % (title, "entry", "case", "branch", "err / bar", "workspace"))
        for e, c, b, f, n in ROWS:
            print("%-28s %-22s %-58s %10.4f %12d" % (e, c, b, f, n))
        print("%d rows, worst %.4f; wall time of the file %.1f s" % (len(ROWS), max(r[3] for r in ROWS), time.time() - T0[0]))
        del ROWS[:]
