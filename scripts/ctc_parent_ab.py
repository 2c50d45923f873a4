"""A change to the alpha/beta sweeps of ctc.hip that must move neither bits nor time: vocr_ctc_loss_grad of the in-tree libvocr.so
against the PARENT commit's library at scripts/_cut/libvocr.so (build a clean checkout of the parent outside the tree and copy its
libvocr.so there), both loaded with ctypes into one process.

Bits: every (case, regime) of tests.ctc_ref.all_cases() at each max_label_len of tests/test_ctc_fp64_gpu.py's forced() (every launch
path that admits the batch), the workspace filled with a constant first; SHA-256 of nll, of dlogits and of the WHOLE workspace (the
log-softmax, every alpha / beta row and pad column, the rows past act_len that no kernel may write) under both libraries.  Every digest
pair must be equal; the script exits 1 otherwise.

Time: the whole call with HIP events on the workloads' own shapes - bench_full (T 294, B 32, V 96: one position per lane), c4_ragged
(T 588, B 32, V 166: two per lane), generic_long (T 1200, B 2, V 166: the LDS path) - both libraries warmed up on every shape, then
windows of --window calls alternating between the libraries for --rounds rounds.  Per shape and library: the median of the round
medians, and the parent's own max - min over its rounds, which is the only margin: the new median must not exceed the parent's median
plus that spread.

    python scripts/ctc_parent_ab.py [--window 200] [--rounds 5] [--out profiles/ctc_mirror_ab.txt]"""
import argparse
import ctypes
import functools
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vistaocr_amd import _lib                                # noqa: E402
from tests import ctc_ref as cr                              # noqa: E402
from tests.test_ctc_fp64_gpu import forced, kernel_of        # noqa: E402

FILL = -3.0
TIMED = ("bench_full", "c4_ragged", "generic_long")


def open_lib(path):
    lib = ctypes.CDLL(path)
    for name in ("vocr_ctc_workspace_bytes", "vocr_ctc_loss_grad", "vocr_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


class Call:
    """one batch on the device and what vocr_ctc_loss_grad needs for it at max_label_len `mll`"""

    def __init__(self, x, flat, ll, act, mll, nbytes):
        self.shape, self.mll = tuple(x.shape), int(mll)
        off = np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int32)
        self.x = x.contiguous().cuda()
        self.ints = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (flat.numpy(), off, ll, act)]
        self.nll = torch.empty(len(ll), dtype=torch.float32, device="cuda")
        self.dl = torch.empty(self.shape, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")

    def run(self, lib):
        T, B, V = self.shape
        rc = lib.vocr_ctc_loss_grad(self.x.data_ptr(), *[a.data_ptr() for a in self.ints], self.nll.data_ptr(), self.dl.data_ptr(),
                                    self.ws.data_ptr(), T, B, V, self.mll, None)
        if rc != 0:
            raise RuntimeError("vocr_ctc_loss_grad failed (%d): %s" % (rc, (lib.vocr_last_error() or b"?").decode()))

    def digests(self, lib):
        for t in (self.nll, self.dl, self.ws):
            t.fill_(FILL)
        self.run(lib)
        torch.cuda.synchronize()
        return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (self.nll, self.dl, self.ws)]


@functools.lru_cache(maxsize=1)
def _case(name, regime):
    return cr.build_case(name, regime)


def make_call(libs, name, regime, mll=None):
    x, flat, ll, act, _ = _case(name, regime)
    mll = max(ll) if mll is None else mll
    sizes = {lib.vocr_ctc_workspace_bytes(*x.shape, mll) for lib in libs}
    assert len(sizes) == 1 and min(sizes) > 0, "the two libraries size the workspace differently: %s" % sorted(sizes)
    return Call(x, flat, ll, act, mll, sizes.pop()), max(ll)


def window(call, lib, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        call.run(lib)
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "_cut", "libvocr.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_mirror_ab.txt"))
    args = ap.parse_args()
    assert args.window >= 200 and args.rounds >= 5
    new, parent = open_lib(_lib.LIB_PATH), open_lib(args.parent)
    libs = (new, parent)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("new: %s   parent: %s" % (os.path.relpath(_lib.LIB_PATH, ROOT), os.path.relpath(args.parent, ROOT)))
    say("")
    say("bits: SHA-256 (first 12 hex digits) of nll, dlogits and the whole workspace, filled with %g before the call" % FILL)
    fmt = "%-17s %-12s %4s %-7s | %-12s %-12s %-12s | %s"
    say(fmt % ("case", "regime", "mll", "path", "nll", "dlogits", "workspace", "new vs parent"))
    differ = 0
    for name, regime in cr.all_cases():
        lmax = max([c for c in cr.GPU_CASES if c[0] == name][0][4])
        for mll in forced(lmax):
            call, _ = make_call(libs, name, regime, mll)
            dn, dp = call.digests(new), call.digests(parent)
            bad = [w for w, a, b in zip(("nll", "dlogits", "workspace"), dn, dp) if a != b]
            differ += len(bad)
            say(fmt % (name, cr.regime_name(regime), mll, kernel_of(mll), dn[0][:12], dn[1][:12], dn[2][:12],
                       "equal" if not bad else "DIFFER: %s (parent %s)" % (", ".join(bad), " ".join(d[:12] for d in dp))))
    say("digest pairs that differ: %d" % differ)
    say("")
    say("time: vocr_ctc_loss_grad, the whole call (log-softmax, alpha/beta, gradient), HIP events, us; per round the median of a window "
        "of %d calls, the libraries alternating, %d rounds after a warm-up window of each" % (args.window, args.rounds))
    tfmt = "%-13s %-7s %5s %3s %4s | %9s %9s %9s | %9s | %s"
    say(tfmt % ("shape", "path", "T", "B", "V", "parent", "p. spread", "new", "new - p.", "new <= parent + spread"))
    slower = 0
    calls = [make_call(libs, name, cr.DENSE) for name in TIMED]
    for call, _ in calls:
        for lib in libs:
            window(call, lib, args.window)
    for name, (call, lmax) in zip(TIMED, calls):
        med = {0: [], 1: []}
        for r in range(args.rounds):
            for i in ((0, 1) if r % 2 == 0 else (1, 0)):
                med[i].append(window(call, libs[i], args.window))
        mn, mp = float(np.median(med[0])), float(np.median(med[1]))
        spread = max(med[1]) - min(med[1])
        ok = mn <= mp + spread
        slower += not ok
        say(tfmt % (name, kernel_of(lmax), *call.shape, "%.2f" % mp, "%.2f" % spread, "%.2f" % mn, "%+.2f" % (mn - mp),
                    "yes" if ok else "NO"))
        say("    rounds, parent: %s   new: %s" % (" ".join("%.2f" % v for v in med[1]), " ".join("%.2f" % v for v in med[0])))
    say("shapes slower than the parent's median plus its spread: %d" % slower)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if differ or slower else 0


if __name__ == "__main__":
    sys.exit(main())
