"""GPU: every LSTM entry point the product runs, called on the C entry (_lib.call) in memory the test owns to the byte (tests/guarded.py):
vocr_lstm_fwd, vocr_lstm_fwd_range, vocr_lstm_bwd, vocr_lstm_bwd_bias, vocr_lstm_bwd_parts + vocr_lstm_bias_from_parts,
vocr_lstm_fwd_packed, vocr_lstm_bwd_packed, vocr_seq_rowmap, vocr_gather_rows, vocr_gather_rows_fill_grad.

The library reads VOCR_LSTM_SWEEP / VOCR_LSTM_WRITE_THROUGH once per process and persistent sweeps must not share the device, so every
setting is ONE child process (this module, child_main), one after the other, each under a time limit sized to its work; one more child
at the default setting has the packed entry points, the row tools, the unaligned-pointer runs and the refusals.

Buffers: float operands between NaN bands, lens and the row maps between bands of 0, outputs NaN / POISON between SENTINEL bands, the
workspace guarded.workspace(vocr_lstm_workspace_bytes(T, B, H)) - exactly that size, NaN-filled, a sentinel band behind it -, the health
word a guarded zeroed int32[4].  Every case (tests/lstm_cases.py: GUARDED_CASES, T = 11 and ragged lengths 11 .. 1, plus T = 1 and T = 2)
holds, at every setting:
  accuracy       y, gates, cell on valid frames, dgates everywhere, dbias from vocr_lstm_bwd_bias and from the parts path, dgates of
                 vocr_lstm_bwd: against lstm_ref.Refs at lstm_ref's own bars;
  written        y, dgates: no NaN and exactly 0 past lens; dbias: no NaN; gates, cell: no NaN and 0 past lens (include/vocr.h: the dense
                 forward writes every frame).  The backward runs on the forward's own buffers, unmodified, and once more on a copy whose
                 frames past lens hold NaN: the same bits (the backward never reads a frame past lens);
  bands          every band of every live buffer is intact after every call, the workspace's included; health stays 0;
  workspace      three runs give the same bits: a fresh NaN-filled workspace in front of every call; ONE workspace carried through
                 fwd -> bwd_bias -> bwd_parts -> bias_from_parts -> fwd; a workspace that a case of another shape (and, at the default
                 setting, another kind: lstm_cases.DONOR) ran its forward and backward in first;
  ranges         vocr_lstm_fwd_range [0, c) + [c, T) on one workspace that is NOT refilled in between (the documented exception), c = 1,
                 4, 5, T - 1: y, gates, cell bit for bit those of the single call.
Default-setting child:
  unaligned      H = 128 and 512: whh_fwd, y (forward), whht_fwd, dgates (backward) one float into their guarded buffers - the generic
                 per-step kernels - under the same accuracy, written and band checks; gates one float off is refused with VOCR_EINVAL by
                 vocr_lstm_fwd, _bwd, _bwd_bias, _bwd_parts and _bwd_packed, every output still all-unwritten;
  packed         y and dgates start as zeros in the rows to_dense marks -1 and NaN everywhere else; afterwards no NaN, the -1 rows still
                 bitwise zero; operand rows the layout has no frame for hold NaN; unpacked on the CPU, the accuracy checks of the dense
                 cases;
  row tools      vocr_seq_rowmap against the layout written out in Python (lstm_cases.packed_layout), outputs fully written, T above
                 max(len), either map alone; vocr_gather_rows at n = 8 / 7 / 8 with dst one float off, fill NULL / given, maps all -1;
                 vocr_gather_rows_fill_grad at n = 7, 96 x nrows = 1, 63, 64, 65, 4097 in a NaN-filled workspace of exactly
                 vocr_gather_rows_fill_grad_workspace_bytes(n) against an fp64 sum at 1e-6 of the column's sum of |dout|, twice: same bits.
Run with -s for the table (profiles/lstm_guarded_errors.txt keeps it)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import guarded as gd
from tests import lstm_cases as lc
from tests import lstm_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, F32 = torch.int32, torch.float32
NAN = float("nan")
_CHILD = "import sys; sys.path.insert(0, %r); from tests import test_lstm_guarded_gpu as m; m.child_main(sys.argv[1])" % ROOT


def _run_child(mode, env, timeout):
    r = subprocess.run([sys.executable, "-c", _CHILD, mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (mode, env, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("setting", lc.SETTINGS)
def test_dense_entry_points_in_guarded_memory(setting):
    floor = setting.split("/")[0]
    out = _run_child("sweeps", dict(VOCR_LSTM_SWEEP=floor, VOCR_LSTM_WRITE_THROUGH="1" if "/wt" in setting else "0"), timeout=240)
    rows = [l for l in out.splitlines() if l.startswith("ROW ")]
    assert len(rows) == len(lc.GUARDED_CASES), out


def test_every_kind_is_reached():
    """over all settings every kind runs forward and backward (the rule: lstm_cases.sweep_kind; the fp64 suite asserts the same)"""
    seen = {False: set(), True: set()}
    for setting in lc.SETTINGS:
        for (T, B, H, _) in lc.GUARDED_CASES:
            for bw in (False, True):
                seen[bw].add(lc.sweep_kind(bw, B, H, setting.split("/")[0], rows=T * B))
    for bw in (False, True):
        assert seen[bw] == set(lc._ALL), ("backward" if bw else "forward", seen[bw])


def test_packed_rows_row_tools_and_unaligned_pointers():
    env = {k: v for k, v in os.environ.items() if not k.startswith("VOCR_LSTM_")}
    r = subprocess.run([sys.executable, "-c", _CHILD, "default"], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------------------ the children
class _Buf(object):
    """a guarded buffer and the tensor inside it that a call sees: the whole of it, or (shift = 1) a view that starts one float in, so
    that its pointer is 4 bytes past a 16-byte boundary; the float in front then counts as band"""

    def __init__(self, pool, name, shape, data=None, dtype=F32, shift=0, band=0):
        numel = 1
        for s in shape:
            numel *= int(s)
        if data is not None:
            data = data.reshape(-1).to(dtype)
            if shift:
                data = torch.cat([torch.full((shift,), NAN, dtype=dtype), data])
        self.g = gd.Guarded((numel + shift,), pool.dev, data=data, dtype=dtype, name=name, band=band)
        self.t = self.g.t[shift:].view(tuple(shape))
        self.ptr, self.name, self.shift, self.is_out = self.t.data_ptr(), name, shift, data is None
        assert self.ptr % 16 == 4 * shift
        pool.live.append(self)

    def lead_ok(self):
        return torch.isnan(self.g.t[:self.shift]).all() if self.shift else torch.ones((), dtype=torch.bool, device=self.t.device)

    def cpu(self):
        return self.t.cpu()

    def bits(self):
        return self.t.view(I32) if self.t.dtype == F32 else self.t


class _Pool(object):
    """every guarded buffer of one case; check() looks at every band of every one of them in one trip to the device"""

    def __init__(self, dev):
        self.dev, self.live = dev, []

    def op(self, name, data, dtype=F32, shift=0):
        return _Buf(self, name, tuple(data.shape), data=data, dtype=dtype, shift=shift)

    def out(self, name, shape, dtype=F32, shift=0):
        return _Buf(self, name, shape, dtype=dtype, shift=shift)

    def ws(self, nbytes, name="workspace"):
        b = _Buf(self, name, (nbytes // 4,))
        assert nbytes % 4 == 0 and b.g.words * 4 == nbytes
        return b

    def drop(self, *bufs):
        for b in bufs:
            self.live.remove(b)

    def check(self, what, health=None):
        torch.cuda.synchronize()
        flags = []
        for b in self.live:
            g = b.g
            flags.append((g.buf[:gd.GUARD] == g.band).all() & (g.buf[gd.GUARD + g.words:] == g.band).all() & b.lead_ok())
        ok = torch.stack(flags).cpu().tolist()
        touched = [b.name for b, f in zip(self.live, ok) if not f]
        assert not touched, (what, "bands touched", touched)
        if health is not None:
            hw = health.cpu().tolist()
            assert hw == [0, 0, 0, 0], (what, "health word", hw)       # a hand-off timed out: stop here, nothing more runs


def _same_bits(a, b):
    return bool(torch.equal(a.bits(), b.bits()))


def _fmt(errs):
    return "  ".join("%s %.2e/%.2e" % (nm, ek, b) for nm, ek, _, b in errs)


class _Dense(object):
    """one dense case: its guarded operands and one method per entry point; every method allocates fresh poisoned outputs, calls the
    entry once and checks every band and the health word"""

    def __init__(self, lib, call, stream, dev, T, B, H, tag):
        self.lib, self.call, self.s, self.dev, self.T, self.B, self.H, self.tag = lib, call, stream, dev, T, B, H, tag
        _, (lens, xproj, whh, dy, mask, refs) = lc.guarded_case(T, B, H)
        self.lens, self.refs = lens, refs
        self.G, self.R = 4 * H, T * B
        G, R = self.G, self.R
        P = self.P = _Pool(dev)
        self.xp = P.op("xproj", xproj.reshape(2, R, G))
        self.whh = whh
        self.wf, self.wr = P.op("whh_fwd", whh[0]), P.op("whh_rev", whh[1])
        self.wtf, self.wtr = P.op("whht_fwd", whh[0].t().contiguous()), P.op("whht_rev", whh[1].t().contiguous())
        self.ln = P.op("lens", torch.tensor(lens, dtype=I32), dtype=I32)
        dyv, mk = dy.reshape(R, 2 * H), mask.reshape(R, 2 * H)
        self.dy, self.mask, self.dym = P.op("dy", dyv), P.op("dy_mask", mk), P.op("dy*mask", dyv * mk)
        self.hw = P.op("health", torch.zeros(4, dtype=I32), dtype=I32)
        self.nbytes = lib.vocr_lstm_workspace_bytes(T, B, H)
        self.parts_ok = bool(lib.vocr_lstm_bwd_parts_supported(T, B, H))

    def fresh(self):
        return self.P.ws(self.nbytes)

    def _done(self, what):
        self.P.check("%s %s" % (self.tag, what), self.hw.t)

    def fwd(self, ws, cut=None, wf=None, yshift=0):
        T, B, H, G, R, P = self.T, self.B, self.H, self.G, self.R, self.P
        y, gt, cl = P.out("y", (R, 2 * H), shift=yshift), P.out("gates", (2, R, G)), P.out("cell", (2, R, H))
        head = (self.xp.ptr, (wf or self.wf).ptr, self.wr.ptr, self.ln.ptr, y.ptr, gt.ptr, cl.ptr, ws.ptr, T, B, H)
        if cut is None:
            self.call("vocr_lstm_fwd", *head, self.hw.ptr, self.s)
            self._done("fwd")
        else:
            self.call("vocr_lstm_fwd_range", *head, 0, cut, self.hw.ptr, self.s)
            self._done("fwd_range [0, %d)" % cut)
            self.call("vocr_lstm_fwd_range", *head, cut, T, self.hw.ptr, self.s)
            self._done("fwd_range [%d, %d)" % (cut, T))
        return y, gt, cl

    def bwd_bias(self, ws, gt, cl, wtf=None, dgshift=0, bias=True):
        T, B, H, G, R, P = self.T, self.B, self.H, self.G, self.R, self.P
        dg = P.out("dgates", (2, R, G), shift=dgshift)
        head = (self.dym.ptr, (wtf or self.wtf).ptr, self.wtr.ptr, self.ln.ptr, gt.ptr, cl.ptr, dg.ptr)
        if not bias:
            self.call("vocr_lstm_bwd", *head, ws.ptr, T, B, H, self.hw.ptr, self.s)
            self._done("bwd")
            return dg, None
        db = P.out("dbias", (2, G))
        self.call("vocr_lstm_bwd_bias", *head, db.ptr, ws.ptr, T, B, H, self.hw.ptr, self.s)
        self._done("bwd_bias")
        return dg, db

    def parts(self, ws, gt, cl):
        T, B, H, G, R, P = self.T, self.B, self.H, self.G, self.R, self.P
        dg, db = P.out("dgates(parts)", (2, R, G)), P.out("dbias(parts)", (2, G))
        self.call("vocr_lstm_bwd_parts", self.dy.ptr, self.mask.ptr, self.wtf.ptr, self.wtr.ptr, self.ln.ptr, gt.ptr, cl.ptr, dg.ptr, ws.ptr,
                  T, B, H, self.hw.ptr, self.s)
        self._done("bwd_parts")
        self.call("vocr_lstm_bias_from_parts", db.ptr, ws.ptr, T, B, H, self.s)
        self._done("bias_from_parts")
        return dg, db

    # ---- the checks of one set of results (CPU)
    def verdict(self, what, y, gt, cl, dg=None, db=None, only_bwd=False):
        """accuracy at lstm_ref's bars and `written`; -> the error rows"""
        T, B, H, refs = self.T, self.B, self.H, self.refs
        tag = "%s %s" % (self.tag, what)
        inv = ~refs.valid
        yc, gc, cc = y.cpu().view(T, B, 2 * H), gt.cpu().view(2, T, B, H, 4), cl.cpu().view(2, T, B, H)
        for nm, v in (("y", yc), ("gates", gc), ("cell", cc)):
            assert not torch.isnan(v).any(), (tag, nm, "NaN: not fully written")
        assert (yc[inv] == 0).all(), (tag, "y past lens")
        assert (gc[:, inv] == 0).all() and (cc[:, inv] == 0).all(), (tag, "gates / cell past lens")
        bw = None
        if dg is not None:
            dgc = dg.cpu().view(2, T, B, 4 * H)
            assert not torch.isnan(dgc).any(), (tag, "dgates NaN: not fully written")
            assert (dgc[:, inv] == 0).all(), (tag, "dgates past lens")
            dbc = db.cpu() if db is not None else None
            assert dbc is None or not torch.isnan(dbc).any(), (tag, "dbias NaN")
            bw = (dgc, dbc)
        errs = refs.errors((yc, gc, cc), bw)
        if only_bwd:
            errs = errs[3:]
        bad = lr.failures(errs)
        assert not bad, (tag, bad)
        return errs


def _donor_run(D, ws_ptr):
    """forward and backward of donor case D (plain device tensors) in the workspace at ws_ptr"""
    T, B, H = D["shape"]
    D["call"]("vocr_lstm_fwd", D["xp"].data_ptr(), D["wf"].data_ptr(), D["wr"].data_ptr(), D["ln"].data_ptr(), D["y"].data_ptr(),
              D["gt"].data_ptr(), D["cl"].data_ptr(), ws_ptr, T, B, H, D["hw"].data_ptr(), D["s"])
    D["call"]("vocr_lstm_bwd_bias", D["dy"].data_ptr(), D["wtf"].data_ptr(), D["wtr"].data_ptr(), D["ln"].data_ptr(), D["gt"].data_ptr(),
              D["cl"].data_ptr(), D["dg"].data_ptr(), D["db"].data_ptr(), ws_ptr, T, B, H, D["hw"].data_ptr(), D["s"])
    torch.cuda.synchronize()
    assert D["hw"].cpu().tolist() == [0, 0, 0, 0], ("donor", D["shape"])


def _donor(lib, call, stream, dev, shape):
    T, B, H = shape
    _, (lens, xproj, whh, dy, mask, _) = lc.guarded_case(T, B, H)
    G, R = 4 * H, T * B
    z = lambda *s: torch.zeros(*s, device=dev)
    return dict(shape=shape, call=call, s=stream, xp=xproj.reshape(2, R, G).to(dev), wf=whh[0].to(dev), wr=whh[1].to(dev),
                wtf=whh[0].t().contiguous().to(dev), wtr=whh[1].t().contiguous().to(dev), ln=torch.tensor(lens, dtype=I32, device=dev),
                dy=dy.reshape(R, 2 * H).to(dev), y=z(R, 2 * H), gt=z(2, R, G), cl=z(2, R, H), dg=z(2, R, G), db=z(2, G),
                hw=torch.zeros(4, dtype=I32, device=dev), nbytes=lib.vocr_lstm_workspace_bytes(T, B, H))


def _foreign(c, D):
    """a workspace of exactly this case's size that donor D ran in first: directly where D needs no more bytes than this case, else D
    runs in a workspace of its own size whose leading bytes are copied over (what a shared allocation would have left there)"""
    ws = c.fresh()
    if D["nbytes"] <= c.nbytes:
        _donor_run(D, ws.ptr)
    else:
        own = torch.full((D["nbytes"] // 4,), NAN, device=c.dev)
        _donor_run(D, own.data_ptr())
        ws.t.copy_(own[:c.nbytes // 4])
    c.P.check("%s donor %s" % (c.tag, D["shape"]))
    return ws


def _dense_case(lib, call, stream, dev, setting, T, B, H, donors):
    floor = setting.split("/")[0]
    kinds = "%s/%s" % (lc.sweep_kind(False, B, H, floor, rows=T * B), lc.sweep_kind(True, B, H, floor))
    tag = "%-10s %2d x %2d x %3d" % (setting, T, B, H)
    c = _Dense(lib, call, stream, dev, T, B, H, tag)
    # (a) a fresh NaN-filled workspace in front of every call
    y, gt, cl = c.fwd(c.fresh())
    dg, db = c.bwd_bias(c.fresh(), gt, cl)
    errs = c.verdict("fresh", y, gt, cl, dg, db)
    dg0, _ = c.bwd_bias(c.fresh(), gt, cl, bias=False)
    errs += [("bwd." + e[0],) + e[1:] for e in c.verdict("vocr_lstm_bwd", y, gt, cl, dg0, None, only_bwd=True)]
    dgp = dbp = None
    if c.parts_ok:
        dgp, dbp = c.parts(c.fresh(), gt, cl)
        errs += [("parts." + e[0],) + e[1:] for e in c.verdict("parts", y, gt, cl, dgp, dbp, only_bwd=True)]
    # the backward never reads a frame past lens: NaN there changes no bit
    inv = (~c.refs.valid).reshape(-1).to(dev)
    gtn, cln = c.P.op("gates(NaN past lens)", gt.cpu()), c.P.op("cell(NaN past lens)", cl.cpu())
    gtn.t[:, inv] = NAN
    cln.t[:, inv] = NAN
    dgn, dbn = c.bwd_bias(c.fresh(), gtn, cln)
    assert _same_bits(dgn, dg) and _same_bits(dbn, db), (tag, "the backward read gates / cell past lens")
    if c.parts_ok:
        dgn, dbn = c.parts(c.fresh(), gtn, cln)
        assert _same_bits(dgn, dgp) and _same_bits(dbn, dbp), (tag, "bwd_parts read gates / cell past lens")
    # (b) one workspace carried through the calls of a training step: each call finds its predecessor's leftovers
    ws = c.fresh()
    y2, gt2, cl2 = c.fwd(ws)
    assert _same_bits(y2, y) and _same_bits(gt2, gt) and _same_bits(cl2, cl), (tag, "carried workspace: fwd")
    dg2, db2 = c.bwd_bias(ws, gt2, cl2)
    assert _same_bits(dg2, dg) and _same_bits(db2, db), (tag, "carried workspace: bwd_bias")
    if c.parts_ok:
        dg2, db2 = c.parts(ws, gt2, cl2)
        assert _same_bits(dg2, dgp) and _same_bits(db2, dbp), (tag, "carried workspace: bwd_parts / bias_from_parts")
    y3, gt3, cl3 = c.fwd(ws)
    assert _same_bits(y3, y) and _same_bits(gt3, gt) and _same_bits(cl3, cl), (tag, "carried workspace: second fwd")
    # (c) a workspace another shape (and kind) used first
    ds = lc.DONOR[(T, B, H)]
    if ds not in donors:
        donors[ds] = _donor(lib, call, stream, dev, ds)
    D = donors[ds]
    y2, gt2, cl2 = c.fwd(_foreign(c, D))
    assert _same_bits(y2, y) and _same_bits(gt2, gt) and _same_bits(cl2, cl), (tag, "foreign workspace: fwd")
    dg2, db2 = c.bwd_bias(_foreign(c, D), gt, cl)
    assert _same_bits(dg2, dg) and _same_bits(db2, db), (tag, "foreign workspace: bwd_bias")
    if c.parts_ok:
        dg2, db2 = c.parts(_foreign(c, D), gt, cl)
        assert _same_bits(dg2, dgp) and _same_bits(db2, dbp), (tag, "foreign workspace: bwd_parts / bias_from_parts")
    # ranges: two calls on one workspace that is not refilled in between
    cuts = sorted(set(k for k in lc.RANGE_CUTS + (T - 1,) if 0 < k < T))
    for cut in cuts:
        y2, gt2, cl2 = c.fwd(c.fresh(), cut=cut)
        assert _same_bits(y2, y) and _same_bits(gt2, gt) and _same_bits(cl2, cl), (tag, "fwd_range cut at %d" % cut)
    print("ROW %s %-15s %s | bands intact, workspace-independent, ranges %s" % (tag, kinds, _fmt(errs), cuts))
    sys.stdout.flush()


def _child_sweeps(lib, call, stream, dev):
    floor = os.environ["VOCR_LSTM_SWEEP"]
    setting = floor + ("/wt" if os.environ.get("VOCR_LSTM_WRITE_THROUGH") == "1" else "")
    donors = {}
    for (T, B, H, _) in lc.GUARDED_CASES:
        _dense_case(lib, call, stream, dev, setting, T, B, H, donors)


# ---- the default-setting child
def _unaligned(lib, call, stream, dev):
    for (T, B, H) in lc.UNALIGNED_CASES:
        tag = "unaligned  %2d x %2d x %3d" % (T, B, H)
        c = _Dense(lib, call, stream, dev, T, B, H, tag)
        y, gt, cl = c.fwd(c.fresh(), wf=c.P.op("whh_fwd+4", c.whh[0], shift=1))
        errs = [("whh." + e[0],) + e[1:] for e in c.verdict("whh_fwd one float off", y, gt, cl)]
        y2, gt2, cl2 = c.fwd(c.fresh(), yshift=1)
        errs += [("y." + e[0],) + e[1:] for e in c.verdict("y one float off", y2, gt2, cl2)]
        dg, db = c.bwd_bias(c.fresh(), gt, cl, wtf=c.P.op("whht_fwd+4", c.whh[0].t().contiguous(), shift=1))
        errs += [("whht." + e[0],) + e[1:] for e in c.verdict("whht_fwd one float off", y, gt, cl, dg, db, only_bwd=True)]
        dg, db = c.bwd_bias(c.fresh(), gt, cl, dgshift=1)
        errs += [("dg." + e[0],) + e[1:] for e in c.verdict("dgates one float off", y, gt, cl, dg, db, only_bwd=True)]
        print("ROW %s step/step (generic) %s | bands intact" % (tag, _fmt(errs)))
        # gates one float off: refused in front of any launch, by every entry that takes gates
        G, R, P = c.G, c.R, c.P
        rows = 4 * (sum(c.lens[4 * k] for k in range((B + 3) // 4)) + (B + 3) // 4 + 1)
        if lib.vocr_lstm_bwd_parts_supported(T, B, H) and lib.vocr_lstm_packed_supported(B, H):
            entries = ("vocr_lstm_fwd", "vocr_lstm_bwd", "vocr_lstm_bwd_bias", "vocr_lstm_bwd_parts", "vocr_lstm_bwd_packed")
        else:
            entries = ("vocr_lstm_fwd", "vocr_lstm_bwd", "vocr_lstm_bwd_bias")
        for entry in entries:
            ws = c.fresh()
            go = P.out("gates+4", (2, R, G), shift=1)
            gi = P.op("gates+4 (read)", gt.cpu(), shift=1)
            yo, co, dgo, dbo = P.out("y", (R, 2 * H)), P.out("cell", (2, R, H)), P.out("dgates", (2, R, G)), P.out("dbias", (2, G))
            bw = (c.wtf.ptr, c.wtr.ptr, c.ln.ptr, gi.ptr, cl.ptr, dgo.ptr)
            if entry == "vocr_lstm_fwd":
                rc = lib.vocr_lstm_fwd(c.xp.ptr, c.wf.ptr, c.wr.ptr, c.ln.ptr, yo.ptr, go.ptr, co.ptr, ws.ptr, T, B, H, c.hw.ptr, stream)
            elif entry == "vocr_lstm_bwd":
                rc = lib.vocr_lstm_bwd(c.dym.ptr, *bw, ws.ptr, T, B, H, c.hw.ptr, stream)
            elif entry == "vocr_lstm_bwd_bias":
                rc = lib.vocr_lstm_bwd_bias(c.dym.ptr, *bw, dbo.ptr, ws.ptr, T, B, H, c.hw.ptr, stream)
            elif entry == "vocr_lstm_bwd_parts":
                rc = lib.vocr_lstm_bwd_parts(c.dy.ptr, c.mask.ptr, *bw, ws.ptr, T, B, H, c.hw.ptr, stream)
            else:
                rc = lib.vocr_lstm_bwd_packed(c.dy.ptr, c.mask.ptr, *bw, dbo.ptr, ws.ptr, T, B, H, rows, c.hw.ptr, stream)
            assert rc == -1 and b"align" in lib.vocr_last_error(), (tag, entry, rc, lib.vocr_last_error())
            c.P.check("%s %s refused" % (tag, entry), c.hw.t)
            for o in (go, yo, co, dgo, dbo, ws):
                assert bool(torch.isnan(o.t).all()), (tag, entry, "a refused call wrote", o.name)
            P.drop(ws, go, gi, yo, co, dgo, dbo)
        print("ROW %s gates one float off: VOCR_EINVAL from %s, outputs all-unwritten" % (tag, ", ".join(e[5:] for e in entries)))
        sys.stdout.flush()


def _packed(lib, call, stream, dev):
    from vistaocr_amd import ops
    for (T, B, H) in lc.PACKED_CASES:
        tag = "packed     %2d x %2d x %3d" % (T, B, H)
        assert lib.vocr_lstm_packed_supported(B, H) == 1, tag
        _, (lens, xproj, whh, dy, mask, refs) = lc.guarded_case(T, B, H)
        G = 4 * H
        rows, tp, td = lc.packed_layout(lens, T, B)
        nch = (B + 3) // 4
        assert rows == 4 * (sum(lens[4 * k] for k in range(nch)) + nch + 1) == ops.packed_row_count(lens, B)      # the header's formula
        tp, td = torch.tensor(tp), torch.tensor(td)
        none = td < 0

        def pk(a, n):                                   # dense [T*B][n] -> packed rows; rows without a frame hold NaN
            o = torch.full((rows, n), NAN)
            o[~none] = a.reshape(T * B, n)[td[~none]]
            return o

        def un(a):                                      # packed -> dense; frames without a packed row: 0
            a = a.cpu()
            o = torch.zeros((T * B,) + tuple(a.shape[1:]))
            o[tp >= 0] = a[tp[tp >= 0]]
            return o

        P = _Pool(dev)
        xp = P.op("xproj", torch.stack([pk(xproj[d], G) for d in range(2)]))
        wf, wr = P.op("whh_fwd", whh[0]), P.op("whh_rev", whh[1])
        wtf, wtr = P.op("whht_fwd", whh[0].t().contiguous()), P.op("whht_rev", whh[1].t().contiguous())
        ln = P.op("lens", torch.tensor(lens, dtype=I32), dtype=I32)
        dyp, mkp = P.op("dy", pk(dy, 2 * H)), P.op("dy_mask", pk(mask, 2 * H))
        hw = P.op("health", torch.zeros(4, dtype=I32), dtype=I32)
        nbytes = lib.vocr_lstm_workspace_bytes(T, B, H)
        y, gt, cl = P.out("y", (rows, 2 * H)), P.out("gates", (2, rows, G)), P.out("cell", (2, rows, H))
        dg, db = P.out("dgates", (2, rows, G)), P.out("dbias", (2, G))
        nd = none.to(dev)
        y.t[nd] = 0                                     # the caller's part of the contract: zeros where the layout has no frame
        dg.t[:, nd] = 0
        ws = P.ws(nbytes)
        call("vocr_lstm_fwd_packed", xp.ptr, wf.ptr, wr.ptr, ln.ptr, y.ptr, gt.ptr, cl.ptr, ws.ptr, T, B, H, rows, hw.ptr, stream)
        P.check(tag + " fwd_packed", hw.t)
        ws = P.ws(nbytes)
        call("vocr_lstm_bwd_packed", dyp.ptr, mkp.ptr, wtf.ptr, wtr.ptr, ln.ptr, gt.ptr, cl.ptr, dg.ptr, db.ptr, ws.ptr, T, B, H, rows,
             hw.ptr, stream)
        P.check(tag + " bwd_packed", hw.t)
        for o in (y, dg, db):
            assert not o.g.has_nan(), (tag, o.name, "NaN: not fully written")
        assert bool((y.bits()[nd] == 0).all()) and bool((dg.bits()[:, nd] == 0).all()), (tag, "rows without a frame were written")
        # frame by frame, the dense checks
        inv = ~refs.valid
        yc, dgc = un(y.t).view(T, B, 2 * H), torch.stack([un(dg.t[d]) for d in range(2)]).view(2, T, B, G)
        gc = torch.stack([un(gt.t[d]) for d in range(2)]).view(2, T, B, H, 4)
        cc = torch.stack([un(cl.t[d]) for d in range(2)]).view(2, T, B, H)
        live = (tp >= 0).view(T, B)
        for nm, v in (("gates", gc), ("cell", cc)):
            assert not torch.isnan(v[:, live]).any(), (tag, nm, "NaN in a frame of the layout")
        assert (yc[inv] == 0).all() and (dgc[:, inv] == 0).all(), (tag, "y / dgates past lens")
        errs = refs.errors((yc, gc, cc), (dgc, db.cpu()))
        assert not lr.failures(errs), (tag, lr.failures(errs))
        print("ROW %s rows %4d  %s | bands intact, rows without a frame bitwise zero" % (tag, rows, _fmt(errs)))
        sys.stdout.flush()


def _rowmap(lib, call, stream, dev):
    cases = [([9, 9, 7, 7, 7, 3, 2, 2, 1], 9), ([6, 5, 4, 3, 2, 1], 8), ([12], 12), (lc._ragged(11, 32), 11), ([5] * 8, 5),
             (lc._ragged(11, 64), 13)]
    for lens, T in cases:
        B = len(lens)
        rows, tp, td = lc.packed_layout(lens, T, B)
        for which in ("both", "to_packed", "to_dense"):
            P = _Pool(dev)
            ln = P.op("lens", torch.tensor(lens, dtype=I32), dtype=I32)
            a = P.out("to_packed", (T * B,), dtype=I32) if which != "to_dense" else None
            b = P.out("to_dense", (rows,), dtype=I32) if which != "to_packed" else None
            call("vocr_seq_rowmap", ln.ptr, T, B, rows, a.ptr if a else None, b.ptr if b else None, stream)
            P.check("rowmap %s T %d %s" % (lens, T, which))
            for o, ref in ((a, tp), (b, td)):
                if o is not None:
                    assert not o.g.has_unwritten(), ("rowmap", lens, T, which, o.name, "not fully written")
                    assert o.cpu().tolist() == ref, ("rowmap", lens, T, which, o.name)
    print("ROW seq_rowmap %d batches x (both, to_packed only, to_dense only): the documented layout, fully written, bands intact" % len(cases))


def _gather(lib, call, stream, dev):
    g = torch.Generator().manual_seed(11)
    nsrc, nrows, count = 13, 10, 0
    for n, shift in ((8, 0), (7, 0), (8, 1)):
        src = torch.rand(nsrc, n, generator=g) - 0.5
        fillv = torch.rand(n, generator=g) - 0.5
        mixed = torch.tensor([3, -1, 12, 0, -1, -1, 7, 7, 1, -1], dtype=I32)
        for mp in (mixed, torch.full((nrows,), -1, dtype=I32)):
            for with_fill in (False, True):
                P = _Pool(dev)
                s_, m_ = P.op("src", src), P.op("map", mp, dtype=I32)
                f_ = P.op("fill", fillv) if with_fill else None
                d_ = P.out("dst", (nrows, n), shift=shift)
                call("vocr_gather_rows", s_.ptr, d_.ptr, m_.ptr, nrows, n, f_.ptr if f_ else None, stream)
                P.check("gather_rows n %d shift %d" % (n, shift))
                ref = (fillv if with_fill else torch.zeros(n)).repeat(nrows, 1)
                ref[mp >= 0] = src[mp[mp >= 0].long()]
                assert torch.equal(d_.cpu(), ref), ("gather_rows", n, shift, mp.tolist(), with_fill)
                count += 1
    print("ROW gather_rows %d calls (n = 8, 7, 8 with dst one float off; fill NULL / given; a mixed map and one all -1): exact, bands intact" % count)
    worst = 0.0
    for n in (7, 96):
        nbytes = lib.vocr_gather_rows_fill_grad_workspace_bytes(n)
        assert nbytes == 64 * n * 4
        for nrows in (1, 63, 64, 65, 4097):
            dout = torch.rand(nrows, n, generator=g) * 2 - 1
            mp = torch.where(torch.rand(nrows, generator=g) < 0.5, torch.tensor(-1), torch.tensor(0)).to(I32)
            mp[0] = -1
            sel = mp < 0
            ref = dout[sel].double().sum(0)
            bar = 1e-6 * dout[sel].double().abs().sum(0)
            got = []
            for _ in range(2):
                P = _Pool(dev)
                d_, m_ = P.op("dout", dout), P.op("map", mp, dtype=I32)
                o_, ws = P.out("dfill", (n,)), P.ws(nbytes)
                call("vocr_gather_rows_fill_grad", d_.ptr, m_.ptr, nrows, n, o_.ptr, ws.ptr, stream)
                P.check("gather_rows_fill_grad n %d nrows %d" % (n, nrows))
                got.append(o_.cpu())
            assert not torch.isnan(got[0]).any(), ("fill_grad", n, nrows, "NaN")
            assert torch.equal(got[0].view(I32), got[1].view(I32)), ("fill_grad", n, nrows, "two runs differ")
            err = (got[0].double() - ref).abs()
            assert bool((err <= bar).all()), ("fill_grad", n, nrows, float(err.max()), float(bar.min()))
            worst = max(worst, float((err / bar).max()))
    print("ROW gather_rows_fill_grad n = 7, 96 x nrows = 1, 63, 64, 65, 4097: worst e_k / bar %.3f, repeatable, bands intact" % worst)


def child_main(mode):
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vistaocr_amd import _lib, ops
    lib, dev, stream = _lib.load(), torch.device("cuda:0"), ops._stream()
    if mode == "sweeps":
        _child_sweeps(lib, _lib.call, stream, dev)
    else:
        _packed(lib, _lib.call, stream, dev)
        _rowmap(lib, _lib.call, stream, dev)
        _gather(lib, _lib.call, stream, dev)
        _unaligned(lib, _lib.call, stream, dev)
    torch.cuda.synchronize()
    print("CHILD OK")
