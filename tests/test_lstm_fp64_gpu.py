"""GPU: every BiLSTM sweep kind, the packed-row entry points and the layer op against an fp64 restatement of the recurrence
(tests/lstm_ref.py; the bars and their reasoning are there, beside the restatement the mutant tests of tests/test_lstm_ref_cpu.py hold
them to).  Random x-projections go straight into the sweeps (no GEMM in the way); the backward consumes the kernel's own gates and cell.

The library reads VOCR_LSTM_SWEEP / VOCR_LSTM_WRITE_THROUGH once per process, so every setting runs in a child process of its own, one
after the other (persistent sweeps must not share a device).  Every case prints e_k (the kernel's max abs error against fp64) and e_32
(the fp32 restatement's) - run with -s to see the table."""
import os
import subprocess
import sys

import pytest
import torch

from tests import lstm_ref as lr
from tests.lstm_cases import _ALL, SETTINGS, _ragged, case, make_inputs, sweep_kind          # noqa: F401 (shared with the guarded suite)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    """the CPU references at no more than 16 threads (what a GPU host gives one command); the caller's count is restored afterwards"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


# (T, B, H, lens, regimes, floors): what each (shape, floor) pair reaches, forward / backward, by the rule (sweep_kind of tests/lstm_cases.py):
#   294 x 32 x 512         wide4: wide4/wide4    chain4: chain4/chain4    chain16: chain16/chain16   step: step/step   (the bench shape)
#   588 x 32 x 512         wide4 and step only (configs[3]'s long ragged line)
#   60 x 17 x 512          wide4: wide4/wide4    chain4: chain4/chain4    chain16: chain16/chain16 (the wide4 lower boundary)
#   60 x 16 x 512          wide4, chain4: chain4/chain4 (nt4 = 4: no wide members)     chain16: chain16/chain16
#   50 x 30 / 7 x 256      wide4, chain4: chain4/chain4 (a partial last chain)          chain16: chain16/chain16
#   40 x 64 x 512          every floor but step: chain16/chain16 (nt4 = 16)
#   40 x 33 x 128          every floor but step: chain16/chain16
#   40 x 48 x 64           every floor but step: chain16 forward / step backward (no backward fast path below H = 128)
#   30 x 5 x 48, 20 x 3 x 16, 12 x 4 x 1024: step/step (the generic per-step kernels) at every floor
#   1 x 1 x 256            wide4, chain4: chain4/chain4;  2 x 3 x 512: the same (T = 1, T = 2, B = 1)
CASES = [
    (294, 32, 512, "full", ("ref",), _ALL),
    (294, 32, 512, "ragged", ("ref",), _ALL),
    (588, 32, 512, "ragged", ("ref",), ("wide4", "step")),
    (60, 17, 512, "ragged", ("ref", "small"), _ALL),
    (60, 16, 512, "ragged", ("ref",), _ALL),
    (50, 30, 256, "ragged", ("ref", "small"), _ALL),
    (50, 7, 256, "ragged", ("ref",), _ALL),
    (40, 64, 512, "ragged", ("ref", "sat", "small"), _ALL),
    (40, 33, 128, "ragged", ("ref", "sat"), _ALL),
    (40, 48, 64, "ragged", ("ref", "sat", "small"), _ALL),
    (30, 5, 48, "ragged", ("ref", "sat", "small"), _ALL),
    (20, 3, 16, "ragged", ("ref", "sat"), _ALL),
    (12, 4, 1024, "ragged", ("ref", "sat"), _ALL),
    (1, 1, 256, "full", ("ref", "sat"), _ALL),
    (2, 3, 512, "ragged", ("ref", "sat"), _ALL),
]


def _run_child(code, args, env=None, timeout=300):
    r = subprocess.run([sys.executable, "-c", code] + [str(a) for a in args], env=dict(os.environ, **(env or {})), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, (args, env, r.stdout[-1000:], r.stderr[-2000:])
    return r.stdout


def _report(tag, errs):
    for nm, ek, e32, b in errs:
        print("%-44s %-7s e_k %.3e  e_32 %.3e  bar %.3e  (%s)" % (tag, nm, ek, e32, b, "ok" if ek <= b else "FAIL"))


_SWEEP_CHILD = r'''
import sys, torch
sys.path.insert(0, %(root)r)
from vistaocr_amd import _lib, ops
from vistaocr_amd._lib import call
lib = _lib.load(); dev = torch.device("cuda:0"); s = torch.cuda.current_stream().cuda_stream
cases = torch.load(sys.argv[1])
out = {}
for key, c in cases.items():
    T, B, H, lens = c["T"], c["B"], c["H"], c["lens"]
    G, R = 4 * H, T * B
    xp = c["xproj"].reshape(2, R, G).to(dev)
    whh = c["whh"].to(dev)
    wf, wr = whh[0], whh[1]
    wtf, wtr = ops.transpose2d(wf), ops.transpose2d(wr)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    dy = c["dy"].reshape(R, 2 * H).to(dev); mask = c["mask"].reshape(R, 2 * H).to(dev)
    y = torch.full((R, 2 * H), float("nan"), device=dev)
    gt = torch.zeros(2, R, G, device=dev); cl = torch.zeros(2, R, H, device=dev)
    ws = torch.zeros(lib.vocr_lstm_workspace_bytes(T, B, H) // 4 + 16, device=dev)
    hw = torch.zeros(4, dtype=torch.int32, device=dev)
    call("vocr_lstm_fwd", xp.data_ptr(), wf.data_ptr(), wr.data_ptr(), lens_d.data_ptr(), y.data_ptr(), gt.data_ptr(), cl.data_ptr(), ws.data_ptr(), T, B, H, hw.data_ptr(), s)
    dg = torch.full((2, R, G), float("nan"), device=dev); db = torch.full((2, G), float("nan"), device=dev)
    dym = dy * mask
    call("vocr_lstm_bwd_bias", dym.data_ptr(), wtf.data_ptr(), wtr.data_ptr(), lens_d.data_ptr(), gt.data_ptr(), cl.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), T, B, H, hw.data_ptr(), s)
    res = {"y": y, "gates": gt, "cell": cl, "dgates": dg, "dbias": db}
    if lib.vocr_lstm_bwd_parts_supported(T, B, H):
        dg2 = torch.full((2, R, G), float("nan"), device=dev); db2 = torch.full((2, G), float("nan"), device=dev)
        call("vocr_lstm_bwd_parts", dy.data_ptr(), mask.data_ptr(), wtf.data_ptr(), wtr.data_ptr(), lens_d.data_ptr(), gt.data_ptr(), cl.data_ptr(), dg2.data_ptr(), ws.data_ptr(), T, B, H, hw.data_ptr(), s)
        call("vocr_lstm_bias_from_parts", db2.data_ptr(), ws.data_ptr(), T, B, H, s)
        res["dgates_parts"], res["dbias_parts"] = dg2, db2
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in res.items()}
    res["health"] = int(hw[0])
    out[key] = res
    del xp, y, gt, cl, dg, db, ws, dy, mask, dym
torch.save(out, sys.argv[2])
print("CHILD OK", len(out))
'''


def _check_dense(tag, T, B, H, lens, refs, r):
    """the common checks of a dense-layout result r (the child's tensors in the library's layouts)"""
    assert r["health"] == 0, (tag, r["health"])
    fwd = (r["y"].view(T, B, 2 * H), r["gates"].view(2, T, B, H, 4), r["cell"].view(2, T, B, H))
    bwd = (r["dgates"].view(2, T, B, 4 * H), r["dbias"])
    for nm, v in list(r.items()):
        if torch.is_tensor(v):
            assert not torch.isnan(v).any(), (tag, nm, "NaN")
    inv = ~refs.valid
    assert (fwd[0][inv] == 0).all(), (tag, "y past lens")
    assert (bwd[0][:, inv] == 0).all(), (tag, "dgates past lens")
    errs = refs.errors(fwd, bwd)
    _report(tag, errs)
    bad = lr.failures(errs)
    if "dgates_parts" in r:
        dgp = r["dgates_parts"].view(2, T, B, 4 * H)
        assert (dgp[:, inv] == 0).all(), (tag, "parts: dgates past lens")
        pe = [("parts." + e[0],) + tuple(e[1:]) for e in refs.errors(fwd, (dgp, r["dbias_parts"]))[3:]]
        _report(tag, pe)
        bad += lr.failures(pe)
    return bad


def test_every_sweep_kind_against_fp64(tmp_path):
    seen = {False: set(), True: set()}
    bad = []
    for setting in SETTINGS:
        floor = setting.split("/")[0]
        todo = {}
        for (T, B, H, lk, regimes, floors) in CASES:
            if floor not in floors:
                continue
            for rg in regimes:
                lens, xproj, whh, dy, mask, _ = case(T, B, H, lk, rg)
                todo["%d_%d_%d_%s_%s" % (T, B, H, lk, rg)] = dict(T=T, B=B, H=H, lens=lens, xproj=xproj, whh=whh, dy=dy, mask=mask)
                seen[False].add(sweep_kind(False, B, H, floor, rows=T * B))
                seen[True].add(sweep_kind(True, B, H, floor))
        fin, fout = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
        torch.save(todo, fin)
        _run_child(_SWEEP_CHILD % dict(root=ROOT), [fin, fout],
                   env=dict(VOCR_LSTM_SWEEP=floor, VOCR_LSTM_WRITE_THROUGH="1" if "/wt" in setting else "0"), timeout=600)
        os.unlink(fin)
        outs = torch.load(fout)
        os.unlink(fout)
        for key, r in outs.items():
            T, B, H = (int(v) for v in key.split("_")[:3])
            lk, rg = key.split("_")[3:]
            lens, _, _, _, _, refs = case(T, B, H, lk, rg)
            tag = "%s %s" % (setting, key)
            bad += [(tag,) + e for e in _check_dense(tag, T, B, H, lens, refs, r)]
        del outs
    for bw in (False, True):
        assert seen[bw] == set(_ALL), ("backward" if bw else "forward", seen[bw])
    assert not bad, bad


_PACKED_CHILD = r'''
import sys, torch
sys.path.insert(0, %(root)r)
from vistaocr_amd import _lib, ops
from vistaocr_amd._lib import call
lib = _lib.load(); dev = torch.device("cuda:0"); s = torch.cuda.current_stream().cuda_stream
cases = torch.load(sys.argv[1])
out = {}
for key, c in cases.items():
    T, B, H, lens = c["T"], c["B"], c["H"], c["lens"]
    G = 4 * H
    assert lib.vocr_lstm_packed_supported(B, H)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    maps = ops.SeqRowMaps(lens_d, lens, T, B)
    R = maps.rows
    pk = lambda a, n: ops.gather_rows(a.reshape(T * B, n).to(dev), maps.to_dense, R)        # dense -> packed rows, zero groups 0
    un = lambda a: ops.gather_rows(a, maps.to_packed, T * B)                                 # packed -> dense, no row: 0
    xp = torch.stack([pk(c["xproj"][d], G) for d in range(2)])
    whh = c["whh"].to(dev); wf, wr = whh[0], whh[1]
    wtf, wtr = ops.transpose2d(wf), ops.transpose2d(wr)
    dy, mask = pk(c["dy"], 2 * H), pk(c["mask"], 2 * H)
    zero = (maps.to_dense < 0)
    y = torch.zeros(R, 2 * H, device=dev)              # the caller zero-fills y and dgates (include/vocr.h)
    gt = torch.full((2, R, G), float("nan"), device=dev); cl = torch.full((2, R, H), float("nan"), device=dev)
    ws = torch.zeros(lib.vocr_lstm_workspace_bytes(T, B, H) // 4 + 16, device=dev)
    hw = torch.zeros(4, dtype=torch.int32, device=dev)
    call("vocr_lstm_fwd_packed", xp.data_ptr(), wf.data_ptr(), wr.data_ptr(), lens_d.data_ptr(), y.data_ptr(), gt.data_ptr(), cl.data_ptr(), ws.data_ptr(), T, B, H, R, hw.data_ptr(), s)
    dg = torch.zeros(2, R, G, device=dev); db = torch.full((2, G), float("nan"), device=dev)
    call("vocr_lstm_bwd_packed", dy.data_ptr(), mask.data_ptr(), wtf.data_ptr(), wtr.data_ptr(), lens_d.data_ptr(), gt.data_ptr(), cl.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), T, B, H, R, hw.data_ptr(), s)
    torch.cuda.synchronize()
    res = {"y": un(y), "gates": torch.stack([un(gt[d].contiguous()) for d in range(2)]), "cell": torch.stack([un(cl[d].contiguous()) for d in range(2)]),
           "dgates": torch.stack([un(dg[d].contiguous()) for d in range(2)]), "dbias": db.clone(),
           "zero_y": int((y[zero] != 0).sum()), "zero_dg": int((dg[:, zero] != 0).sum())}
    torch.cuda.synchronize()
    res = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.items()}
    res["health"] = int(hw[0])
    out[key] = res
torch.save(out, sys.argv[2])
print("CHILD OK", len(out))
'''


def test_packed_rows_against_fp64(tmp_path):
    shapes = [(294, 32, 512), (50, 30, 256), (50, 7, 256)]
    todo = {}
    for T, B, H in shapes:
        lens, xproj, whh, dy, mask, _ = case(T, B, H, "ragged", "ref")
        todo["%d_%d_%d" % (T, B, H)] = dict(T=T, B=B, H=H, lens=lens, xproj=xproj, whh=whh, dy=dy, mask=mask)
    fin, fout = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save(todo, fin)
    _run_child(_PACKED_CHILD % dict(root=ROOT), [fin, fout], timeout=300)
    os.unlink(fin)
    outs = torch.load(fout)
    os.unlink(fout)
    bad = []
    for T, B, H in shapes:
        r = outs["%d_%d_%d" % (T, B, H)]
        lens, _, _, _, _, refs = case(T, B, H, "ragged", "ref")
        tag = "packed %d_%d_%d" % (T, B, H)
        assert r["zero_y"] == 0 and r["zero_dg"] == 0, (tag, "zero groups written", r["zero_y"], r["zero_dg"])
        bad += [(tag,) + e for e in _check_dense(tag, T, B, H, lens, refs, r)]
    assert not bad, bad


# ---- (c) the layer op (x-projection GEMM + sweeps + gradient GEMMs) against nn.LSTM in double
_LAYER_CHILD = r'''
import sys, torch
sys.path.insert(0, %(root)r)
from vistaocr_amd import ops
if sys.argv[3] == "one_view":
    ops._X6_TWO_VIEWS = False
dev = torch.device("cuda:0")
cases = torch.load(sys.argv[1])
out = {}
for key, c in cases.items():
    T, B, H, D, lens, packed = c["T"], c["B"], c["H"], c["D"], c["lens"], c["packed"]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    x = c["x"].reshape(T * B, D).to(dev)
    dy = c["dy"].reshape(T * B, 2 * H).to(dev)
    rows = 0
    if packed:
        maps = ops.SeqRowMaps(lens_d, lens, T, B)
        rows = maps.rows
        x = ops.gather_rows(x, maps.to_dense, rows)
        dy = ops.gather_rows(dy, maps.to_dense, rows)
    params = [p.to(dev).requires_grad_(True) for p in c["params"]]
    xg = x.clone().requires_grad_(True)
    try:
        y = ops.BiLstmLayerFn.apply(xg, lens_d, T, B, *params, None, False, 0.0, 0, rows)
        y.backward(dy)
    except RuntimeError as e:
        if "failed (-1)" not in str(e):           # only a call the library refused (VOCR_EINVAL: nothing ran) is reported per case
            raise
        out[key] = {"error": str(e)}
        continue
    yv, dx = y.detach(), xg.grad
    if packed:
        yv, dx = ops.gather_rows(yv, maps.to_packed, T * B), ops.gather_rows(dx, maps.to_packed, T * B)
    torch.cuda.synchronize()
    out[key] = {"y": yv.cpu(), "dx": dx.cpu(), "g": [p.grad.cpu() for p in params], "health": int(ops.health(dev)[0])}
torch.save(out, sys.argv[2])
print("CHILD OK", len(out))
'''

# (T, B, D, H, packed): H = 32 and 96 are G = 4H = 128 (2j + 1), whose recurrent weight gradient cannot take the split products' views;
# H = 48: f32 GEMMs and the generic step kernel; B = 27: the recurrent product on gemm_pair (the time shift is not whole k16 steps)
LAYER_CASES = [(24, 32, 256, 32, 0), (24, 32, 256, 96, 0), (24, 32, 256, 128, 0), (24, 32, 256, 256, 0), (24, 32, 256, 512, 0),
               (24, 32, 256, 48, 0), (24, 27, 256, 512, 0), (41, 32, 256, 512, 1), (50, 30, 256, 256, 1)]
LAYER_MODES = (("bf16x6", "two_views"), ("fp16x3", "two_views"), ("f32", "two_views"), ("bf16x6", "one_view"))
_PNAMES = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse",
           "bias_hh_l0_reverse"]


def test_bilstm_layer_against_fp64_nn_lstm(tmp_path):
    from tests.test_ops_gpu import _ref_bilstm
    todo, refs = {}, {}
    for (T, B, D, H, packed) in LAYER_CASES:
        g = torch.Generator().manual_seed(T * 7 + B * 3 + H + packed)
        lens = sorted([max(1, T - (3 * i) // 2) for i in range(B)], reverse=True)
        x = (torch.rand(T, B, D, generator=g) - 0.5) * 2
        for b in range(B):
            x[lens[b]:, b] = 0.37
        params = [(torch.rand(*s, generator=g) - 0.5) * 0.16 for s in [(4 * H, D), (4 * H, H), (4 * H,), (4 * H,)] * 2]
        dy = (torch.rand(T, B, 2 * H, generator=g) - 0.5) * 0.1
        vm = lr.valid_mask(T, B, lens)
        dy = dy * vm.unsqueeze(2)                     # nothing flows back from a padded frame
        key = "%d_%d_%d_%d_%d" % (T, B, D, H, packed)
        todo[key] = dict(T=T, B=B, D=D, H=H, lens=lens, packed=packed, x=x, params=params, dy=dy)
        xr = x.double().requires_grad_(True)
        m, yr = _ref_bilstm(xr, lens, [p.double() for p in params], H, dtype=torch.float64)
        yr.backward(dy.double())
        dx64 = xr.grad * vm.unsqueeze(2)
        refs[key] = (yr.detach(), dx64, [getattr(m, nm).grad for nm in _PNAMES])
    fin = str(tmp_path / "in.pt")
    torch.save(todo, fin)
    bad = []
    for scheme, views in LAYER_MODES:
        fout = str(tmp_path / "out.pt")
        _run_child(_LAYER_CHILD % dict(root=ROOT), [fin, fout, views], env=dict(VOCR_LSTM_GEMM=scheme), timeout=300)
        outs = torch.load(fout)
        os.unlink(fout)
        for key, r in outs.items():
            T, B, D, H, packed = (int(v) for v in key.split("_"))
            y64, dx64, g64 = refs[key]
            tag = "layer %s/%s %s" % (scheme, views, key)
            if "error" in r:
                print("%-44s ERROR %s" % (tag, r["error"]))
                bad.append((tag, r["error"]))
                continue
            assert r["health"] == 0, tag
            errs = [("y", lr.max_err(r["y"].view(T, B, 2 * H), y64), 2e-5),
                    ("dx", lr.max_err(r["dx"].view(T, B, D), dx64), 1e-4 * float(dx64.abs().max()))]
            errs += [("d" + nm, lr.max_err(gk, gr), 2e-4 * float(gr.abs().max())) for nm, gk, gr in zip(_PNAMES, r["g"], g64)]
            for nm, ek, b in errs:
                print("%-44s %-26s e_k %.3e  bar %.3e  (%s)" % (tag, nm, ek, b, "ok" if ek <= b else "FAIL"))
            bad += [(tag, nm, ek, b) for nm, ek, b in errs if not ek <= b]
    os.unlink(fin)
    assert not bad, bad


# ---- (d) the long-input boundary: T x B = 262 400 rows at H = 512 (the reverse direction's rows start past 2^18: a 32-bit byte offset of
# gates / xproj that included the direction's plane wrapped there).  No fp64 here (over a TFLOP on the CPU): each persistent kind against
# one launch per step at the reorder bar of test_persistent_sweeps_match_per_step_launches, in ONE child per kind.  The per-step
# reference is the generic step kernel, which a W_hh that is not 16-byte aligned selects (lstm_fwd_impl / lstm_bwd_impl: the fast and
# persistent paths need aligned operands); it addresses in 64 bits.  About 30 GB of device memory per child, freed when it exits.
_LONG_CHILD = r'''
import sys, torch
sys.path.insert(0, %(root)r)
from vistaocr_amd import _lib, ops
from vistaocr_amd._lib import call
lib = _lib.load(); dev = torch.device("cuda:0"); s = torch.cuda.current_stream().cuda_stream
T, B, H, packed = %(T)d, %(B)d, %(H)d, %(packed)d
G, R = 4 * H, T * B
lens = [T] * (B - 4) + [T - 1, T - 2, T - 3, T - 5]
lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
g = torch.Generator(device=dev).manual_seed(5)
xp = (torch.rand(2, R, G, generator=g, device=dev) - 0.5)
dy = (torch.rand(R, 2 * H, generator=g, device=dev) - 0.5)
for b in range(B):
    dy.view(T, B, 2 * H)[lens[b]:, b] = 0
def unaligned(a):
    """a copy of matrix a whose data starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(a.numel() + 4, device=dev)
    v = buf[1:1 + a.numel()].view(a.shape)
    v.copy_(a)
    return v
def sweep(wf, wr, wtf, wtr, rows=0, maps=None):
    R_ = rows or R
    x = xp if not rows else torch.stack([ops.gather_rows(xp[d], maps.to_dense, R_) for d in range(2)])
    d_ = dy if not rows else ops.gather_rows(dy, maps.to_dense, R_)
    y = torch.zeros(R_, 2 * H, device=dev) if rows else torch.full((R_, 2 * H), float("nan"), device=dev)
    gt = torch.zeros(2, R_, G, device=dev); cl = torch.zeros(2, R_, H, device=dev)
    dg = torch.zeros(2, R_, G, device=dev) if rows else torch.full((2, R_, G), float("nan"), device=dev)
    ws = torch.zeros(lib.vocr_lstm_workspace_bytes(T, B, H) // 4 + 16, device=dev); hw = torch.zeros(4, dtype=torch.int32, device=dev)
    if rows:
        call("vocr_lstm_fwd_packed", x.data_ptr(), wf.data_ptr(), wr.data_ptr(), lens_d.data_ptr(), y.data_ptr(), gt.data_ptr(), cl.data_ptr(), ws.data_ptr(), T, B, H, R_, hw.data_ptr(), s)
        call("vocr_lstm_bwd_packed", d_.data_ptr(), None, wtf.data_ptr(), wtr.data_ptr(), lens_d.data_ptr(), gt.data_ptr(), cl.data_ptr(), dg.data_ptr(), None, ws.data_ptr(), T, B, H, R_, hw.data_ptr(), s)
    else:
        call("vocr_lstm_fwd", x.data_ptr(), wf.data_ptr(), wr.data_ptr(), lens_d.data_ptr(), y.data_ptr(), gt.data_ptr(), cl.data_ptr(), ws.data_ptr(), T, B, H, hw.data_ptr(), s)
        call("vocr_lstm_bwd", d_.data_ptr(), wtf.data_ptr(), wtr.data_ptr(), lens_d.data_ptr(), gt.data_ptr(), cl.data_ptr(), dg.data_ptr(), ws.data_ptr(), T, B, H, hw.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(hw[0]) == 0, int(hw[0])
    del x, d_, ws
    if rows:                                      # back to the dense layout: frames without a packed row read 0, as the dense sweeps write them
        unp = lambda a: torch.stack([ops.gather_rows(a[d].contiguous(), maps.to_packed, R) for d in range(2)])
        y, gt, cl, dg = ops.gather_rows(y, maps.to_packed, R), unp(gt), unp(cl), unp(dg)
    return [y, gt, cl, dg]
def cmp(a, b):
    """(max |a - b|, max |b|) in chunks; NaN anywhere -> inf"""
    e = m = 0.0
    fa, fb = a.reshape(-1), b.reshape(-1)
    for i in range(0, fa.numel(), 1 << 26):
        d = (fa[i:i + (1 << 26)] - fb[i:i + (1 << 26)]).abs()
        e = max(e, float("inf") if bool(torch.isnan(d).any()) else float(d.max()))
        m = max(m, float(fb[i:i + (1 << 26)].abs().max()))
    return e, m
wf, wr = (torch.rand(G, H, generator=g, device=dev) - 0.5) * 0.16, (torch.rand(G, H, generator=g, device=dev) - 0.5) * 0.16
wtf, wtr = ops.transpose2d(wf), ops.transpose2d(wr)
ref = sweep(unaligned(wf), unaligned(wr), unaligned(wtf), unaligned(wtr))        # one launch per step (the generic kernels)
runs = [("dense", {})]
if packed:
    maps = ops.SeqRowMaps(lens_d, lens, T, B)
    ok = bool(lib.vocr_lstm_packed_supported(B, H))
    print("PACKED rows %%d supported %%d" %% (maps.rows, ok))
    if ok:
        runs.append(("packed", dict(rows=maps.rows, maps=maps)))
for name, kw in runs:
    got = sweep(wf, wr, wtf, wtr, **kw)
    for nm, a, b in zip(("y", "gates", "cell", "dgates"), got, ref):
        e, m = cmp(a, b)
        print("LONG %%s %%s %%s max|diff| %%.3e bar %%.3e" %% (name, nm, "ok" if e <= 3e-5 * m else "FAIL", e, 3e-5 * m))
    del got
print("CHILD OK")
'''


LONG_T, LONG_B, LONG_H = 8200, 32, 512


@pytest.mark.parametrize("floor", ["wide4", "chain4", "chain16"])
def test_long_input_boundary(floor):
    T, B, H = LONG_T, LONG_B, LONG_H
    assert T * B > 2 ** 18 and T * B * 2 * H * 4 < 2 ** 31          # past the old wrap, inside the library's 2-GB plane guard
    assert sweep_kind(False, B, H, floor, rows=T * B) == floor and sweep_kind(True, B, H, floor) == floor
    packed = floor in ("wide4", "chain4")                             # the packed rows need a 4-row chain sweep
    out = _run_child(_LONG_CHILD % dict(root=ROOT, T=T, B=B, H=H, packed=int(packed)), [], env=dict(VOCR_LSTM_SWEEP=floor), timeout=600)
    print(out)
    lines = [l for l in out.splitlines() if l.startswith("LONG ")]
    assert len(lines) == (8 if packed else 4), out
    assert all(" ok " in l for l in lines), out
    if packed:
        # the library takes packed rows of this size (rows * 2H * 4 < 2 GB), and so does the model's guard (model.py: the same bound)
        lens = [T] * (B - 4) + [T - 1, T - 2, T - 3, T - 5]          # the child's
        rows = 4 * (sum(lens[4 * c] for c in range(8)) + 8 + 1)
        assert rows > 2 ** 18
        assert "PACKED rows %d supported 1" % rows in out, out
        assert rows * 2 * H * 4 < 2 ** 31
