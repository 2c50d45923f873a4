"""Time vocr_edit_stats (ErrorScorer) where validation and n-best analysis use it, on lines of random symbols of the English alphabet
(96 classes, the space among them) whose hypothesis has 10 % of the characters replaced:

  (a) one configs[1] batch, 32 lines of about 100 characters: ErrorScorer.score (character and word statistics, hypotheses on the
      device, references in the collate's form on the host; the call ends with its one device-to-host copy) against what
      test_on_val does per batch, the compute_cer_wer loop on this box's CPU - and the eval forward of configs[1]'s model in the
      same run;
  (b) 4096 pairs (B = 32 references, K = 128 hypotheses each), distances only (ops.edit_stats, want = EDIT_CHARS, everything on the
      device) against the same anti-diagonal recursion written in batched torch on the same GPU (it lives here, not in the product);
  (c) the trace (operation counts, operations, confusion matrix) on against off, for both shapes.

The integers of (a) and (b) are compared with the comparison's.  Every leg runs in a child process of its own and the legs alternate;
a timed window is HIP events around enough back-to-back calls for about 50 ms (the CPU leg: perf_counter around whole batches).
Lane packing of short pairs was not built, so there is no A/B of it.
  (e) with an A/B library (python -m vistaocr_amd.build --experiments, scripts/_cut/libvocr.so; skipped, and said so, without one) the
      4096 pairs with the recursion's lane shift as ds_bpermute (__shfl_up) or as a DPP wave_shr (VOCR_ES_DPP = 0 / 1), and with 256 or
      2048 workgroups where the trace's back pointers all fit the LDS (VOCR_ES_GTRACE_LDS).
Output: profiles/r12_score_bench.txt.

    python scripts/score_bench.py [--repeats 10] [--rounds 2] [--out profiles/r12_score_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, K, LEN = 32, 128, 100
LEGS = ("score", "cpu", "pairs", "torch", "forward")
CUT = os.path.join(ROOT, "scripts", "_cut", "libvocr.so")
AB = ((0, 256), (1, 256), (0, 2048), (1, 2048))                   # (VOCR_ES_DPP, VOCR_ES_GTRACE_LDS)


def _windows(fn, warmup, repeats, window_ms=50.0):
    """ms per call of `repeats` windows of HIP events around n back-to-back calls (n chosen for a window of about window_ms)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    n = max(1, int(round(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / n)
    return ms


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def data(n_hyp):
    """(alphabet, hyps [B][n_hyp] label lists, refs [B] label lists): references of 90 .. 110 random labels; a hypothesis is its
    reference with 10 % of the characters replaced (and, for n_hyp > 1, a few dropped, so that the ranks differ in length)."""
    import vistaocr_amd as va
    al = va.english_alphabet()
    rng = np.random.default_rng(12)
    refs = [rng.integers(1, len(al), int(rng.integers(LEN - 10, LEN + 11))).tolist() for _ in range(B)]
    hyps = []
    for r in refs:
        row = []
        for q in range(n_hyp):
            h = [int(rng.integers(1, len(al))) if rng.random() < 0.1 else v for v in r]
            if q:
                h = [v for v in h if rng.random() >= 0.02]
            row.append(h)
        hyps.append(row)
    return al, hyps, refs


def device_inputs(hyps, refs):
    n = len(hyps[0])
    T = max(len(h) for row in hyps for h in row)
    lab = np.zeros((B, n, T), dtype=np.int32)
    ln = np.zeros((B, n), dtype=np.int32)
    for b, row in enumerate(hyps):
        for q, h in enumerate(row):
            lab[b, q, :len(h)] = h
            ln[b, q] = len(h)
    targets = torch.tensor([v for r in refs for v in r], dtype=torch.int32)
    target_lens = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    return torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda(), targets, target_lens


def torch_distances(a, la, b, lb):
    """Levenshtein distances of P pairs at once, a [P, La], b [P, Lb] int64 class labels on the device: the anti-diagonal recursion,
    vectorised over (pair, cell of the diagonal), a Python loop over the La + Lb - 1 diagonals."""
    P, La = a.shape
    Lb = b.shape[1]
    dev = a.device
    big = La + Lb + 1
    i = torch.arange(La + 1, device=dev)
    prev2 = torch.full((P, La + 1), big, device=dev, dtype=torch.int64)          # diagonal d - 2, indexed by i
    prev1 = torch.full((P, La + 1), big, device=dev, dtype=torch.int64)          # diagonal d - 1
    prev2[:, 0] = 0                                                              # d = 0: cell (0, 0)
    prev1[:, 0], prev1[:, 1] = 1, 1                                              # d = 1: cells (0, 1) and (1, 0)
    out = torch.zeros(P, device=dev, dtype=torch.int64)
    target = la + lb
    out = torch.where(target == 0, torch.zeros_like(out), out)
    out = torch.where(target == 1, torch.ones_like(out), out)
    bpad = torch.cat([b, b.new_zeros(P, La + 1)], dim=1)
    for d in range(2, La + Lb + 1):
        j = d - i                                                                # cell (i, d - i)
        inside = (i >= 1) & (j >= 1) & (j <= Lb)
        jj = j.clamp(1, Lb) - 1
        ne = (a[:, (i - 1).clamp(0, La - 1)] != bpad[:, jj]).to(torch.int64)
        diag = torch.cat([prev2.new_full((P, 1), big), prev2[:, :-1]], dim=1) + ne       # (i-1, j-1) sits on d - 2 at i - 1
        up = torch.cat([prev1.new_full((P, 1), big), prev1[:, :-1]], dim=1) + 1          # (i-1, j) on d - 1 at i - 1
        left = prev1 + 1                                                                 # (i, j-1) on d - 1 at i
        cur = torch.minimum(torch.minimum(diag, up), left)
        cur = torch.where(inside[None, :], cur, torch.full_like(cur, big))
        if d <= Lb:
            cur[:, 0] = d                                                        # cell (0, d)
        if d <= La:
            cur[:, d] = d                                                        # cell (d, 0)
        hit = target == d
        out = torch.where(hit, cur.gather(1, la[:, None].clamp(0, La))[:, 0], out)
        prev2, prev1 = prev1, cur
    return out


def leg(name, args):
    """One leg in this process: {"key": [ms per call of every window], ..} and, under "check", integers to compare."""
    import vistaocr_amd as va
    from vistaocr_amd import ops
    from vistaocr_amd.textutils import compute_cer_wer
    if args.cut:
        import vistaocr_amd._lib as L
        L.LIB_PATH = CUT
    out = {}
    if name == "forward":
        hp = dict(num_in_channels=1, input_line_height=30, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3,
                  num_lstm_hidden_units=512, p_lstm_dropout=0.5)
        torch.manual_seed(0)
        model = va.CnnOcrModel(alphabet=va.english_alphabet(), verbose=False, **hp).cuda().eval()
        x = torch.rand(B, 1, 30, 600, device="cuda")
        widths = torch.tensor([600] * B)
        with torch.no_grad():
            out["forward"] = _windows(lambda: model(x, widths), args.warmup, args.repeats)
        return out
    if name in ("score", "cpu"):
        al, hyps, refs = data(1)
        if name == "cpu":
            ux = lambda s: " ".join(al.idx_to_char[k] for k in s)
            hs, rs = [ux(row[0]) for row in hyps], [ux(r) for r in refs]
            ms = []
            for _ in range(max(args.repeats // 2, 3)):
                t0 = time.perf_counter()
                got = [compute_cer_wer(h, r) for h, r in zip(hs, rs)]
                ms.append((time.perf_counter() - t0) * 1e3)
            out["cpu"] = ms
            out["check"] = {"cer": [g[0] for g in got], "wer": [g[1] for g in got]}
            return out
        lab, ln, targets, target_lens = device_inputs(hyps, refs)
        sc = va.ErrorScorer(al)
        lab1, ln1 = lab[:, 0].contiguous(), ln[:, 0].contiguous()
        out["score"] = _windows(lambda: sc.score(lab1, ln1, targets, target_lens), args.warmup, args.repeats)
        out["score+trace"] = _windows(lambda: sc.score(lab1, ln1, targets, target_lens, trace=True), args.warmup, args.repeats)
        res = sc.score(lab1, ln1, targets, target_lens)
        out["check"] = {"cer": res.cer.tolist(), "wer": res.wer.tolist()}
        return out
    al, hyps, refs = data(K)
    lab, ln, targets, target_lens = device_inputs(hyps, refs)
    sc = va.ErrorScorer(al)
    canon, kinds = sc.tables(lab.device)
    ref_labels, ref_lens = sc.references(targets, target_lens, lab.device)
    rows = torch.arange(B * K, dtype=torch.int32, device="cuda")
    pairs = torch.stack([rows, torch.div(rows, K, rounding_mode="floor")], dim=1)
    a, al_ = lab.reshape(B * K, -1), ln.reshape(-1)
    V = len(al)
    if name == "pairs":
        out["pairs"] = _windows(lambda: ops.edit_stats(a, al_, ref_labels, ref_lens, pairs, V, canon, None, ops.EDIT_CHARS), args.warmup,
                                args.repeats)
        conf = torch.zeros(V, V, dtype=torch.int32, device="cuda")
        out["pairs+trace"] = _windows(lambda: ops.edit_stats(a, al_, ref_labels, ref_lens, pairs, V, canon, None,
                                                             ops.EDIT_CHARS | ops.EDIT_TRACE, confusion=conf, ops=True), args.warmup, args.repeats)
        out["check"] = {"dist": ops.edit_stats(a, al_, ref_labels, ref_lens, pairs, V, canon, None, ops.EDIT_CHARS)[:, 0].cpu().tolist()}
        return out
    cl = canon.long()
    ac, bc = cl[a.long()], cl[ref_labels.long()][pairs[:, 1].long()]
    fn = lambda: torch_distances(ac, al_.long(), bc, ref_lens.long()[pairs[:, 1].long()])
    out["torch"] = _windows(fn, 1, max(args.repeats // 2, 3), window_ms=1.0)
    out["check"] = {"dist": fn().cpu().tolist()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per leg and round")
    ap.add_argument("--rounds", type=int, default=2, help="how often the legs alternate")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_score_bench.txt"))
    ap.add_argument("--leg", choices=LEGS, help="internal: time one leg in this process, print JSON")
    ap.add_argument("--cut", action="store_true", help="internal: the leg loads the A/B library")
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(leg(args.leg, args)), flush=True)
        return
    from __graft_entry__ import build
    build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pooled, checks = {}, {}
    ab, ab_same = {}, True
    for _ in range(args.rounds if os.path.exists(CUT) else 0):
        for dpp, g in AB:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "pairs", "--cut", "--repeats", str(args.repeats), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=900,
                               env=dict(os.environ, VOCR_ES_DPP=str(dpp), VOCR_ES_GTRACE_LDS=str(g)))
            got = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not got:
                say("the A/B leg %s failed (exit %d): %s" % ((dpp, g), r.returncode, r.stderr[-600:]))
                raise SystemExit(1)
            res = json.loads(got[0][len("LEG "):])
            for k in ("pairs", "pairs+trace"):
                ab.setdefault((dpp, g, k), []).extend(res[k])
            checks.setdefault("ab", res["check"])
            ab_same &= checks["ab"] == res["check"]
    for _ in range(args.rounds):
        for name in LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--repeats", str(args.repeats), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=900)
            got = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not got:
                say("the leg %s failed (exit %d): %s" % (name, r.returncode, r.stderr[-600:]))
                raise SystemExit(1)
            for k, v in json.loads(got[0][len("LEG "):]).items():
                if k == "check":
                    checks[name] = v
                else:
                    pooled.setdefault(k, []).extend(v)
    st = {k: _stats(v) for k, v in pooled.items()}
    say("device: %s" % torch.cuda.get_device_name(0))
    say("vocr_edit_stats / ErrorScorer on lines of %d .. %d random symbols of the English alphabet, hypotheses with 10 %% of the characters "
        "replaced.  Every leg in a child process of its own, the legs alternating %d times; a timed window is HIP events around n "
        "back-to-back calls (about 50 ms), ms per call = window / n; median / min / max over a leg's windows.  The CPU leg is "
        "perf_counter around whole batches on this box's CPU." % (LEN - 10, LEN + 10, args.rounds))
    row = "%-58s %10.3f %10.3f %10.3f"
    say("%-58s %10s %10s %10s" % ("ms per call", "median", "min", "max"))
    say("(a) one batch, %d lines, characters and words" % B)
    say(row % ("    ErrorScorer.score (ends with its device-to-host copy)", *st["score"]))
    say(row % ("    compute_cer_wer loop on the CPU (test_on_val's scoring)", *st["cpu"]))
    say(row % ("    eval forward of configs[1]'s model, 32 x 1x30x600", *st["forward"]))
    same_a = checks["score"] == checks["cpu"]
    say("    CPU loop / score: %.0fx; score / eval forward: %.3f; CER and WER of all %d lines %s the CPU loop's floats"
        % (st["cpu"][0] / st["score"][0], st["score"][0] / st["forward"][0], B, "EQUAL" if same_a else "DIFFER FROM"))
    say("(b) %d pairs (B = %d, K = %d), distances only, everything on the device" % (B * K, B, K))
    say(row % ("    ops.edit_stats, want = EDIT_CHARS", *st["pairs"]))
    say(row % ("    the anti-diagonal recursion in batched torch", *st["torch"]))
    same_b = checks["pairs"] == checks["torch"]
    say("    torch / kernel: %.0fx; %.1f ns per pair; the %d distances %s torch's" % (st["torch"][0] / st["pairs"][0],
                                                                                  st["pairs"][0] * 1e6 / (B * K), B * K,
                                                                                  "EQUAL" if same_b else "DIFFER FROM"))
    say("(c) the trace (operation counts, operations, confusion matrix) on against off")
    say(row % ("    ErrorScorer.score(trace=True), %d lines" % B, *st["score+trace"]))
    say(row % ("    ops.edit_stats, EDIT_CHARS | EDIT_TRACE, %d pairs" % (B * K), *st["pairs+trace"]))
    say("    on / off: %.2fx for the batch, %.2fx for the %d pairs" % (st["score+trace"][0] / st["score"][0],
                                                                      st["pairs+trace"][0] / st["pairs"][0], B * K))
    say("(d) lane packing of short pairs: not built, nothing to compare")
    if ab:
        say("(e) A/B library: the %d pairs with the lane shift as ds_bpermute / DPP wave_shr, and 256 / 2048 workgroups where the trace's "
            "table fits the LDS; distances %s the shipped library's" % (B * K, "EQUAL" if ab_same and checks["ab"] == checks["pairs"]
                                                                       else "DIFFER FROM"))
        for dpp, g in AB:
            what = "%s, %4d workgroups" % ("DPP wave_shr" if dpp else "ds_bpermute ", g)
            if g == AB[0][1]:
                say(row % ("    distances only, " + what.split(",")[0], *_stats(ab[(dpp, g, "pairs")])))
            say(row % ("    with the trace, " + what, *_stats(ab[(dpp, g, "pairs+trace")])))
        same_b = same_b and ab_same and checks["ab"] == checks["pairs"]
    else:
        say("(e) no A/B library at scripts/_cut/libvocr.so: the lane shift and the trace's grid were not compared")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if not (same_a and same_b and st["score"][0] < st["forward"][0]):
        raise SystemExit("REQUIRED: identical integers in (a) and (b), and a batch scored in less than its eval forward")


if __name__ == "__main__":
    main()
