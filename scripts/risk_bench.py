"""Time the minimum-error-rate criterion and its kernel, vocr_ctc_nbest_grad, on configs[1]'s logits shape (T = 294, B = 32, V = 96) for
n = 4, 8 and 16 hypotheses per line, on peaky logits (labellings of 45-70 labels) and on the dense logits of the untrained configs[1]
model (whatever its search returns):

  (a) vocr_ctc_nbest_grad, both calls of the criterion (scores only, then scores and gradient), with the labels packed to the longest
      labelling and in the search's own layout (label_stride = T, what the criterion passes);
  (b) the composition it replaces: the logits repeated n times, vocr_ctc_loss_grad on B * n lines, the weighted reduction over n in
      torch (its flat labels are prepared outside the timed region; it has no classes, so it is fed the canonical labels and agrees
      with (a) only as far as no duplicate-string column carries weight: the largest difference is printed);
  (c) the whole criterion, forward and backward: search, error counts, scores, coefficients, gradient (ctc_weight = 0.01: CTCLoss inside);
  (d) CTCLoss, forward and backward;
  (e) one train() step of configs[1]'s model (32 lines of 1 x 30 x 600) with each criterion.

Every leg group runs in a child process of its own under a time limit; a timed window is HIP events around enough back-to-back calls
for about 50 ms, ms per call = window / calls, median / min / max over the windows.  Output: profiles/r13_risk_bench.txt.

    python scripts/risk_bench.py [--repeats 7] [--out profiles/r13_risk_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, B, V = 294, 32, 96
NS = (4, 8, 16)
HP = dict(num_in_channels=1, input_line_height=30, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3, num_lstm_hidden_units=512,
          p_lstm_dropout=0.5)
GROUPS = ("peaky", "dense", "step")


def _windows(fn, warmup, repeats, window_ms=50.0):
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
    return [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))]


def _model():
    import vistaocr_amd as va
    torch.manual_seed(0)
    return va.CnnOcrModel(alphabet=va.english_alphabet(), verbose=False, **HP)


def _logits(kind):
    """(logits [T,B,V] on the device, flat targets, target lens): peaky logits with a competitor on half of the frames and the greedy
    labelling with 10 % of the labels replaced as the reference; or the untrained model's logits with 20 random labels per line"""
    import vistaocr_amd as va
    from tests import align_ref as ar
    from tests import beam_data as bd
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    rng = np.random.default_rng(13)
    if kind == "peaky":
        x = bd.peaky_logits(rng, T, B, V, classes=cls, p_char=0.35)
        x[:, :, 0] = np.where(np.isinf(x[:, :, 0]), x.max(axis=2) - 12.0, x[:, :, 0])
        x = np.where(np.isinf(x), x.max(axis=2, keepdims=True) - 25.0, x).astype(np.float32)
        refs = []
        for b in range(B):
            lab = ar.greedy_labels(x[:, b], T)
            refs.append([int(cls[rng.integers(len(cls))]) if rng.random() < 0.1 else v for v in lab])
        xd = torch.from_numpy(x).cuda()
    else:
        model = _model().eval()
        with torch.no_grad():
            xd, _ = model(torch.rand(B, 1, 30, 600, generator=torch.Generator().manual_seed(1)).cuda(), torch.tensor([600] * B))
        xd = xd.detach().float().contiguous()
        assert tuple(xd.shape) == (T, B, V), tuple(xd.shape)
        refs = [[int(cls[i]) for i in rng.integers(0, len(cls), 20)] for _ in range(B)]
    return xd, torch.tensor([v for r in refs for v in r], dtype=torch.int32), torch.tensor([len(r) for r in refs], dtype=torch.int32)


def group(kind, args):
    import vistaocr_amd as va
    from vistaocr_amd import _lib, ops
    from vistaocr_amd import risk as rk
    al = va.english_alphabet()
    out = {}
    act = torch.tensor([T] * B, dtype=torch.int32)
    if kind == "step":
        g = torch.Generator().manual_seed(5)
        L = 20
        batch = (torch.rand(B, 1, 30, 600, generator=g), torch.randint(1, V, (B * L,), generator=g).to(torch.int32),
                 torch.full((B,), 600, dtype=torch.int32), torch.full((B,), L, dtype=torch.int32), {})
        for name, crit in [("CTCLoss", va.CTCLoss())] + [("MinErrorRateLoss n=%d" % n, va.MinErrorRateLoss(al, nbest=n)) for n in NS]:
            model = _model()
            model.train()
            opt = va.make_optimizer(model, lr=1e-4)
            out["e train() step, " + name] = _windows(lambda: va.train(batch, model, crit, opt), args.warmup, args.repeats, 200.0)
        return out
    xd, targets, tl = _logits(kind)
    lens = [T] * B
    xg = xd.clone().requires_grad_(True)

    def fb(crit):
        xg.grad = None
        crit(xg, targets, act, tl).backward()
    out["d CTCLoss forward + backward"] = _windows(lambda: fb(va.CTCLoss()), args.warmup, args.repeats)
    for n in NS:
        crit = va.MinErrorRateLoss(al, nbest=n)
        labels, lengths, errors, ctc, member, canon = rk.nbest_list(xd, targets, act, tl, crit.decoder, crit.scorer, n)
        _, c, _ = rk.risk_terms(errors, ctc, member)
        hn = lengths.cpu().numpy()
        hi = max(int(hn.max()), 1)
        packed = labels[:, :, :hi].contiguous()
        tag = "n=%2d (L %d-%d, %d of %d ranks in the lists)" % (n, int(hn[hn >= 0].min()), hi, int(member.sum()), B * n)

        def both(lab):
            ops.ctc_nbest(xd, lens, lab, lengths, canon)
            return ops.ctc_nbest(xd, lens, lab, lengths, canon, c)[1]
        out["a %s vocr_ctc_nbest_grad x 2, packed" % tag] = _windows(lambda: both(packed), args.warmup, args.repeats)
        out["a %s vocr_ctc_nbest_grad x 2, label_stride = T" % tag] = _windows(lambda: both(labels), args.warmup, args.repeats)
        out["a %s   of which the scores-only call, packed" % tag] = _windows(lambda: ops.ctc_nbest(xd, lens, packed, lengths, canon),
                                                                             args.warmup, args.repeats)
        # (b): B * n lines for vocr_ctc_loss_grad
        hl = labels.cpu().numpy()
        ll = np.maximum(hn.reshape(-1), 0).astype(np.int32)
        flat = np.concatenate([hl.reshape(B * n, -1)[i, :ll[i]] for i in range(B * n)] + [np.zeros(1, np.int32)]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int32)
        fd, od, ld = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ll).cuda()
        ad = torch.full((B * n,), T, dtype=torch.int32, device="cuda")
        lib = _lib.load()
        mx = int(ll.max())
        p = ops._p
        neg = (-c).view(1, B, n, 1)

        def composed():
            rep = xd.repeat_interleave(n, dim=1)
            ws = ops._ws(lib.vocr_ctc_workspace_bytes(T, B * n, V, mx), xd.device)
            nll = torch.empty(B * n, 1, dtype=torch.float32, device=xd.device)
            dl = torch.empty_like(rep)
            _lib.call("vocr_ctc_loss_grad", p(rep), p(fd), p(od), p(ld), p(ad), p(nll), p(dl), p(ws), T, B * n, V, mx, ops._stream())
            return (dl.view(T, B, n, V) * neg).sum(2)
        out["b %s logits x n, vocr_ctc_loss_grad on B * n lines, reduction" % tag] = _windows(composed, args.warmup, args.repeats)
        diff = float((both(packed) - composed()).abs().max()) if bool(member.all()) else float("nan")
        out["check %s" % tag] = [diff, float(both(packed).abs().max()), 0.0]
        out["c %s MinErrorRateLoss forward + backward" % tag] = _windows(lambda: fb(crit), args.warmup, args.repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_risk_bench.txt"))
    ap.add_argument("--group", choices=GROUPS, help="internal: time one group of legs in this process, print JSON")
    args = ap.parse_args()
    if args.group:
        print("LEG " + json.dumps(group(args.group, args)), flush=True)
        return
    from __graft_entry__ import build
    build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("minimum-error-rate criterion on configs[1]'s logits shape, T=%d B=%d V=%d.  Every group of legs in a child process of its own; a "
        "timed window is HIP events around n back-to-back calls (about 50 ms; 200 ms for the train() step), ms per call = window / n; "
        "median / min / max over %d windows after %d warm-up calls." % (T, B, V, args.repeats, args.warmup))
    row = "%-100s %9.3f %9.3f %9.3f"
    for kind in GROUPS:
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--group", kind, "--repeats",
                            str(args.repeats), "--warmup", str(args.warmup)], capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
        if r.returncode != 0 or not got:
            say("the group %s failed (exit %d): %s" % (kind, r.returncode, r.stderr[-800:]))
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            raise SystemExit(1)
        res = json.loads(got[0][len("LEG "):])
        say("")
        say({"peaky": "peaky logits (one dominant class per frame, a competitor on half of the frames)",
             "dense": "dense logits: the untrained configs[1] model on 32 random 1 x 30 x 600 images",
             "step": "(e) one train() step of configs[1]'s model, 32 lines of 1 x 30 x 600, FlatClampAdam"}[kind])
        say("%-100s %9s %9s %9s" % ("ms per call", "median", "min", "max"))
        for k, v in res.items():
            if k.startswith("check"):
                say("    %s: largest |(a) - (b)| over the gradient %.3g (largest |gradient| %.3g)" % (k, v[0], v[1]))
            else:
                say(row % ("(%s) %s" % (k[0], k[2:]), *v))
        for n in NS:
            a = [v for k, v in res.items() if k.startswith("a n=%2d" % n) and k.endswith("x 2, packed")]
            b = [v for k, v in res.items() if k.startswith("b n=%2d" % n)]
            if a and b:
                say("    n=%2d: (b) / (a) = %.2fx" % (n, b[0][0] / a[0][0]))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
