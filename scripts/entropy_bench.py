"""Time the entropy-regularised CTC criterion and its kernel, vocr_ctc_entropy, on configs[1]'s logits shape (T = 294, B = 32, V = 96), on
peaky logits (labellings of 45-70 labels) and on the dense logits of the untrained configs[1] model (20 random labels per line):

  (a) vocr_ctc_entropy, the scores-only call (ln P and the alignment entropy; the forward paired sweep alone);
  (b) vocr_ctc_entropy with the gradient (both paired sweeps, the four lattices, the combine kernel);
  (c) EntropyRegularizedCTCLoss, forward and backward;
  (d) CTCLoss, forward and backward, in the same process on the same logits;
  (e) one train() step of configs[1]'s model (32 lines of 1 x 30 x 600) with each criterion.

Every leg group runs in a child process of its own under a time limit; a timed window is HIP events around enough back-to-back calls
for about 50 ms, ms per call = window / calls, median / min / max over the windows.  Output: profiles/r16_entropy_bench.txt.

    python scripts/entropy_bench.py [--repeats 7] [--out profiles/r16_entropy_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from risk_bench import B, T, V, _logits, _model, _windows  # noqa: E402  (the same logits and the same timing windows as r13)

BETA = 0.2
GROUPS = ("peaky", "dense", "step")


def group(kind, args):
    import vistaocr_amd as va
    from vistaocr_amd import ops
    out = {}
    act = torch.tensor([T] * B, dtype=torch.int32)
    if kind == "step":
        g = torch.Generator().manual_seed(5)
        L = 20
        batch = (torch.rand(B, 1, 30, 600, generator=g), torch.randint(1, V, (B * L,), generator=g).to(torch.int32),
                 torch.full((B,), 600, dtype=torch.int32), torch.full((B,), L, dtype=torch.int32), {})
        for name, crit in (("CTCLoss", va.CTCLoss()), ("EntropyRegularizedCTCLoss(%.1f)" % BETA, va.EntropyRegularizedCTCLoss(BETA))):
            model = _model()
            model.train()
            opt = va.make_optimizer(model, lr=1e-4)
            out["e train() step, " + name] = _windows(lambda: va.train(batch, model, crit, opt), args.warmup, args.repeats, 200.0)
        return out
    xd, targets, tl = _logits(kind)
    lens = [T] * B
    width = int(tl.max())
    rows = torch.zeros(B, width, dtype=torch.int32)
    o = 0
    for b in range(B):
        rows[b, :int(tl[b])] = targets[o:o + int(tl[b])]
        o += int(tl[b])
    labels, label_lens = rows.cuda(), tl.cuda()
    coeff = torch.tensor([[-1.0, -BETA]] * B, device="cuda")
    ctc, ent, _ = ops.ctc_entropy(xd, lens, labels, label_lens)
    tag = "(L %d-%d; mean nll %.1f, mean entropy %.2f nats)" % (int(tl.min()), width, float(-ctc.mean()), float(ent.mean()))
    out["a vocr_ctc_entropy, scores only %s" % tag] = _windows(lambda: ops.ctc_entropy(xd, lens, labels, label_lens), args.warmup, args.repeats)
    out["b vocr_ctc_entropy with the gradient"] = _windows(lambda: ops.ctc_entropy(xd, lens, labels, label_lens, None, coeff),
                                                          args.warmup, args.repeats)
    out["  vocr_ctc_nbest_grad with the gradient, n = 1 (the single sweep, for scale)"] = _windows(
        lambda: ops.ctc_nbest(xd, lens, labels, label_lens, None, coeff[:, 0].contiguous()), args.warmup, args.repeats)
    xg = xd.clone().requires_grad_(True)

    def fb(crit):
        xg.grad = None
        crit(xg, targets, act, tl).backward()
    ent_crit, ctc_crit = va.EntropyRegularizedCTCLoss(BETA), va.CTCLoss()
    out["c EntropyRegularizedCTCLoss(%.1f) forward + backward" % BETA] = _windows(lambda: fb(ent_crit), args.warmup, args.repeats)
    out["d CTCLoss forward + backward"] = _windows(lambda: fb(ctc_crit), args.warmup, args.repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_entropy_bench.txt"))
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
    say("entropy-regularised CTC on configs[1]'s logits shape, T=%d B=%d V=%d, beta = %.1f.  Every group of legs in a child process of its "
        "own; a timed window is HIP events around n back-to-back calls (about 50 ms; 200 ms for the train() step), ms per call = window / "
        "n; median / min / max over %d windows after %d warm-up calls." % (T, B, V, BETA, args.repeats, args.warmup))
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
            say(row % ("(%s) %s" % (k[0], k[2:]) if k[0] != " " else "    " + k[2:], *v))
        c = [v for k, v in res.items() if k.startswith("c ")]
        d = [v for k, v in res.items() if k.startswith("d ")]
        if c and d:
            say("    (c) / (d) = %.2fx" % (c[0][0] / d[0][0]))
        e = [v for k, v in res.items() if k.startswith("e ")]
        if len(e) == 2:
            say("    the step with the entropy criterion / the step with CTCLoss = %.3fx" % (e[1][0] / e[0][0]))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
