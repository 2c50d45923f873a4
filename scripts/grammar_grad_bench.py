"""Time grammar-constrained CTC training, vocr_ctc_grammar_grad and GrammarCTCLoss, on configs[1]'s logits shape (T = 294, B = 32, V = 96),
on peaky logits (labellings of 45-70 labels) and on the dense logits of the untrained configs[1] model (20 random labels per line):

  chains   every line against the chain of its own labelling (32 automata):
           (a) vocr_ctc_grammar_grad, scores only;  (b) with the gradient;  (c) GrammarCTCLoss.exact forward + backward;
           (d) CTCLoss forward + backward, in the same process on the same logits;
  one automaton for all lines, a gapped transcript (line 0's labelling with a hole before its last three labels) and a date regex:
           (f) vocr_ctc_grammar_grad, scores only;  (g) with the gradient;  (h) the same recursion in batched torch autograd (an edge
           list of the product graph, gather / scatter-amax / index_add per frame, forward + backward) - no symbol classes in (f)-(h);
  host     (i) what GrammarCTCLoss does on the host per batch - targets to automata, packing, one host-to-device copy - with a cold
           cache (every target new) and a warm one, for exact targets and for targets with a hole, wall clock;
  step     (e) one train() step of configs[1]'s model (32 lines of 1 x 30 x 600) with CTCLoss, GrammarCTCLoss.exact and with_gaps.

Every leg group runs in a child process of its own under a time limit; a timed window is HIP events around enough back-to-back calls
for about 50 ms, ms per call = window / calls, median / min / max over the windows.  Output: profiles/r17_grammar_grad_bench.txt.

    python scripts/grammar_grad_bench.py [--repeats 7] [--out profiles/r17_grammar_grad_bench.txt]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from risk_bench import B, T, V, _logits, _model, _windows  # noqa: E402  (the same logits and the same timing windows as r13, r16)

GROUPS = ("peaky", "dense", "host", "step")
DATE = r"\d\d/\d\d/\d\d\d\d"
NEG = float("-inf")


def _split(targets, tl):
    out, o = [], 0
    for n in tl.tolist():
        out.append([int(v) for v in targets[o:o + n]])
        o += n
    return out


class TorchRecursion(object):
    """The header's recursion over an explicit edge list of the product graph, all lines against ONE automaton, in torch."""

    def __init__(self, g, dev):
        S, E = g.n_states, g.n_arcs
        src, dst, cls = g.arc_src.tolist(), g.arc_dst.tolist(), g.arc_cls.tolist()
        tail, head = list(range(S + E)), list(range(S + E))
        out_of = {}
        for i in range(E):
            tail += [src[i], S + i]
            head += [S + i, dst[i]]
            out_of.setdefault(src[i], []).append(i)
        for i in range(E):
            for j in out_of.get(dst[i], ()):
                if cls[j] != cls[i]:
                    tail.append(S + i)
                    head.append(S + j)
        self.N, self.edges = S + E, len(tail)
        self.tail, self.head = torch.tensor(tail, device=dev), torch.tensor(head, device=dev)
        self.emit = torch.tensor([0] * S + cls, device=dev)
        self.first = torch.tensor([s == 0 for s in range(S)] + [s == 0 for s in src], device=dev)
        acc = g.accept.tolist()
        self.last = torch.tensor([bool(a) for a in acc] + [bool(acc[d]) for d in dst], device=dev)

    def __call__(self, x):
        lp = torch.log_softmax(x, 2)
        nb = x.shape[1]
        alpha = torch.where(self.first, lp[0][:, self.emit], torch.full((), NEG, device=x.device, dtype=x.dtype))
        head = self.head.unsqueeze(0).expand(nb, -1)
        for t in range(1, x.shape[0]):
            g = alpha[:, self.tail]
            m = torch.full((nb, self.N), NEG, device=x.device, dtype=x.dtype).scatter_reduce(1, head, g.detach(), "amax")
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            s = torch.zeros(nb, self.N, device=x.device, dtype=x.dtype).index_add(1, self.head, torch.exp(g - m[:, self.head]))
            dead = s <= 0                                          # a cell nothing reaches: -inf, and no 0 * inf in the backward pass
            alpha = lp[t][:, self.emit] + torch.where(dead, torch.full_like(s, NEG), m + torch.log(s.clamp_min(1e-30)))
        return torch.logsumexp(alpha[:, self.last], 1)


def group(kind, args):
    import vistaocr_amd as va
    from vistaocr_amd import Grammar, ops
    from vistaocr_amd.grammar import pack_grammars
    from vistaocr_amd.grammar_loss import pack_batch
    al = va.english_alphabet()
    out = {}
    act = torch.tensor([T] * B, dtype=torch.int32)
    star = al.char_to_idx["u002a"]
    if kind == "step":
        g = torch.Generator().manual_seed(5)
        L = 20
        targets = torch.randint(1, 60, (B, L), generator=g).to(torch.int32)
        holed = targets.clone()
        holed[:, 10:13] = star                                     # three labels of every line unread: one hole
        for name, crit, tg in (("CTCLoss", va.CTCLoss(), targets), ("GrammarCTCLoss.exact", va.GrammarCTCLoss.exact(al), targets),
                               ("GrammarCTCLoss.with_gaps, a hole in every target", va.GrammarCTCLoss.with_gaps(al, "*"), holed)):
            batch = (torch.rand(B, 1, 30, 600, generator=torch.Generator().manual_seed(6)), tg.reshape(-1),
                     torch.full((B,), 600, dtype=torch.int32), torch.full((B,), L, dtype=torch.int32), {})
            model = _model()
            model.train()
            opt = va.make_optimizer(model, lr=1e-4)
            out["e train() step, " + name] = _windows(lambda: va.train(batch, model, crit, opt), args.warmup, args.repeats, 200.0)
        return out
    if kind == "host":
        rng = np.random.default_rng(3)
        dev = torch.device("cuda")

        def batches(n, holes):
            res = []
            for _ in range(n):
                labs = [[int(v) for v in rng.integers(1, 60, int(rng.integers(45, 71)))] for _ in range(B)]
                if holes:
                    labs = [l[:len(l) // 2] + [star] + l[len(l) // 2 + 3:] for l in labs]
                res.append(([v for l in labs for v in l], [len(l) for l in labs]))
            return res

        def host(crit, flat, lens):
            grammars, which = crit.batch_grammars(flat, lens)
            pack_batch(grammars, which, [T] * B, dev)
            torch.cuda.synchronize()

        for name, make, holes in (("exact targets of 45-70 labels", lambda: va.GrammarCTCLoss.exact(al), False),
                                  ("targets of 45-70 labels with a hole in the middle", lambda: va.GrammarCTCLoss.with_gaps(al, "*"), True)):
            data = batches(args.repeats + 1, holes)
            crit = make()
            host(crit, *data[0])                                   # imports, the pinned buffer's first allocation
            cold, warm = [], []
            for flat, lens in data[1:]:
                t0 = time.perf_counter()
                host(crit, flat, lens)                             # 32 targets never seen
                cold.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                host(crit, flat, lens)                             # the same 32 again
                warm.append(1e3 * (time.perf_counter() - t0))
            g = crit.grammar_for(tuple(data[-1][0][:data[-1][1][0]]))
            tag = " (line 0: %d states + %d arcs)" % (g.n_states, g.n_arcs)
            out["i host, cold cache, %s%s" % (name, tag)] = [float(np.median(cold)), float(np.min(cold)), float(np.max(cold))]
            out["i host, warm cache, %s" % name] = [float(np.median(warm)), float(np.min(warm)), float(np.max(warm))]
        return out
    xd, targets, tl = _logits(kind)
    labs = _split(targets, tl)
    lens = [T] * B
    ones = torch.ones(B, device="cuda")
    # chains: 32 automata
    gp = pack_grammars([Grammar.from_labels(al, l) for l in labs], xd.device)
    which = torch.arange(B, dtype=torch.int32, device="cuda")
    logp = ops.ctc_grammar_grad(xd, lens, gp, which)[0]
    tag = "(L %d-%d; %d + %d cells at most; mean nll %.1f)" % (int(tl.min()), int(tl.max()), gp["max_states"], gp["max_arcs"], float(-logp.mean()))
    out["a chains: vocr_ctc_grammar_grad, scores only %s" % tag] = _windows(lambda: ops.ctc_grammar_grad(xd, lens, gp, which), args.warmup, args.repeats)
    out["b chains: vocr_ctc_grammar_grad with the gradient"] = _windows(lambda: ops.ctc_grammar_grad(xd, lens, gp, which, None, ones), args.warmup, args.repeats)
    xg = xd.clone().requires_grad_(True)

    def fb(crit):
        xg.grad = None
        crit(xg, targets, act, tl).backward()
    own, ctc = va.GrammarCTCLoss.exact(al), va.CTCLoss()
    out["c chains: GrammarCTCLoss.exact forward + backward (warm cache)"] = _windows(lambda: fb(own), args.warmup, args.repeats)
    out["d CTCLoss forward + backward"] = _windows(lambda: fb(ctc), args.warmup, args.repeats)
    # one automaton for all lines
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    l0 = labs[0]
    for name, g in (("gapped transcript", Grammar.from_template(al, l0[:-3] + [Grammar.GAP] + l0[-3:])), ("date regex", Grammar.from_regex(al, DATE))):
        gp1 = pack_grammars([g], xd.device)
        rec = TorchRecursion(g, xd.device)
        lp = ops.ctc_grammar_grad(xd, lens, gp1, zero)[0]
        with torch.no_grad():
            diff = float((rec(xd) - lp).abs().max())
        tag = "(%d states + %d arcs, %d product edges; mean -ln P %.1f; torch's ln P within %.1e)" % (g.n_states, g.n_arcs, rec.edges, float(-lp.mean()), diff)
        out["f %s: vocr_ctc_grammar_grad, scores only %s" % (name, tag)] = _windows(lambda: ops.ctc_grammar_grad(xd, lens, gp1, zero), args.warmup, args.repeats)
        out["g %s: vocr_ctc_grammar_grad with the gradient" % name] = _windows(lambda: ops.ctc_grammar_grad(xd, lens, gp1, zero, None, ones), args.warmup, args.repeats)

        def torch_fb():
            xg.grad = None
            rec(xg).sum().backward()
        out["h %s: the recursion in batched torch autograd, forward + backward" % name] = _windows(torch_fb, 1, min(args.repeats, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_grammar_grad_bench.txt"))
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
    say("grammar-constrained CTC training on configs[1]'s logits shape, T=%d B=%d V=%d.  Every group of legs in a child process of its own; a "
        "timed window is HIP events around n back-to-back calls (about 50 ms; 200 ms for the train() step), ms per call = window / n; "
        "median / min / max over %d windows after %d warm-up calls (the torch recursion: 3 windows after 1).  The host legs are wall "
        "clock per batch, device synchronised." % (T, B, V, args.repeats, args.warmup))
    row = "%-150s %9.3f %9.3f %9.3f"
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
             "host": "(i) the criterion's host work per batch of 32 targets, wall clock",
             "step": "(e) one train() step of configs[1]'s model, 32 lines of 1 x 30 x 600, 20 labels per line, FlatClampAdam"}[kind])
        say("%-150s %9s %9s %9s" % ("ms per call", "median", "min", "max"))
        for k, v in res.items():
            say(row % ("(%s) %s" % (k[0], k[2:]), *v))
        med = {k[0]: v[0] for k, v in res.items() if k[0] in "abcd"}
        if len(med) == 4:
            say("    chains: the kernel with the gradient (b) / CTCLoss (d) = %.2fx, the criterion (c) / (d) = %.2fx" % (med["b"] / med["d"], med["c"] / med["d"]))
        for name in ("gapped transcript", "date regex"):
            f = [v[0] for k, v in res.items() if k.startswith("f " + name)]
            g = [v[0] for k, v in res.items() if k.startswith("g " + name)]
            h = [v[0] for k, v in res.items() if k.startswith("h " + name)]
            if f and g and h:
                say("    %s: with the gradient (g) / scores only (f) = %.2fx; torch autograd (h) / (g) = %.1fx" % (name, g[0] / f[0], h[0] / g[0]))
        e = [v for k, v in res.items() if k.startswith("e ")]
        if len(e) == 3:
            say("    the step with GrammarCTCLoss.exact / the step with CTCLoss = %.3fx; with_gaps / CTCLoss = %.3fx" % (e[1][0] / e[0][0], e[2][0] / e[0][0]))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
