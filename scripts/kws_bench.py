"""Time vocr_ctc_keyword_scores on configs[1]'s logits shape (T = 294, B = 32, V = 96), peaky and dense inputs of tests/beam_data.py,
Q = 100 / 1000 / 10000 queries of 3 .. 12 labels (half of them substrings of the lines' greedy labellings).  Device time per call and
per (line, query) of the shipped library; the same with lane packing on and off (off: every query a wave of its own), both with the A/B
library of `python -m vistaocr_amd.build --experiments` (scripts/_cut/libvocr.so, VOCR_KWS_PACK=1 / 0; skipped, and said so, when that
library is not there), so that only the switch differs; and, for scale, a straightforward torch implementation of the same recursion on
the same GPU: vectorised over (B, Q, S), a Python loop over T.  That implementation lives here, not in the product; its counts are
compared with the kernel's.  Every leg runs in a child process of its own and the legs alternate; a timed window is HIP events around
enough back-to-back calls for about 50 ms, with every argument on the device already.  Output: profiles/r11_kws_bench.txt.

    python scripts/kws_bench.py [--repeats 10] [--rounds 2] [--out profiles/r11_kws_bench.txt]"""
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
QS = (100, 1000, 10000)
NEG = float("-inf")


def _windows(fn, warmup, repeats, window_ms=50.0):
    """`repeats` timed windows of HIP events around n back-to-back calls of fn (n chosen so that a window lasts about window_ms: a
    window of one sub-millisecond call would measure the clock and the scheduler); ms per call of every window."""
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


def inputs(kind):
    from tests import beam_data as bd
    rng = np.random.default_rng(7)
    return bd.peaky_logits(rng, T, B, V, p_char=0.35) if kind == "peaky" else bd.dense_logits(rng, T, B, V)


def queries(x, Q, seed=8):
    """int32 [Q, 12] labels and [Q] lengths 3 .. 12: even entries substrings of a line's argmax collapse, odd ones random."""
    rng = np.random.default_rng(seed)
    greedy = []
    for b in range(B):
        idx = np.argmax(x[:, b], axis=1)
        keep = (idx != 0) & (idx != np.concatenate([[0], idx[:-1]]))
        greedy.append(idx[keep])
    lab = np.zeros((Q, 12), dtype=np.int32)
    ln = rng.integers(3, 13, Q).astype(np.int32)
    for q in range(Q):
        g = greedy[q % B]
        if q % 2 == 0 and len(g) >= ln[q]:
            o = int(rng.integers(0, len(g) - ln[q] + 1))
            lab[q, :ln[q]] = g[o:o + ln[q]]
        else:
            lab[q, :ln[q]] = rng.integers(1, V, ln[q])
    return lab, ln


def torch_frame_terms(x):
    """(lp [T,B,V] log-softmax, notc [T,B,V] = ln of the other columns' summed probability): one masked logsumexp per column."""
    lp = torch.log_softmax(x, dim=2)
    notc = torch.empty_like(lp)
    for c in range(V):
        keep = torch.ones(V, dtype=torch.bool, device=x.device)
        keep[c] = False
        notc[:, :, c] = torch.logsumexp(lp[:, :, keep], dim=2)
    return lp, notc


def torch_search(lp, notc, lab, ln):
    """The recursion of include/vocr.h on [B, Q, S] tensors, no anchors, no classes: (log_count, best) [B, Q]."""
    dev = lp.device
    Q, L = lab.shape
    S = 2 * L - 1
    pos = torch.arange(S, device=dev)
    ext = torch.zeros(Q, S, dtype=torch.long, device=dev)
    ext[:, 0::2] = lab.long()
    inside = pos[None, :] < (2 * ln.long() - 1)[:, None]
    skip = torch.zeros(Q, S, dtype=torch.bool, device=dev)
    skip[:, 2::2] = lab[:, 1:] != lab[:, :-1]
    last = (2 * ln.long() - 2)[None, :, None].expand(B, Q, 1)
    k1, kL = lab[:, 0].long(), lab.long().gather(1, (ln.long() - 1)[:, None])[:, 0]
    a = torch.full((B, Q, S), NEG, device=dev)
    m = torch.full((B, Q, S), NEG, device=dev)
    acc = torch.full((B, Q), NEG, device=dev)
    best = torch.full((B, Q), NEG, device=dev)
    pad2 = torch.full((B, Q, 2), NEG, device=dev)
    zero = torch.zeros(B, Q, device=dev)
    for t in range(T):
        lpe = lp[t][:, ext]
        en = zero if t == 0 else notc[t - 1][:, k1]
        ex = zero if t == T - 1 else notc[t + 1][:, kL]
        a1 = torch.cat([en[:, :, None], a[:, :, :-1]], dim=2)
        a2 = torch.cat([pad2, a[:, :, :-2]], dim=2).masked_fill(~skip[None], NEG)
        m1 = torch.cat([en[:, :, None], m[:, :, :-1]], dim=2)
        m2 = torch.cat([pad2, m[:, :, :-2]], dim=2).masked_fill(~skip[None], NEG)
        a = (torch.logsumexp(torch.stack([a, a1, a2]), dim=0) + lpe).masked_fill(~inside[None], NEG)
        m = (torch.maximum(torch.maximum(m, m1), m2) + lpe).masked_fill(~inside[None], NEG)
        acc = torch.logaddexp(acc, a.gather(2, last)[:, :, 0] + ex)
        best = torch.maximum(best, m.gather(2, last)[:, :, 0] + ex)
    return acc, best


LEGS = {"shipped": (None, None), "ab-packed": ("_cut", "1"), "ab-unpacked": ("_cut", "0")}     # (library directory under scripts/, VOCR_KWS_PACK)


def kernel_leg(args):
    """ms per call of ops.ctc_keyword_scores for every (input, Q) as {"peaky/100": [every window], ..}.  Logits, lens, queries and
    query lengths are on the device before the clock starts: a call is the wrapper's checks, its three output allocations and the five
    launches, with no host-to-device copy."""
    from vistaocr_amd import ops
    out = {}
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    for kind in ("peaky", "dense"):
        x = inputs(kind)
        xd = torch.from_numpy(x).cuda()
        for Q in QS:
            lab, ln = queries(x, Q)
            labd, lnd = torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda()
            out["%s/%d" % (kind, Q)] = _windows(lambda: ops.ctc_keyword_scores(xd, lens, labd, lnd), args.warmup, args.repeats)
    return out


def run_legs(args, names, say):
    """Every leg of `names` in a child process of its own (a process loads one library), the legs alternating `args.rounds` times so
    that a drift of the machine falls on all of them alike; the windows of a leg's rounds are pooled."""
    pooled = {n: {} for n in names}
    for _ in range(args.rounds):
        for name in names:
            pack = LEGS[name][1]
            env = dict(os.environ) if pack is None else dict(os.environ, VOCR_KWS_PACK=pack)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--repeats", str(args.repeats), "--warmup",
                                str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
            got = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not got:
                say("the leg %s failed (exit %d): %s" % (name, r.returncode, r.stderr[-400:]))
                return None
            for k, v in json.loads(got[0][len("LEG "):]).items():
                pooled[name].setdefault(k, []).extend(v)
    return {n: {k: _stats(v) for k, v in d.items()} for n, d in pooled.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per leg and round")
    ap.add_argument("--rounds", type=int, default=2, help="how often the legs alternate")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_kws_bench.txt"))
    ap.add_argument("--leg", choices=sorted(LEGS), help="internal: time one leg in this process, print JSON")
    args = ap.parse_args()
    if args.leg:
        if LEGS[args.leg][0]:
            import vistaocr_amd._lib as L
            L.LIB_PATH = os.path.join(ROOT, "scripts", LEGS[args.leg][0], "libvocr.so")
        print("LEG " + json.dumps(kernel_leg(args)), flush=True)
        return
    from __graft_entry__ import build
    build()
    from vistaocr_amd import ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("vocr_ctc_keyword_scores, T=%d B=%d V=%d, queries of 3 .. 12 labels (S = 5 .. 23: all in the 16- and 32-lane layouts)" % (T, B, V))
    say("a timed window: HIP events around n back-to-back calls of ops.ctc_keyword_scores, n chosen for a window of about 50 ms, ms per "
        "call = window / n.  Logits, lens, queries and query lengths are device tensors, so a call is the wrapper's checks, its three "
        "output allocations (caching allocator) and the five kernel launches; no host-to-device copy, no synchronise inside a window.")
    say("every leg runs in a child process of its own; the legs alternate %d times, %d windows each time after %d warm-up calls per "
        "shape; median / min / max over a leg's %d windows" % (args.rounds, args.repeats, args.warmup, args.rounds * args.repeats))
    names = ["shipped"]
    if os.path.exists(os.path.join(ROOT, "scripts", "_cut", "libvocr.so")):
        names += ["ab-packed", "ab-unpacked"]
    else:
        say("no A/B library at scripts/_cut/libvocr.so: the legs with and without lane packing were not run")
    legs = run_legs(args, names, say)
    if legs is None:
        raise SystemExit(1)
    packed = legs["shipped"]
    abp, abu = legs.get("ab-packed"), legs.get("ab-unpacked")
    fmt = "%-6s %6s | %8s %8s %8s %9s | %9s %9s %9s %6s | %11s %10s %6s %9s"
    say(fmt % ("input", "Q", "median", "min", "max", "ns/(b,q)", "A/B pack", "A/B unp.", "ns/(b,q)", "ratio", "torch terms", "torch loop", "ratio",
               "|diff|"))
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    for kind in ("peaky", "dense"):
        x = inputs(kind)
        xd = torch.from_numpy(x).cuda()
        terms = _stats(_windows(lambda: torch_frame_terms(xd), 2, 5))[0]
        lp, notc = torch_frame_terms(xd)
        for Q in QS:
            lab, ln = queries(x, Q)
            labd, lnd = torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda()
            med, lo, hi = packed["%s/%d" % (kind, Q)]
            loop = _stats(_windows(lambda: torch_search(lp, notc, labd, lnd), 2, 5))[0]
            mine = ops.ctc_keyword_scores(xd, lens, labd, lnd)
            ref = torch_search(lp, notc, labd, lnd)
            fin = torch.isfinite(ref[0]) & torch.isfinite(mine[0])
            same_inf = bool((torch.isfinite(ref[0]) == torch.isfinite(mine[0])).all())
            diff = float((ref[0][fin] - mine[0][fin]).abs().max()) if bool(fin.any()) else 0.0
            pk = abp["%s/%d" % (kind, Q)][0] if abp else None
            un = abu["%s/%d" % (kind, Q)][0] if abu else None
            say(fmt % (kind, Q, "%.3f" % med, "%.3f" % lo, "%.3f" % hi, "%.1f" % (med * 1e6 / (B * Q)),
                       "%.3f" % pk if pk else "-", "%.3f" % un if un else "-", "%.1f" % (un * 1e6 / (B * Q)) if un else "-",
                       "%.2fx" % (un / pk) if un else "-",
                       "%.2f" % terms, "%.1f" % loop, "%.0fx" % ((terms + loop) / med), "%.2g%s" % (diff, "" if same_inf else " inf!")))
    say("")
    say("median / min / max / ns/(b,q): the shipped library.  A/B pack, A/B unp.: the median of the same call with the A/B library "
        "(python -m vistaocr_amd.build --experiments) and VOCR_KWS_PACK=1 / 0, that is with short queries sharing a wave as shipped / "
        "with every query a wave of its own; ns/(b,q) of the latter; ratio: unpacked / packed, both of the A/B library.")
    say("torch terms: log-softmax and the not-class rows in torch (per call, independent of Q); torch loop: the recursion, count and best "
        "score without spans (both: the median of 5 windows after 2 warm-up calls, in this process); ratio: (terms + loop) / the shipped "
        "library's call; |diff|: the largest difference of the two log counts.")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
