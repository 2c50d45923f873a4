"""Time vocr_ctc_edit_scores on configs[1]'s logits shape (T = 294, B = 32, V = 96) with the 1-best of a K = 16 beam search at short
(S <= 64: one wave per lattice) and long (the LDS-row path) label lengths; in the same run, for scale, vocr_ctc_align on the same
input, the search itself, and the NAIVE route to the same numbers: every edited labelling scored by vocr_ctc_align, 128 labellings
per call.  The naive route is timed on a fixed subset - three calls of n = 128, holding for every line the first 128 edits (the
substitutions by every other class, the deletion, the insertions of every class) at the first, the middle and the last position - and
scaled to the number of calls the longest line needs, ceil((L * 2 C + C) / 128) with C classes; its scores are compared with the new
call's.  HIP events, warm-up, median / min / max of the repeats.  Output: profiles/r10_edit_bench.txt.

    python scripts/edit_bench.py [--repeats 20] [--out profiles/r10_edit_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vistaocr_amd as va                                    # noqa: E402
from vistaocr_amd import ops                                 # noqa: E402
from tests import beam_data as bd                            # noqa: E402

T, B, V = 294, 32, 96
N = 128


def _time(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def edits_at(labels, p, classes, canon):
    """(kind, column, labelling) of every edit at position p: substitutions by every other class, the deletion, insertions before p."""
    out = [("sub", c, labels[:p] + [c] + labels[p + 1:]) for c in classes if c != canon[labels[p]]]
    out.append(("del", 0, labels[:p] + labels[p + 1:]))
    out += [("ins", c, labels[:p] + [c] + labels[p:]) for c in classes]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_edit_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    cls = [int(c) for c in np.nonzero(canon == np.arange(V))[0][1:]]
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    lens = [T] * B
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("vocr_ctc_edit_scores, T=%d B=%d V=%d (%d classes), the 1-best of ctc_beam_search(K = 16) on peaky logits; median of %d after %d "
        "warm-up (ms per batch, all kernels of a call)" % (T, B, V, len(cls), args.repeats, args.warmup))
    fmt = "%-76s %8s %8s %8s"
    say(fmt % ("leg", "median", "min", "max"))

    def leg(name, fn):
        r = _time(fn, args.warmup, args.repeats)
        say(fmt % ((name,) + tuple("%.3f" % v for v in r)))
        return r[0]

    summary = []
    for p_char, tag in ((0.10, "short"), (0.35, "long")):
        xs = bd.peaky_logits(np.random.default_rng(7), T, B, V, classes=cls, p_char=p_char)
        xd = torch.from_numpy(xs).cuda()
        lab, ln, _ = ops.ctc_beam_search(xd, lens, cd, 16, 1)
        hl, hn = lab.cpu().numpy(), ln.cpu().numpy()
        labels = [[int(v) for v in hl[b, 0, :hn[b, 0]]] for b in range(B)]
        lo, hi = min(map(len, labels)), max(map(len, labels))
        say("%s labellings (p_char %.2f, L %d-%d)" % (tag, p_char, lo, hi))
        search = leg("  the K = 16 search (nbest = 1)", lambda: ops.ctc_beam_search(xd, lens, cd, 16, 1))
        packed = lab[:, :, :hi].contiguous()
        edit = leg("  vocr_ctc_edit_scores, packed (label_stride = %d)" % hi, lambda: ops.ctc_edit_scores(xd, lens, packed, ln, cd))
        leg("  vocr_ctc_edit_scores, label_stride = T (the search's layout)", lambda: ops.ctc_edit_scores(xd, lens, lab, ln, cd))
        align = leg("  vocr_ctc_align, packed", lambda: ops.ctc_align(xd, lens, packed, ln, cd))
        aligner = va.CtcAligner(al)
        leg("  CtcAligner.alternatives(topk=3): reduction, copy and host formatting included", lambda: aligner.alternatives(xd, lens, labels))
        dec = va.BeamDecoder(al, beam=16)
        leg("  BeamDecoder(beam=16).decode_alternatives, host formatting included", lambda: dec.decode_alternatives(xd, lens))
        leg("  BeamDecoder(beam=16).decode, host formatting included", lambda: dec.decode(xd, lens))
        # the naive route: three calls of 128 edited labellings per line
        ctc, sub, dele, ins = [t.cpu().numpy() for t in ops.ctc_edit_scores(xd, lens, packed, ln, cd)]
        naive, worst = [], 0.0
        for which in ("first", "middle", "last"):
            nl = np.zeros((B, N, hi + 1), dtype=np.int32)
            nn = np.zeros((B, N), dtype=np.int32)
            kept = []
            for b in range(B):
                p = {"first": 0, "middle": len(labels[b]) // 2, "last": len(labels[b]) - 1}[which]
                e = edits_at(labels[b], p, cls, canon)[:N]
                kept.append((p, e))
                for q, (_, _, l) in enumerate(e):
                    nl[b, q, :len(l)] = l
                    nn[b, q] = len(l)
            nld, nnd = torch.from_numpy(nl).cuda(), torch.from_numpy(nn).cuda()
            naive.append(leg("  naive: vocr_ctc_align, n = 128 edits at the %s position of every line" % which,
                             lambda: ops.ctc_align(xd, lens, nld, nnd, cd)))
            sc = ops.ctc_align(xd, lens, nld, nnd, cd)[0].cpu().numpy()
            for b, (p, e) in enumerate(kept):
                for q, (kind, c, _) in enumerate(e):
                    mine = {"sub": sub[b, 0, p, c], "del": dele[b, 0, p], "ins": ins[b, 0, p, c]}[kind]
                    if np.isfinite(mine) or np.isfinite(sc[b, q, 1]):
                        worst = max(worst, abs(float(mine) - float(sc[b, q, 1])))
        calls = -(-(hi * 2 * len(cls) + len(cls)) // N)
        total = float(np.mean(naive)) * calls
        say("  naive route, scaled: %d calls for the longest line (L = %d: %d edits) x %.3f ms = %.1f ms; largest |naive - new| over the "
            "%d timed edits per line %.3g" % (calls, hi, hi * 2 * len(cls) + len(cls), float(np.mean(naive)), total, 3 * N, worst))
        summary.append("%s (L %d-%d): the new call %.3f ms = %.2fx the alignment (%.3f ms) = %.2fx the search (%.3f ms); the naive route "
                       "%.1f ms = %.0fx the new call" % (tag, lo, hi, edit, edit / align, align, edit / search, search, total, total / edit))
    say("")
    for s in summary:
        say(s)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
