"""Time vocr_ctc_align on configs[1]'s logits shape (T = 294, B = 32, V = 96): short labellings (one wave per labelling, S <= 64), long
labellings (the LDS-row path), the 1-best and 4-best of a K = 16 beam search handed over on the device, and a 60-label transcript on
dense logits; in the same run, for scale, the K = 16 search that produced the labels, the eval forward of that batch (configs[1]'s
model, 32 lines of 1x30x600) and, once, the fp64 CPU restatement of tests/align_ref.py.  HIP events, warm-up, median / min / max of
the repeats.  Output: profiles/r09_align_bench.txt.

    python scripts/align_bench.py [--repeats 20] [--out profiles/r09_align_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vistaocr_amd as va                                    # noqa: E402
from vistaocr_amd import ops                                 # noqa: E402
from tests import align_ref as ar                            # noqa: E402
from tests import beam_data as bd                            # noqa: E402

T, B, V = 294, 32, 96


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


def _pack(labels, width=None):
    width = max(len(l) for l in labels) if width is None else width
    lab = np.zeros((len(labels), 1, width), dtype=np.int32)
    for b, l in enumerate(labels):
        lab[b, 0, :len(l)] = l
    return torch.from_numpy(lab).cuda(), torch.tensor([[len(l)] for l in labels], dtype=torch.int32).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_align_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    lens = [T] * B
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    hp = dict(num_in_channels=1, input_line_height=30, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3,
              num_lstm_hidden_units=512, p_lstm_dropout=0.5)
    torch.manual_seed(0)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp).cuda().eval()
    x = torch.rand(B, 1, 30, 600, device="cuda")
    widths = torch.tensor([600] * B)
    with torch.no_grad():
        out, _ = model(x, widths)
        fwd = _time(lambda: model(x, widths), args.warmup, args.repeats)
    assert tuple(out.shape) == (T, B, V), tuple(out.shape)
    say("device: %s" % torch.cuda.get_device_name(0))
    say("eval forward, configs[1] batch (32 x 1x30x600 -> logits %s): median %.3f ms (min %.3f, max %.3f)" % ((tuple(out.shape),) + fwd))
    say("")
    say("vocr_ctc_align, T=%d B=%d V=%d; median of %d after %d warm-up (ms per batch, both kernels of the call)" % (T, B, V, args.repeats, args.warmup))
    fmt = "%-62s %8s %8s %8s"
    say(fmt % ("leg", "median", "min", "max"))

    def leg(name, logits, lab, ln):
        r = _time(lambda: ops.ctc_align(logits, lens, lab, ln, cd), args.warmup, args.repeats)
        say(fmt % ((name,) + tuple("%.3f" % v for v in r)))
        return r

    host = {}
    for p_char, tag in ((0.10, "short"), (0.35, "long")):
        xs = bd.peaky_logits(np.random.default_rng(7), T, B, V, classes=cls, p_char=p_char)
        labels = [ar.greedy_labels(xs[:, b], T) for b in range(B)]
        host[tag] = (xs, labels)
        lab, ln = _pack(labels)
        leg("%s labellings (p_char %.2f, L %d-%d), n = 1, packed" % (tag, p_char, min(map(len, labels)), max(map(len, labels))),
            torch.from_numpy(xs).cuda(), lab, ln)
        lab, ln = _pack(labels, T)
        leg("  the same, label_stride = T (the beam searches' layout)", torch.from_numpy(xs).cuda(), lab, ln)

    # the K = 16 search and the alignment of what it found, handed over on the device
    xs = host["long"][0]
    xd = torch.from_numpy(xs).cuda()
    results = {}
    for n in (1, 4):
        s = _time(lambda: ops.ctc_beam_search(xd, lens, cd, 16, n), args.warmup, args.repeats)
        lab, ln, _ = ops.ctc_beam_search(xd, lens, cd, 16, n)
        a = leg("n = %d from ctc_beam_search(K = 16), peaky p_char 0.35" % n, xd, lab, ln)
        say(fmt % (("  the K = 16 search that produced them (nbest = %d)" % n,) + tuple("%.3f" % v for v in s)))
        results[n] = (a[0], s[0])
    dec = va.BeamDecoder(al, beam=16)
    r = _time(lambda: dec.decode_aligned(xd, lens), args.warmup, args.repeats)
    say(fmt % (("BeamDecoder(beam=16).decode_aligned, host formatting included",) + tuple("%.3f" % v for v in r)))
    r = _time(lambda: dec.decode(xd, lens), args.warmup, args.repeats)
    say(fmt % (("BeamDecoder(beam=16).decode, host formatting included",) + tuple("%.3f" % v for v in r)))

    dense = np.random.default_rng(7).normal(0, 1, (T, B, V)).astype(np.float32)
    dl = [ar.greedy_labels(dense[:, b], T)[:60] for b in range(B)]
    lab, ln = _pack(dl)
    leg("dense N(0,1) logits, 60-label transcript, n = 1, packed", torch.from_numpy(dense).cuda(), lab, ln)
    say("")
    a1, s1 = results[1]
    say("aligning the 1-best costs %.3f ms, the K = 16 search that found it %.3f ms: %.2fx the search (%s)"
        % (a1, s1, a1 / s1, "less, as expected" if a1 < s1 else "NOT less than the search"))
    t0 = time.time()
    for b in range(B):
        ar.align(xs[:, b], T, host["long"][1][b], canon)
    say("CPU restatement (fp64 numpy, one thread), long labellings: %.2f s per batch" % (time.time() - t0))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
