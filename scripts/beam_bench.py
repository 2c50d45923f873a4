"""Time vocr_ctc_beam_search on configs[1]'s logits shape (T = 294, B = 32, V = 96) for K in {1, 4, 16, 64}, without an LM and with a
synthetic character 6-gram, against the eval forward of that batch (configs[1]'s model, 32 lines of 1x30x600) and, once, the fp64 CPU
restatement of tests/beam_ref.py.  HIP events, warm-up, median of repeats.  Output: profiles/r07_beam_bench.txt.

    python scripts/beam_bench.py [--repeats 20] [--out profiles/r07_beam_bench.txt]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vistaocr_amd as va                                    # noqa: E402
from vistaocr_amd import ops                                 # noqa: E402
from tests import beam_data as bd                            # noqa: E402
from tests import beam_ref as br                             # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_beam_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the eval forward of configs[1]'s batch (the logits the decoder consumes)
    hp = dict(num_in_channels=1, input_line_height=30, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3,
              num_lstm_hidden_units=512, p_lstm_dropout=0.5)
    torch.manual_seed(0)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp).cuda().eval()
    x = torch.rand(B, 1, 30, 600, device="cuda")
    widths = torch.tensor([600] * B)
    with torch.no_grad():
        out, lens = model(x, widths)
        fwd = _time(lambda: model(x, widths), args.warmup, args.repeats)
    assert tuple(out.shape) == (T, B, V), tuple(out.shape)
    say("device: %s" % torch.cuda.get_device_name(0))
    say("eval forward, configs[1] batch (32 x 1x30x600 -> logits %s): median %.3f ms (min %.3f, max %.3f)" % ((tuple(out.shape),) + fwd))

    # decode inputs: peaky synthetic logits of the same shape, and a character 6-gram over 39 symbols written from random text
    logits = torch.from_numpy(bd.peaky_logits(np.random.default_rng(7), T, B, V, classes=cls)).cuda()
    logits_model = out.detach().float().contiguous()
    tmp = tempfile.mkdtemp()
    path = bd.write_char_arpa(os.path.join(tmp, "char6.arpa"), [al.idx_to_char[c] for c in range(1, 40)], order=6, lines=600, seed=1)
    t0 = time.time()
    lm = va.CharNgramLM.from_arpa(path, al)
    say("LM: character 6-gram, %d states (tables %.1f MiB), resolved in %.2f s on the host"
        % (lm.num_states, lm.num_states * V * 8 / 2.0 ** 20, time.time() - t0))
    lmd = lm.to("cuda")
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    lens_l = [T] * B
    say("")
    say("vocr_ctc_beam_search, T=%d B=%d V=%d, nbest=1, no pruning; median of %d after %d warm-up (ms per batch)" % (T, B, V, args.repeats, args.warmup))
    say("%-4s %-10s %-16s %10s %10s %10s %12s" % ("K", "LM", "logits", "median", "min", "max", "vs forward"))
    for K in (1, 4, 16, 64):
        for name, lmx, a, bb in (("none", None, 0.0, 0.0), ("6-gram", lmd, 0.8, 1.0)):
            for lname, lg in (("peaky synth", logits), ("model (rand)", logits_model)):
                r = _time(lambda: ops.ctc_beam_search(lg, lens_l, cd, K, 1, lmx, a, bb), args.warmup, args.repeats)
                say("%-4d %-10s %-16s %10.3f %10.3f %10.3f %11.2fx" % ((K, name, lname) + r + (r[0] / fwd[0],)))
    # the fp64 CPU restatement, once, for scale
    xs = logits.cpu().numpy()
    for K, lmx in ((16, None), (16, lm)):
        t0 = time.time()
        for b in range(B):
            br.beam_search(xs[:, b], T, K, canon=canon, lm=lmx, alpha=0.8 if lmx is not None else 0.0, beta=1.0 if lmx is not None else 0.0)
        say("CPU restatement (fp64 numpy, one thread), K=%d %s: %.2f s per batch" % (K, "with the 6-gram" if lmx is not None else "no LM",
                                                                                      time.time() - t0))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
