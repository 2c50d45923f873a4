"""Time vocr_ctc_word_beam_search on configs[1]'s logits shape (T = 294, B = 32, V = 96) for K in {1, 4, 16, 64} with a synthetic word
3-gram over a 20 000-word Zipf lexicon (tests/word_beam_data.py), closed and open vocabulary, on sentence-peaky logits and on the
logits of an untrained configs[1] model; beside it the eval forward of that batch and vocr_ctc_beam_search with a character 6-gram
at the same K on the same logits.  Also the host time of WordNgramLM.from_arpa and the table sizes.  HIP events, warm-up, median
of repeats.  Output: profiles/r08_word_beam_bench.txt.

    python scripts/word_beam_bench.py [--repeats 20] [--words 20000] [--out profiles/r08_word_beam_bench.txt]"""
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
from tests import word_beam_data as wd                       # noqa: E402

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
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--sentences", type=int, default=40000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_word_beam_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
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
        out, lens = model(x, widths)
        fwd = _time(lambda: model(x, widths), args.warmup, args.repeats)
    assert tuple(out.shape) == (T, B, V), tuple(out.shape)
    say("device: %s" % torch.cuda.get_device_name(0))
    say("eval forward, configs[1] batch (32 x 1x30x600 -> logits %s): median %.3f ms (min %.3f, max %.3f)" % ((tuple(out.shape),) + fwd))

    # the word 3-gram: a Zipf lexicon, random sentences with punctuation and digits, estimated counts
    rng = np.random.default_rng(5)
    words, wts = wd.make_lexicon(rng, args.words, min_len=2, max_len=10)
    sents = wd.make_sentences(rng, words, wts, args.sentences + B)
    tmp = tempfile.mkdtemp()
    path = wd.write_word_arpa(os.path.join(tmp, "word3.arpa"), words, wts, sents[:args.sentences], seed=6)
    t0 = time.time()
    wlm = va.WordNgramLM.from_arpa(path, al)
    t_word = time.time() - t0
    say("word LM: 3-gram, %d lexicon words, %d dropped, %d LM states, %d successors, %d trie nodes; tables %.1f MiB "
        "(trie_next %.1f MiB); WordNgramLM.from_arpa %.2f s on the host"
        % (wlm.num_words, wlm.dropped, wlm.num_states, len(wlm.succ_tok), wlm.num_trie_nodes, wlm.table_bytes / 2.0 ** 20,
           wlm.trie_next.size * 4 / 2.0 ** 20, t_word))
    cpath = bd.write_char_arpa(os.path.join(tmp, "char6.arpa"), [al.idx_to_char[c] for c in range(1, 40)], order=6, lines=600, seed=1)
    t0 = time.time()
    clm = va.CharNgramLM.from_arpa(cpath, al)
    say("char LM: 6-gram, %d states (tables %.1f MiB), CharNgramLM.from_arpa %.2f s on the host"
        % (clm.num_states, clm.num_states * V * 8 / 2.0 ** 20, time.time() - t0))
    wd_ = wlm.to("cuda")
    cd_ = clm.to("cuda")
    xs, lens_l = wd.sentence_logits(np.random.default_rng(7), sents[args.sentences:], al, T)
    peaky = torch.from_numpy(xs).cuda()
    dense = out.detach().float().contiguous()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    say("")
    say("T=%d B=%d V=%d, nbest=1; median of %d after %d warm-up (ms per batch).  word: lm_weight 0.8, word_bonus 0.5; open: "
        "oov_penalty -5.  char: the 6-gram, lm_weight 0.8, insertion_bonus 1.0" % (T, B, V, args.repeats, args.warmup))
    say("%-4s %-22s %-14s %10s %10s %10s %12s %10s" % ("K", "decoder", "logits", "median", "min", "max", "vs forward", "vs char"))
    for K in (1, 4, 16, 64):
        for lname, lg in (("sentence-peaky", peaky), ("model (rand)", dense)):
            rc = _time(lambda: ops.ctc_beam_search(lg, lens_l, cd, K, 1, cd_, 0.8, 1.0), args.warmup, args.repeats)
            say("%-4d %-22s %-14s %10.3f %10.3f %10.3f %11.2fx %10s" % ((K, "char 6-gram", lname) + rc + (rc[0] / fwd[0], "")))
            for name, oov in (("word 3-gram closed", None), ("word 3-gram open", -5.0)):
                r = _time(lambda: ops.ctc_word_beam_search(lg, lens_l, cd, wd_, K, 1, 0.8, 0.5, oov), args.warmup, args.repeats)
                say("%-4d %-22s %-14s %10.3f %10.3f %10.3f %11.2fx %9.2fx" % ((K, name, lname) + r + (r[0] / fwd[0], r[0] / rc[0])))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
