"""A change to the CTC kernels that must move neither bits nor time: the in-tree libvocr.so against the PARENT commit's library at
scripts/_cut/libvocr.so (build a clean checkout of the parent outside the tree and copy its libvocr.so there), both loaded with ctypes
into one process.  --what chooses the entry points:

loss (the alpha/beta sweeps of ctc.hip): vocr_ctc_loss_grad.
  Bits: every (case, regime) of tests.ctc_ref.all_cases() at each max_label_len of tests/test_ctc_fp64_gpu.py's forced() (every launch
  path that admits the batch); SHA-256 of nll, of dlogits and of the WHOLE workspace (the log-softmax, every alpha / beta row and pad
  column, the rows past act_len that no kernel may write).
  Time: bench_full (T 294, B 32, V 96: one position per lane), c4_ragged (T 588, B 32, V 166: two per lane), generic_long (T 1200, B 2,
  V 166: the LDS path).

labelling (the sweep, the host preamble and the class rule the scorers of a known labelling share): the entries of ENTRIES below.  A
  call is RECORDED where vistaocr_amd.ops makes it - the C arguments and the tensors behind their pointers - and replayed on both
  libraries, so the inputs are the tests' own.
  Bits: vocr_ctc_align, vocr_ctc_edit_scores and vocr_ctc_nbest_grad (with and without weights) on every case of tests/nbest_cases.py,
  the small exact cases of tests/test_align_cpu.py and tests/test_edit_cpu.py (what the GPU tests of both run), the empty and invalid
  labellings of their edge cases, and two lines of 4000 frames with 1796 and 1554 labels (beyond 1663 the alignment keeps its rows in
  the workspace); vocr_ctc_entropy, without and with its coefficients, on every case of tests/test_entropy_gpu.py (the seam shapes:
  31 - 33 and 63 - 65 labels, lens 1 .. 17 and 65 .. 74, V 2 / 96 / 256, classes with -inf members, the bad and the empty line) and on
  the 3500-frame line of 1554 labels alone (the two-row layout near its limit of 1663); vocr_ctc_keyword_scores on every call the tests of tests/test_kws_gpu.py make; vocr_ctc_beam_search and
  vocr_ctc_word_beam_search on one English-canon case each of tests/beam_cases.py.  SHA-256 of every output and of the whole workspace.
  Time: T 294, B 32, V 96 (scripts/align_bench.py, edit_bench.py, risk_bench.py), the n = 4 and n = 16 best of a K = 16 search on peaky
  logits at p_char 0.35 (43 - 67 labels: the rows in LDS) and 0.10 (5 - 24 labels: one position per lane), packed to the longest;
  vocr_ctc_entropy on the 1-best of the same search, scores only and with the gradient.

search (the three prefix beam searches: vocr_ctc_beam_search and vocr_ctc_grammar_beam_search, one templated kernel of ctc_beam.hip,
  and vocr_ctc_word_beam_search), recorded and replayed as above.
  Bits: every character case of tests/beam_cases.py (dense, variants, ties, come-back, intermediate beams, the K = 128, V = 256
  launch) and its word cases, through the _run of tests/test_beam_fp64_gpu.py and tests/test_word_beam_fp64_gpu.py; the dense and trie
  cases of tests/grammar_beam_cases.py; every call that the Sigma*, bad-index and poisoned-row, K = 128 alphabet and distance-rule
  tests of tests/test_grammar_beam_gpu.py make.  SHA-256 of every output and of the whole workspace (the node pool).
  Time: T 294, B 32, V 96, the English classes, peaky logits at p_char 0.35, K = 16 and 64: the character search and the grammar search
  under the one-state automaton and under a date regex, without an LM and with the synthetic 6-gram of scripts/beam_bench.py; the word
  search with the LM of scripts/word_beam_bench.py.

Bits, all: outputs and workspace are filled with a constant before the call, so bytes that no kernel writes compare equal trivially;
every digest pair must be equal, and the script exits 1 otherwise.
Time, all: the whole call with HIP events, both libraries warmed up on every shape, then windows of --window calls alternating between
the libraries for --rounds rounds.  Per shape and library: the median of the round medians, and the parent's own max - min over its
rounds, which is the only margin: the new median must not exceed the parent's median plus that spread.

    python scripts/ctc_parent_ab.py [--what loss|labelling|search] [--window 200] [--rounds 5] [--out profiles/ctc_<what>_ab.txt]"""
import argparse
import ctypes
import functools
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vistaocr_amd import _lib                                # noqa: E402
from tests import ctc_ref as cr                              # noqa: E402
from tests.test_ctc_fp64_gpu import forced, kernel_of        # noqa: E402

FILL = -3.0
TIMED = ("bench_full", "c4_ragged", "generic_long")


# labelling: C entry -> (its workspace-size function, where that function's arguments sit in the entry's argument list - or a callable
# of that list for one that is no argument of the entry -, the output pointers, the workspace pointer; the workspace's size follows it)
ENTRIES = {
    "vocr_ctc_align": ("vocr_ctc_align_workspace_bytes", (2, 3, 4, 8, 10), (11, 12, 13), 14),
    "vocr_ctc_edit_scores": ("vocr_ctc_edit_workspace_bytes", (2, 3, 4, 8, 10), (11, 12, 13, 14), 15),
    "vocr_ctc_nbest_grad": ("vocr_ctc_nbest_workspace_bytes", (2, 3, 4, 8, 10), (12, 13), 14),
    "vocr_ctc_entropy": ("vocr_ctc_entropy_workspace_bytes", (2, 3, 4, 9, lambda a: int(a[10] is not None)), (11, 12, 13), 14),
    "vocr_ctc_keyword_scores": ("vocr_ctc_keyword_workspace_bytes", (2, 3, 4, 9, 11), (12, 13, 14), 15),
    "vocr_ctc_beam_search": ("vocr_ctc_beam_workspace_bytes", (2, 3, 4, 6, 7), (16, 17, 18), 19),
    "vocr_ctc_word_beam_search": ("vocr_ctc_word_beam_workspace_bytes", (2, 3, 4, 6, 7), (29, 30, 31), 32),
    "vocr_ctc_grammar_beam_search": ("vocr_ctc_grammar_beam_workspace_bytes", (2, 3, 4, 6, 7), (21, 22, 23), 24),
}
SEARCHES = ("vocr_ctc_beam_search", "vocr_ctc_grammar_beam_search", "vocr_ctc_word_beam_search")


def open_lib(path):
    lib = ctypes.CDLL(path)
    for name in ["vocr_ctc_workspace_bytes", "vocr_ctc_loss_grad", "vocr_last_error"] + list(ENTRIES) + [e[0] for e in ENTRIES.values()]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


class Call:
    """one batch on the device and what vocr_ctc_loss_grad needs for it at max_label_len `mll`"""

    def __init__(self, x, flat, ll, act, mll, nbytes):
        self.shape, self.mll = tuple(x.shape), int(mll)
        off = np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int32)
        self.x = x.contiguous().cuda()
        self.ints = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (flat.numpy(), off, ll, act)]
        self.nll = torch.empty(len(ll), dtype=torch.float32, device="cuda")
        self.dl = torch.empty(self.shape, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")

    def run(self, lib):
        T, B, V = self.shape
        rc = lib.vocr_ctc_loss_grad(self.x.data_ptr(), *[a.data_ptr() for a in self.ints], self.nll.data_ptr(), self.dl.data_ptr(),
                                    self.ws.data_ptr(), T, B, V, self.mll, None)
        if rc != 0:
            raise RuntimeError("vocr_ctc_loss_grad failed (%d): %s" % (rc, (lib.vocr_last_error() or b"?").decode()))

    def digests(self, lib):
        for t in (self.nll, self.dl, self.ws):
            t.fill_(FILL)
        self.run(lib)
        torch.cuda.synchronize()
        return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (self.nll, self.dl, self.ws)]


@functools.lru_cache(maxsize=1)
def _case(name, regime):
    return cr.build_case(name, regime)


def make_call(libs, name, regime, mll=None):
    x, flat, ll, act, _ = _case(name, regime)
    mll = max(ll) if mll is None else mll
    sizes = {lib.vocr_ctc_workspace_bytes(*x.shape, mll) for lib in libs}
    assert len(sizes) == 1 and min(sizes) > 0, "the two libraries size the workspace differently: %s" % sorted(sizes)
    return Call(x, flat, ll, act, mll, sizes.pop()), max(ll)


def window(call, lib, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        call.run(lib)
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) * 1e3          # us


def race(call, libs, window_calls, rounds):
    """call.run(lib) timed in alternating windows; returns (new median, parent median, parent spread, new rounds, parent rounds)"""
    med = {0: [], 1: []}
    for r in range(rounds):
        for i in ((0, 1) if r % 2 == 0 else (1, 0)):
            med[i].append(window(call, libs[i], window_calls))
    return float(np.median(med[0])), float(np.median(med[1])), max(med[1]) - min(med[1]), med[0], med[1]


class Replay:
    """one recorded call of an ENTRIES entry: its C arguments, the tensors behind its output and workspace pointers"""

    def __init__(self, name, args, tensors):
        _, _, outs, ws = ENTRIES[name]
        self.name, self.args = name, args
        self.outs = [tensors[args[i]] for i in outs if args[i] is not None]
        self.ws = tensors[args[ws]]
        self.keep = tensors                                   # the inputs stay alive with the call

    def run(self, lib):
        rc = getattr(lib, self.name)(*self.args)
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (self.name, rc, (lib.vocr_last_error() or b"?").decode()))

    def sizes(self, lib):
        fn, where, _, _ = ENTRIES[self.name]
        return getattr(lib, fn)(*[i(self.args) if callable(i) else self.args[i] for i in where])

    def digests(self, lib):
        for t in self.outs + [self.ws]:
            t.fill_(FILL)
        self.run(lib)
        torch.cuda.synchronize()
        return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in self.outs + [self.ws]]


class Recorder:
    """while active, every call of an ENTRIES entry that vistaocr_amd.ops makes and that succeeds is kept as a Replay"""

    def __enter__(self):
        from vistaocr_amd import ops
        self.calls, self.tensors, self.ops, self.p, self.call = [], {}, ops, ops._p, ops.call

        def p(t):
            if t is not None:
                self.tensors[t.data_ptr()] = t
            return self.p(t)

        def call(name, *args):
            self.call(name, *args)
            if name in ENTRIES:
                self.calls.append(Replay(name, args, dict(self.tensors)))

        ops._p, ops.call = p, call
        return self

    def __exit__(self, *exc):
        self.ops._p, self.ops.call = self.p, self.call
        self.tensors = {}


def record(fn, *a, **k):
    with Recorder() as rec:
        fn(*a, **k)
    return rec.calls


def labelling_calls(x, lens, labels, label_lens, canon, w):
    """the four calls on one batch of device tensors: alignment, edit scores, n-best with and without weights"""
    from vistaocr_amd import ops

    def go():
        ops.ctc_align(x, lens, labels, label_lens, canon)
        ops.ctc_edit_scores(x, lens, labels, label_lens, canon)
        ops.ctc_nbest(x, lens, labels, label_lens, canon, w)
        ops.ctc_nbest(x, lens, labels, label_lens, canon)
    calls = record(go)
    assert [c.name for c in calls] == ["vocr_ctc_align", "vocr_ctc_edit_scores", "vocr_ctc_nbest_grad", "vocr_ctc_nbest_grad"]
    return list(zip(("align", "edit", "nbest+w", "nbest"), calls))


def entropy_calls(x, lens, labels, label_lens, canon, coeff):
    """the two calls of the entropy entry on one batch of device tensors (labels [B,L]): scores only, and with the gradient"""
    from vistaocr_amd import ops

    def go():
        ops.ctc_entropy(x, lens, labels, label_lens, canon)
        ops.ctc_entropy(x, lens, labels, label_lens, canon, coeff)
    calls = record(go)
    assert [c.name for c in calls] == ["vocr_ctc_entropy"] * 2 and calls[0].args[10] is None and calls[1].args[10] is not None
    return list(zip(("entropy", "entropy+c"), calls))


def host_batch(x, lens, hyps, canon, width=None):
    """numpy logits [T,B,V] and hyps[b][q] (lists or None) as the device tensors of labelling_calls"""
    from tests import nbest_ref as nr
    M = max([len(h) for row in hyps for h in row if h is not None] + [1]) if width is None else width
    n = max(len(row) for row in hyps)
    labels, label_lens = nr.pack([list(row) + [None] * (n - len(row)) for row in hyps], M, "cuda")
    B = len(hyps)
    w = torch.linspace(-1.0, 1.0, B * n, device="cuda").reshape(B, n).contiguous()
    cd = None if canon is None else torch.as_tensor(np.asarray(canon), dtype=torch.int32).cuda()
    return (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(), torch.tensor([int(v) for v in lens], dtype=torch.int32).cuda(),
            labels, label_lens, cd, w)


def labelling_bit_cases():
    """(case name, [(entry label, Replay)])"""
    from tests import align_ref as ar
    from tests import beam_cases as bc
    from tests import beam_data as bd
    from tests import nbest_cases as nc
    from tests import test_align_cpu as tac
    from tests import test_beam_fp64_gpu as tb
    from tests import test_edit_cpu as tec
    from tests import test_entropy_gpu as te
    from tests import test_kws_gpu as tk
    from tests import test_nbest_gpu as tn
    from tests import test_word_beam_fp64_gpu as tw
    for c in nc.CASES:
        yield "nbest_cases " + c[0], labelling_calls(*tn._device_case(nc.build_case(c[0])))
    for i, (T, V, labels, canon) in enumerate(tac.EXACT):
        yield "align exact %d" % i, labelling_calls(*host_batch(tac.exact_logits(i, T, V)[:, None, :], [T], [[labels]], canon))
    for i, (T, V, length, labels, canon, _) in enumerate(tec.CASES):
        yield "edit exact %d" % i, labelling_calls(*host_batch(tec.case_logits(i)[:, None, :], [length], [[labels]], canon))
    x = np.random.default_rng(21).normal(0, 1, (40, 7, 96)).astype(np.float32)       # test_edge_cases / test_edge_shapes
    g = [ar.greedy_labels(x[:, b], 40) for b in range(7)]
    yield "empty and invalid", labelling_calls(*host_batch(x, [0, 0, 40, 3, 40, 40, 40],
                                                           [[[]], [g[1][:3]], [[]], [g[3][:9]], [[5, 96, 7]], [[5, 0, 7]], [[-3]]], None))
    yield "ragged, 6 labels", labelling_calls(*host_batch(x, [0, 1, 40, 17, 2, 39, 33], [[g[b][:6]] for b in range(7)], None))
    x = bd.peaky_logits(np.random.default_rng(31), 4000, 2, 96, p_char=0.9)           # test_long_lines_keep_rows_and_back_pointers_in_the_workspace
    hyps = [[ar.greedy_labels(x[:, b], ln)] for b, ln in enumerate((4000, 3500))]
    assert len(hyps[0][0]) > 1663 > len(hyps[1][0]) > 1000
    yield "T 4000, %d and %d labels" % (len(hyps[0][0]), len(hyps[1][0])), labelling_calls(*host_batch(x, [4000, 3500], hyps, None))
    for c in te.CASES:
        yield "entropy " + c[0], entropy_calls(*te._device_case(te.build_case(c[0])))
    xd, lens, labels, label_lens, _, _ = host_batch(x[:3500, 1:2], [3500], [hyps[1]], None)
    yield "T 3500, %d labels" % len(hyps[1][0]), entropy_calls(xd, lens, labels[:, 0].contiguous(), label_lens[:, 0].contiguous(), None,
                                                             torch.tensor([[0.75, -0.5]], device="cuda"))
    kws = [(tk.test_query_lengths_and_lane_layouts, (L,)) for L in tk.QUERY_LENGTHS]
    kws += [(f, ()) for f in (tk.test_mixed_lengths_land_at_the_callers_index, tk.test_frame_counts,
                              tk.test_alphabet_sizes_classes_and_minus_infinity, tk.test_peak_before_the_start_and_after_the_end,
                              tk.test_tie_rule, tk.test_anchors_and_the_forward_score, tk.test_trimmed_spans,
                              tk.test_invalid_queries_poison_only_their_own_column)]
    for fn, a in kws:
        calls = [c for c in record(fn, *a) if c.name == "vocr_ctc_keyword_scores"]
        yield "kws %s%s" % (fn.__name__[5:29], a if a else ""), [("keyword %d" % i, c) for i, c in enumerate(calls)]
    case = bc.char_case("K16_lm")
    yield "beam_cases K16_lm", [("beam", record(tb._run, case.x, case.lens, case.K, case.nbest, canon=case.canon, lm=case.lm, alpha=case.alpha,
                                                beta=case.beta, prune=case.prune)[0])]
    case = bc.word_case("w_K16_oov")
    yield "beam_cases w_K16_oov", [("word beam", record(tw._run, case.x, case.lens, case.K, case.nbest, case.lm, canon=case.canon,
                                                        alpha=case.alpha, beta=case.beta, oov=case.oov)[0])]


def labelling_timed_cases():
    """(shape name, longest labelling, [(entry label, Replay)]): the n best of a K = 16 search over the English classes, and its 1-best
    for the entropy entry"""
    import vistaocr_amd as va
    from tests import beam_data as bd
    from vistaocr_amd import ops
    T, B, V = 294, 32, 96
    canon = np.array(va.english_alphabet().canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    for p_char in (0.35, 0.10):
        xd = torch.from_numpy(bd.peaky_logits(np.random.default_rng(7), T, B, V, classes=cls, p_char=p_char)).cuda()
        lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
        for n in (4, 16):
            lab, ln, _ = ops.ctc_beam_search(xd, [T] * B, cd, 16, n)
            M = max(int(ln.max()), 1)
            w = torch.linspace(-1.0, 1.0, B * n, device="cuda").reshape(B, n).contiguous()
            yield "p_char %.2f n %2d" % (p_char, n), M, labelling_calls(xd, lens, lab[:, :, :M].contiguous(), ln.contiguous(), cd, w)
        lab, ln, _ = ops.ctc_beam_search(xd, [T] * B, cd, 16, 1)
        M = max(int(ln.max()), 1)
        coeff = torch.tensor([[1.0, -0.2]] * B, device="cuda")
        yield "p_char %.2f 1-best" % p_char, M, entropy_calls(xd, lens, lab[:, 0, :M].contiguous(), ln[:, 0].contiguous(), cd, coeff)


def search_bit_cases():
    """(case name, [(entry label, Replay)]): the three beam searches on the tests' own inputs"""
    from tests import beam_cases as bc
    from tests import grammar_beam_cases as gc
    from tests import test_beam_fp64_gpu as tb
    from tests import test_grammar_beam_gpu as tg
    from tests import test_word_beam_fp64_gpu as tw
    label = {"vocr_ctc_beam_search": "beam", "vocr_ctc_grammar_beam_search": "grammar", "vocr_ctc_word_beam_search": "word beam"}
    for name in bc.CHAR_DENSE + bc.CHAR_VARIANTS + bc.CHAR_TIES + bc.CHAR_COMEBACK + bc.CHAR_INTERMEDIATE + ["big_K128_V256"]:
        case = bc.char_case(name)
        yield "char " + name, [("beam", record(tb._run, case.x, case.lens, case.K, case.nbest, canon=case.canon, lm=case.lm,
                                               alpha=case.alpha, beta=case.beta, prune=case.prune)[0])]
    for name in bc.WORD_DENSE + ["w_big_K128_V256", "w_tie_lm_K6"]:
        case = bc.word_case(name)
        yield "word " + name, [("word beam", record(tw._run, case.x, case.lens, case.K, case.nbest, case.lm, canon=case.canon,
                                                    alpha=case.alpha, beta=case.beta, oov=case.oov)[0])]
    for name in gc.DENSE + gc.TRIE:
        yield "grammar " + name, [("grammar", record(tg._search, gc.case(name))[0])]
    fns = [(tg.test_sigma_star_is_the_existing_kernel, (K, with_lm)) for K in (1, 16, 128) for with_lm in (False, True)]
    fns += [(f, ()) for f in (tg.test_per_line_automata_bad_indices_and_a_poisoned_row, tg.test_smallest_and_largest_alphabet_at_K128,
                              tg.test_corners_of_the_distance_rule)]
    for fn, a in fns:
        calls = [c for c in record(fn, *a) if c.name in SEARCHES]
        yield "%s%s" % (fn.__name__[5:35], a if a else ""), [("%s %d" % (label[c.name], i), c) for i, c in enumerate(calls)]


def search_timed_cases():
    """(shape name, K, [(entry label, Replay)]): T 294, B 32, V 96, the English classes, peaky logits at p_char 0.35, nbest 1; the
    character search, the grammar search under the one-state automaton and under scripts/grammar_beam_bench.py's date regex, without an
    LM and with scripts/beam_bench.py's synthetic 6-gram; the word search with scripts/word_beam_bench.py's LM, open vocabulary"""
    import tempfile
    import vistaocr_amd as va
    from tests import beam_data as bd
    from tests import word_beam_data as wd
    from vistaocr_amd import ops
    from vistaocr_amd.grammar import Grammar, pack_dense_grammars
    T, B, V = 294, 32, 96
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    xd = torch.from_numpy(bd.peaky_logits(np.random.default_rng(7), T, B, V, classes=cls, p_char=0.35)).cuda()
    lens = [T] * B
    tmp = tempfile.mkdtemp()
    path = bd.write_char_arpa(os.path.join(tmp, "char6.arpa"), [al.idx_to_char[c] for c in range(1, 40)], order=6, lines=600, seed=1)
    clm = va.CharNgramLM.from_arpa(path, al).to("cuda")
    rng = np.random.default_rng(5)
    words, wts = wd.make_lexicon(rng, 20000, min_len=2, max_len=10)
    sents = wd.make_sentences(rng, words, wts, 40000 + B)
    wlm = va.WordNgramLM.from_arpa(wd.write_word_arpa(os.path.join(tmp, "word3.arpa"), words, wts, sents[:40000], seed=6), al).to("cuda")
    sigma, date = (pack_dense_grammars([Grammar.from_regex(al, r)], "cuda") for r in (".*", r"\d{4}-\d\d-\d\d"))
    for K in (16, 64):
        for lname, lm, a, bb in (("no LM", None, 0.0, 0.0), ("6-gram", clm, 0.8, 1.0)):
            def go():
                ops.ctc_beam_search(xd, lens, cd, K, 1, lm, a, bb)
                ops.ctc_grammar_beam_search(xd, lens, sigma, None, cd, K, 1, lm, a, bb)
                ops.ctc_grammar_beam_search(xd, lens, date, None, cd, K, 1, lm, a, bb)
            yield lname, K, list(zip(("beam", "g. Sigma*", "g. date"), record(go)))
        yield "word 3-gram", K, [("word beam", record(ops.ctc_word_beam_search, xd, lens, cd, wlm, K, 1, 0.8, 0.5, -5.0)[0])]


def replay_tables(libs, args, say, bit_cases, timed_cases, col="M"):
    """the two tables of a mode made of recorded calls; `col`: what the timed cases' second field is"""
    new, parent = libs
    say("bits: SHA-256 (first 12 hex digits) of every output and of the whole workspace, all filled with %g before the call" % FILL)
    fmt = "%-42s %-11s | %-64s | %s"
    say(fmt % ("case", "entry", "outputs in the C order, workspace", "new vs parent"))
    differ = pairs = 0
    for case, calls in bit_cases():
        for label, call in calls:
            assert call.sizes(new) == call.sizes(parent) > 0, "the two libraries size the workspace differently: %s %s" % (case, label)
            dn, dp = call.digests(new), call.digests(parent)
            bad = sum(a != b for a, b in zip(dn, dp))
            differ, pairs = differ + bad, pairs + len(dn)
            say(fmt % (case, label, " ".join(d[:12] for d in dn), "equal" if not bad else "DIFFER (parent %s)" % " ".join(d[:12] for d in dp)))
    say("digest pairs: %d, of which differ: %d" % (pairs, differ))
    say("")
    say("time: the whole call (every kernel behind it), HIP events, us; per round the median of a window of "
        "%d calls, the libraries alternating, %d rounds after a warm-up window of each" % (args.window, args.rounds))
    tfmt = "%-17s %3s %-9s | %9s %9s %9s | %9s | %s"
    say(tfmt % ("shape", col, "entry", "parent", "p. spread", "new", "new - p.", "new <= parent + spread"))
    slower = 0
    for shape, M, calls in timed_cases():
        for label, call in calls:
            for lib in libs:
                window(call, lib, args.window)
            mn, mp, spread, rn, rp = race(call, libs, args.window, args.rounds)
            ok = mn <= mp + spread
            slower += not ok
            say(tfmt % (shape, M, label, "%.2f" % mp, "%.2f" % spread, "%.2f" % mn, "%+.2f" % (mn - mp), "yes" if ok else "NO"))
            say("    rounds, parent: %s   new: %s" % (" ".join("%.2f" % v for v in rp), " ".join("%.2f" % v for v in rn)))
    say("shapes slower than the parent's median plus its spread: %d" % slower)
    return differ, slower


def loss_tables(libs, args, say):
    new, parent = libs
    say("bits: SHA-256 (first 12 hex digits) of nll, dlogits and the whole workspace, filled with %g before the call" % FILL)
    fmt = "%-17s %-12s %4s %-7s | %-12s %-12s %-12s | %s"
    say(fmt % ("case", "regime", "mll", "path", "nll", "dlogits", "workspace", "new vs parent"))
    differ = 0
    for name, regime in cr.all_cases():
        lmax = max([c for c in cr.GPU_CASES if c[0] == name][0][4])
        for mll in forced(lmax):
            call, _ = make_call(libs, name, regime, mll)
            dn, dp = call.digests(new), call.digests(parent)
            bad = [w for w, a, b in zip(("nll", "dlogits", "workspace"), dn, dp) if a != b]
            differ += len(bad)
            say(fmt % (name, cr.regime_name(regime), mll, kernel_of(mll), dn[0][:12], dn[1][:12], dn[2][:12],
                       "equal" if not bad else "DIFFER: %s (parent %s)" % (", ".join(bad), " ".join(d[:12] for d in dp))))
    say("digest pairs that differ: %d" % differ)
    say("")
    say("time: vocr_ctc_loss_grad, the whole call (log-softmax, alpha/beta, gradient), HIP events, us; per round the median of a window "
        "of %d calls, the libraries alternating, %d rounds after a warm-up window of each" % (args.window, args.rounds))
    tfmt = "%-13s %-7s %5s %3s %4s | %9s %9s %9s | %9s | %s"
    say(tfmt % ("shape", "path", "T", "B", "V", "parent", "p. spread", "new", "new - p.", "new <= parent + spread"))
    slower = 0
    calls = [make_call(libs, name, cr.DENSE) for name in TIMED]
    for call, _ in calls:
        for lib in libs:
            window(call, lib, args.window)
    for name, (call, lmax) in zip(TIMED, calls):
        mn, mp, spread, rn, rp = race(call, libs, args.window, args.rounds)
        ok = mn <= mp + spread
        slower += not ok
        say(tfmt % (name, kernel_of(lmax), *call.shape, "%.2f" % mp, "%.2f" % spread, "%.2f" % mn, "%+.2f" % (mn - mp),
                    "yes" if ok else "NO"))
        say("    rounds, parent: %s   new: %s" % (" ".join("%.2f" % v for v in rp), " ".join("%.2f" % v for v in rn)))
    say("shapes slower than the parent's median plus its spread: %d" % slower)
    return differ, slower


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "_cut", "libvocr.so"))
    ap.add_argument("--what", choices=("loss", "labelling", "search"), default="loss")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", {"loss": "ctc_mirror_ab.txt", "labelling": "ctc_labelling_ab.txt",
                                                      "search": "ctc_search_ab.txt"}[args.what])
    assert args.window >= 200 and args.rounds >= 5
    new, parent = open_lib(_lib.LIB_PATH), open_lib(args.parent)
    libs = (new, parent)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("new: %s   parent: %s" % (os.path.relpath(_lib.LIB_PATH, ROOT), os.path.relpath(args.parent, ROOT)))
    say("")
    if args.what == "loss":
        differ, slower = loss_tables(libs, args, say)
    elif args.what == "labelling":
        differ, slower = replay_tables(libs, args, say, labelling_bit_cases, labelling_timed_cases)
    else:
        differ, slower = replay_tables(libs, args, say, search_bit_cases, search_timed_cases, col="K")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if differ or slower else 0


if __name__ == "__main__":
    sys.exit(main())
