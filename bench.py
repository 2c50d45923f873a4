#!/usr/bin/env python
"""bench.py — training line-images/sec of the CnnOcrModel hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

N > 1: started plainly (no WORLD_SIZE in the environment) this script spawns its own N rank processes, one per GPU, and
relays rank 0's JSON line; started under `python -m torch.distributed.run --nproc-per-node N ...` it is one of the ranks.
The parent of a self-launch never touches the GPU (no exec of a GPU-initialised process, children are fresh interpreters).

Workload (modelled on the reference's src/speed_test.py): per GPU a batch of 32
synthetic 1x30x600 grey lines x~U[0,1), 20 labels/line, English alphabet (V=96), 3x BiLSTM-512, lstm_input_dim 128,
dropout 0.5, fp32.  One step = train() of src/train_cnn_lstm.py:131-150: forward + CTC + backward + (RCCL all-reduce of
the flat gradient) + clamp(+-5) + Adam, returning the loss as a Python float.  SURVEY.md §8(d) counts the H2D copy of the image
batch as part of the step, so `value` is the loop fed from a pinned HOST batch (2.3 MB over PCIe inside train()); the same K steps
with the batch already resident in HBM are the side number `resident_input` of --full (the two agree within box noise).
A plain run sets up, warms up, times the K steps and prints ONE JSON line on rank 0 (metric, value, unit, dtype, ms_per_step, ...).
`--full` adds the side measurements and checks: the resident-input loop, the per-family kernel events and the roofline, the
per-entry-point breakdown, the host enqueue time, the GEMM launches alone, the all-reduce times and, on one rank, the parity leg and
the CPU baseline; it exits non-zero if the parity leg finds a label mismatch or a CTC-loss error above 1e-3.
`--dump-outputs DIR` writes what the last timed step left to its caller as DIR/<name>.npy (see dump_outputs)."""
import argparse
import json
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # before the first HIP call: see vistaocr_amd/__init__.py
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md: dense f32 matrix peak (= vector peak)
F16_MFMA_PEAK_TFLOPS = 2500.0    # same guide: BF16/F16 MFMA ~2.5 PF dense (never the 2:1-sparsity figure)
HBM_PEAK_GBS = 8000.0

HP = dict(num_in_channels=1, input_line_height=30, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3,
          num_lstm_hidden_units=512, p_lstm_dropout=0.5)
B, HIMG, WIMG, LABELS = 32, 30, 600, 20
CPU_THREAD_SWEEP = (16, 8, 32, 64, 128)   # the CPU leg times one step at each (most promising first, while the budget lasts) and reports the best
CPU_TIMED_STEPS = 2
PROFILE_STEPS = 5             # un-timed pass that records HIP events around every entry point (breakdown only)


def madcat_widths(n, wmax, seed):
    """n line widths from the width distribution the reference measured on MADCAT (src/madcat.py:58-66: 10 % of the lines up to
    150 px, 20 % up to 200, 45 % up to 300, 70 % up to 350, 90 % up to 450, 99 % up to 600), scaled so that 600 px becomes `wmax`
    (BASELINE configs[3]: "wider ~1200-px lines"), drawn by inverse CDF from seeded uniforms and sorted descending like
    SortByWidthCollater does.  One batch mixes all width classes - more ragged than the reference's width-grouped batches."""
    import numpy as np
    xs = np.array([60, 150, 200, 300, 350, 450, 600, 640], dtype=np.float64) * (wmax / 600.0)
    cdf = np.array([0.0, 0.10, 0.20, 0.45, 0.70, 0.90, 0.99, 1.0])
    u = np.random.RandomState(seed).uniform(size=n)
    w = np.interp(u, cdf, xs)
    return sorted((int(min(wmax, max(16, round(v)))) for v in w), reverse=True)


# configs[1] is the headline; c4 / c5 are BASELINE configs[3] / configs[4] as SIDE lines of the same JSON shape (own workload string, own
# parity leg).  `widths`: per-line widths of a batch, `labels`: labels per line.
WORKLOADS = {
    "c1": dict(hp=HP, alphabet="english", himg=30, widths=[600] * B, labels=[20] * B, conv_dtype="fp32", parity_seed=56,
               what="configs[1]: 32 synthetic 1x30x600 grey lines per GPU, 20 labels/line, V=96"),
    "c4": dict(hp=HP, alphabet="arabic", himg=30, widths=madcat_widths(B, 1200, 4), labels=None, conv_dtype="fp32", parity_seed=93,
               what="configs[3]: MADCAT-style Arabic alphabet (V=166), 32 synthetic 1x30xW grey lines per GPU with W from the MADCAT width "
                    "distribution of src/madcat.py:58-66 scaled to <= 1200 px (one ragged batch across all width classes, sorted descending, "
                    "zero-padded to the widest), W // 30 labels/line"),
    "c5": dict(hp=dict(HP, input_line_height=60), alphabet="english", himg=60, widths=[1200] * B, labels=[40] * B, conv_dtype="fp16", parity_seed=1,
               what="configs[4]: 32 synthetic 1x60x1200 grey lines per GPU (ASAR'18-style high resolution: rapid_ds 60 -> 30), 40 labels/line, "
                    "V=96, fp16 conv operands with fp32 accumulation, everything else fp32"),
}
for _w in WORKLOADS.values():
    if _w["labels"] is None:
        _w["labels"] = [max(1, v // 30) for v in _w["widths"]]
WL = WORKLOADS["c1"]


def select_workload(name):
    global WL
    WL = WORKLOADS[name]
    return WL


def alphabet_of(wl):
    import vistaocr_amd as va
    return va.english_alphabet() if wl["alphabet"] == "english" else va.arabic_alphabet()


def make_batch(rank, vocab):
    import torch
    g = torch.Generator().manual_seed(1234 + rank)
    widths = torch.tensor(WL["widths"], dtype=torch.int32)
    x = torch.rand(B, 1, WL["himg"], int(widths.max()), generator=g)
    for b, w in enumerate(WL["widths"]):                  # the collater's zero padding right of each line
        x[b, :, :, w:] = 0.0
    tl = torch.tensor(WL["labels"], dtype=torch.int32)
    tgt = torch.randint(1, vocab, (int(tl.sum()),), generator=g).to(torch.int32)
    return x, tgt, widths, tl


def parity_samples():
    import torch
    g = torch.Generator().manual_seed(777)
    return torch.rand(B, 64, 2, generator=g), torch.rand(B, 128, 2, generator=g)


# Parity leg: random-init weights emit almost no labels (the blank wins every frame), so the label comparison would be vacuous.
# The leg therefore loads the tests' closed-form weights (recurrent weights in the reference's own +-0.08 init range, output layer
# widened so that ~6000 labels come out of the 32 lines) and a closed-form batch whose seed was chosen on the ORACLE side for a
# greedy-decode margin >= 1e-3 (scripts/margin_search.py bench 1 300); the oracle re-computes and reports the margin on the box.
PARITY_STATE_KW = dict(lstm_scale=0.08, prob_scale=2.0)
PARITY_BATCH_SEED = None        # override of the workload's parity_seed (scripts/margin_search.py bench; c1: seed 56 of 299, margin 1.02e-3)


def parity_inputs(hidden, vocab):
    """(state dict as numpy, x, widths, targets, target_lens) of the parity leg - closed forms shared with tests/ (oracle/closed_form.py
    holds no arithmetic of the path: seeded tensors only)."""
    from oracle import closed_form as cf
    hp = dict(WL["hp"], num_lstm_hidden_units=hidden)
    sd_np = cf.closed_form_state(hp, vocab, **PARITY_STATE_KW)
    seed = PARITY_BATCH_SEED if PARITY_BATCH_SEED is not None else WL["parity_seed"]
    x, w, tgt, tl = cf.closed_form_batch(B, 1, WL["himg"], WL["widths"], vocab, WL["labels"], seed=seed)
    return sd_np, x, w, tgt, tl


DUMP_BUDGET_ELEMS = 14 << 20      # 56 MiB of float32 over all arrays of --dump-outputs


def dump_outputs(out_dir, model, loss):
    """What a caller of train() holds after the last timed step: the loss it returned (loss.npy, float64) and the model's state that
    the step updated in place, parameters and BatchNorm buffers, as <state-dict key>.npy (float32; integer buffers float64).  Arrays
    are written whole, smallest first, while each fits its share of DUMP_BUDGET_ELEMS; a larger one is written as a 1-D sample at flat
    indices drawn without replacement by numpy RandomState(0) and sorted, so the same arguments give the same sample on every run."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), np.array([loss], dtype=np.float64))
    state = [(k, v.detach().cpu().numpy()) for k, v in model.state_dict().items()]
    left, todo = DUMP_BUDGET_ELEMS, len(state)
    for name, a in sorted(state, key=lambda kv: kv[1].size):
        a = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
        share = left // todo
        if a.size > share:
            a = a.ravel()[np.sort(np.random.RandomState(0).choice(a.size, share, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.size * a.itemsize // 4
        todo -= 1


def conv_flops(args):
    n, cin, h, w, cout = args[4:9]
    return 2.0 * n * h * w * cin * cout * 9


def gemm_flops(args):
    m, n, k = args[2:5]
    return 2.0 * m * n * k


def gemm_pair_flops(args):
    m, n, k = args[3:6]
    return 2 * 2.0 * m * n * k                   # two products (mode 0) or one product with two K segments (mode 1)


def lstm_flops(args, first_dim_arg):
    t, b, h = args[first_dim_arg:first_dim_arg + 3]
    return 2.0 * 2 * t * b * h * 4 * h           # both directions: [B, H] x [H, 4H] per time step


# MFMA FLOPs a launch EXECUTES per algorithmic FLOP: the F(2,3) kernels issue 4 multiplications where the direct form needs 6, the
# F(4,3) kernel (forward / data-gradient launches with >= 64 output channels) 6 where it needs 12.  The shipped library has one code
# path per shape (the kernel-variant switches exist only in -DVOCR_EXPERIMENTS builds), so these are constants of the product
_WINO4 = True
# the weight gradient applies F(3,2) along the row AND across row pairs: 16 multiplications where the direct form needs 36, times
# 2 ceil(H/2) / H (an odd height's last pair is half empty)
_WGRAD2D = True


def executed_share(name, args):
    if name == "vocr_conv3x3_wino_fwd":
        return 0.5 if (_WINO4 and args[8] >= 64) else 2.0 / 3.0
    if name == "vocr_conv3x3_wgrad_wino":
        h = args[6]
        return (4.0 / 9.0) * (2.0 * ((h + 1) // 2) / h) if (_WGRAD2D and (args[5] * args[8]) % 4 == 0) else 2.0 / 3.0
    return 1.0


def lstm_packed_flops(args, h_arg):
    h, rows = args[h_arg], args[h_arg + 1]       # packed rows (include/vocr.h): the frames the sweep computes, plus the zero groups
    return 2.0 * 2 * rows * h * 4 * h


def gemm_x6_flops(args):
    m, n, k = args[10:13]
    return 2.0 * m * n * k


FLOPS_OF = {"vocr_gemm_x6": gemm_x6_flops, "vocr_gemm_h3": gemm_x6_flops,
            "vocr_gemm_x6_two_views": lambda a: 2.0 * a[7] * a[8] * a[9], "vocr_gemm_h3_two_views": lambda a: 2.0 * a[7] * a[8] * a[9], "vocr_conv3x3_fwd": conv_flops, "vocr_conv3x3_wino_fwd": conv_flops, "vocr_conv3x3_wgrad": conv_flops,
            "vocr_conv3x3_wgrad_wino": conv_flops, "vocr_conv3x3_f16_fwd": conv_flops, "vocr_conv3x3_wgrad_f16": conv_flops,
            "vocr_conv3x3_h16_fwd": conv_flops, "vocr_conv3x3_wgrad_h16": conv_flops,
            "vocr_gemm": gemm_flops, "vocr_gemm_pair": gemm_pair_flops,
            "vocr_lstm_fwd": lambda a: lstm_flops(a, 8), "vocr_lstm_fwd_range": lambda a: lstm_flops(a, 8),
            "vocr_lstm_bwd_bias": lambda a: lstm_flops(a, 9),
            "vocr_lstm_fwd_packed": lambda a: lstm_packed_flops(a, 10), "vocr_lstm_bwd_packed": lambda a: lstm_packed_flops(a, 12)}
_F16_CONV = ("conv3x3 with fp16 operands, fp32 accumulate (conv3x3_h16_kernel on NHWC fp16 activations: forward + data gradient; conv3x3_wgrad_h16_kernel on "
             "channel-major fp16 copies: weight gradient; the register-staged kernels where the channel counts do not fit; v_mfma_f32_32x32x16_f16)")
_X6_GEMM = ("dense fp32 GEMMs on the bf16 matrix pipe (gemm_x6_kernel behind vocr_gemm_x6: every fp32 operand split EXACTLY into three bf16 planes, six "
            "v_mfma_f32_32x32x16_bf16 per fp32 product, fp32 accumulate, error below the f32-MFMA kernels' against fp64 - the LSTM projections and their "
            "dX / dW; FLOPs counted as the fp32 products they replace, peak = the bf16 MFMA peak / 6 = 416.7 TFLOP/s)")
X6_EQUIV_PEAK_TFLOPS = F16_MFMA_PEAK_TFLOPS / 6.0      # six bf16 MFMAs per fp32 product
# the opt-in split (VOCR_LSTM_GEMM=fp16x3 / ops.set_lstm_gemm): not what the headline line runs
_H3_GEMM = ("dense GEMMs as fp16x3 products (gemm_x6_kernel<., 2> behind vocr_gemm_h3: every fp32 operand as two fp16 planes with per-row power-of-two scales, "
            "three v_mfma_f32_32x32x16_f16 per product, fp32 accumulate - a norm-wise fp32-grade approximation, OPT-IN; FLOPs counted as the products they "
            "replace, peak = the fp16 MFMA peak / 3 = 833.3 TFLOP/s)")
H3_EQUIV_PEAK_TFLOPS = F16_MFMA_PEAK_TFLOPS / 3.0
# a family's own roofline where it is not the f32 matrix pipe
FAMILY_PEAK = {_F16_CONV: F16_MFMA_PEAK_TFLOPS, _X6_GEMM: X6_EQUIV_PEAK_TFLOPS, _H3_GEMM: H3_EQUIV_PEAK_TFLOPS}
FAMILY = {"vocr_gemm_x6": _X6_GEMM, "vocr_gemm_h3": _H3_GEMM, "vocr_gemm_x6_two_views": _X6_GEMM, "vocr_gemm_h3_two_views": _H3_GEMM, "vocr_conv3x3_fwd": "conv3x3 forward + data gradient (conv3x3_wino4 / conv3x3_wino2 kernels: F(4,3) / F(2,3) along the row)",
          "vocr_conv3x3_wino_fwd": "conv3x3 forward + data gradient (conv3x3_wino4 / conv3x3_wino2 kernels: F(4,3) / F(2,3) along the row)",
          "vocr_conv3x3_wgrad": "conv3x3 weight gradient (conv3x3_wgrad_wino2d_kernel: F(3,2) along the row and across row pairs, piece stream)",
          "vocr_conv3x3_wgrad_wino": "conv3x3 weight gradient (conv3x3_wgrad_wino2d_kernel: F(3,2) along the row and across row pairs, piece stream)",
          "vocr_gemm": "dense GEMMs (gemm_dma_kernel / gemm_f32_kernel behind vocr_gemm and vocr_gemm_pair: bridge, LSTM projections, prob, their dX / dW)",
          "vocr_gemm_pair": "dense GEMMs (gemm_dma_kernel / gemm_f32_kernel behind vocr_gemm and vocr_gemm_pair: bridge, LSTM projections, prob, their dX / dW)",
          "vocr_conv3x3_f16_fwd": _F16_CONV, "vocr_conv3x3_wgrad_f16": _F16_CONV, "vocr_conv3x3_h16_fwd": _F16_CONV, "vocr_conv3x3_wgrad_h16": _F16_CONV,
          "vocr_lstm_fwd": "LSTM sweeps (lstm_fwd_chain4w / lstm_bwd_chain4w)", "vocr_lstm_fwd_range": "LSTM sweeps (lstm_fwd_chain4w / lstm_bwd_chain4w)",
          "vocr_lstm_bwd_bias": "LSTM sweeps (lstm_fwd_chain4w / lstm_bwd_chain4w)",
          "vocr_lstm_fwd_packed": "LSTM sweeps (lstm_fwd_chain4w / lstm_bwd_chain4w)", "vocr_lstm_bwd_packed": "LSTM sweeps (lstm_fwd_chain4w / lstm_bwd_chain4w)"}


def ops_x6_on():
    from vistaocr_amd import ops
    return ops.lstm_gemm() != "f32"


def lstm_gemm_mode():
    from vistaocr_amd import ops
    return ops.lstm_gemm()


def gemm_alone(hidden, din=128):
    """The step's large GEMM launches ALONE on the chip (both directions of a BiLSTM layer per launch, random operands): inside the
    step the side-stream launches also wait for CUs that the persistent sweeps hold, so their in-step durations say little about the
    kernel.  With the bf16x6 products on: those (and the split passes that feed them), against the bf16 MFMA peak / 6.  ~0.2 s."""
    import torch
    from vistaocr_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    M, G, H = 294 * B, 4 * hidden, hidden
    x6 = ops_x6_on()
    peak = {"bf16x6": X6_EQUIV_PEAK_TFLOPS, "fp16x3": H3_EQUIV_PEAK_TFLOPS, "f32": F32_MFMA_PEAK_TFLOPS}[lstm_gemm_mode()]

    def timed(fn, n=20):
        for _ in range(8):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    out = []
    for what, mode, ta, tb, m, n, k in (("x-projection, layers 1-2", 0, 0, 1, M, G, 2 * H), ("data gradient, layers 1-2", 1, 0, 0, M, 2 * H, G),
                                        ("weight gradient W_ih, layers 1-2", 0, 1, 0, G, 2 * H, M), ("weight gradient W_hh", 0, 1, 0, G, H, M - B)):
        a0 = torch.randn((k, m) if ta else (m, k), device=dev)
        a1 = torch.randn_like(a0)
        b0 = torch.randn((n, k) if tb else (k, n), device=dev)
        b1 = torch.randn_like(b0)
        c0 = torch.empty(m, n, device=dev)
        c1 = torch.empty(m, n, device=dev) if mode == 0 else None
        rec = {"what": what, "m_n_k": [m, n, k], "products_per_launch": 2}
        if x6:
            # the same two products as ONE bf16x6 launch (or two, for the recurrent weight gradient) from plane sets made outside the timed loop
            if mode == 1:          # c0 = a0 b0 + a1 b1: K runs through both pairs
                pa = ops.x6_planes(a0, m, 2 * k, True, k, x2=a1, seg=k, axis=0)
                pb = ops.x6_planes(b0, n, 2 * k, False, n, x2=b1, seg=k, axis=0)
                fn = lambda: ops.gemm_x6(pa, m, 2 * k, pb, n, 2 * k, m, n, 2 * k, c0, n)
                split = lambda: ops.x6_planes(a0, m, 2 * k, True, k, x2=a1, seg=k, axis=0)
            elif ta:               # weight gradients: both operands K-strided, the two gate planes along the rows
                pa = ops.x6_planes(a0, 2 * m, k, False, m, x2=a1, seg=m, axis=1)
                pb = ops.x6_planes(b0, n, k, False, n)
                k16 = k // 16 * 16
                fn = lambda: ops.gemm_x6(pa, 2 * m, k, pb, n, k, 2 * m, n, k16, c0, n, c1=c1, rsplit=m)
                split = lambda: (ops.x6_planes(a0, 2 * m, k, False, m, x2=a1, seg=m, axis=1), ops.x6_planes(b0, n, k, False, n))
            else:                  # x-projection: one input, the two weight matrices along the rows
                pa = ops.x6_planes(a0, m, k, True, k)
                pb = ops.x6_planes(b0, 2 * n, k, True, k, x2=b1, seg=n, axis=1)
                fn = lambda: ops.gemm_x6(pa, m, k, pb, 2 * n, k, m, 2 * n, k, c0, n, c1=c1, csplit=n)
                split = lambda: ops.x6_planes(a0, m, k, True, k)
            rec["kernel"] = "gemm_x6_kernel"
            rec["split_ms"] = round(timed(split), 4)
        else:
            fn = lambda: ops.gemm_pair(mode, ta, tb, m, n, k, a0, a1, a0.shape[1], b0, b1, b0.shape[1], c0, c1, n)
            rec["kernel"] = "gemm_dma_kernel"
        ms = timed(fn)
        tf = 2 * 2.0 * m * n * k / (ms * 1e-3) / 1e12
        rec.update({"ms": round(ms, 4), "achieved": round(tf, 1), "peak": round(peak, 1), "frac": round(tf / peak, 4)})
        out.append(rec)
        del a0, a1, b0, b1, c0, c1
    return out


# ------------------------------------------------------------------------------------------------ CPU leg (child process)
def cpu_baseline_worker(parity_file, config, budget_s):
    """The oracle (CPU restatement of the same step on PyTorch-CPU).  (1) parity: ONE forward of the parity batch with the closed-form
    weights the GPU side used and the same pool samples (dropout off on both sides) -> loss / greedy labels vs the HIP path's;
    (2) baseline: timed train steps (fwd+CTC+bwd+clamp+Adam) of the bench workload - one step at each thread count of
    CPU_THREAD_SWEEP while the time budget lasts (an estimate from the steps already timed decides whether the next count still fits),
    then a second step at the best count; the best count's mean is reported."""
    import torch
    from oracle import vista_oracle as vo
    from vistaocr_amd.textutils import compute_cer_wer
    t_start = time.time()
    wl = select_workload(config)
    al = alphabet_of(wl)
    vocab = len(al)
    n_cores = os.cpu_count() or 1
    torch.set_num_threads(min(n_cores, 32))
    out = {}
    hp = dict(wl["hp"])
    if parity_file and os.path.exists(parity_file):
        blob = torch.load(parity_file, map_location="cpu", weights_only=True)
        hp = dict(wl["hp"], num_lstm_hidden_units=int(blob["hidden"]))
        sd_np, xp, wp, tgtp, tlp = parity_inputs(int(blob["hidden"]), vocab)
        sd = vo.state_from_numpy(sd_np, requires_grad=False)
        u = parity_samples()
        t0 = time.time()
        with torch.no_grad():
            lo, ln = vo.forward(sd, hp, torch.from_numpy(xp), wp, u, training=True, lstm_training=False)
            loss_o = float(vo.ctc_criterion(lo, torch.from_numpy(tgtp), ln, torch.from_numpy(tlp)))
        strs_o, labels_o = vo.greedy_decode(lo, ln, al.idx_to_char, uxxxx=True)
        T = lo.shape[0]
        valid = torch.arange(T).unsqueeze(1) < torch.as_tensor(ln).to(torch.int64).unsqueeze(0)
        top2 = torch.topk(lo, 2, dim=2)
        gap = (top2.values[:, :, 0] - top2.values[:, :, 1])[valid]
        thr = (top2.values[:, :, 0] - 3.0 / vocab).abs()[valid & (top2.indices[:, :, 0] != 0)]      # the decoder's raw-logit threshold (cnnlstm.py:481,515)
        margin = min(float(gap.min()), float(thr.min()) if thr.numel() else float("inf"))
        loss_h = float(blob["loss"])
        labels_h = [[int(v) for v in row] for row in blob["labels"]]
        strs_h = list(blob["strings"])
        cer = 0.0
        for hyp, ref in zip(strs_h, strs_o):
            c, _ = compute_cer_wer(hyp, ref) if ref.strip() != "" else ((0.0 if hyp.strip() == "" else 1.0), 0.0)
            cer += c / len(strs_o)
        # per-frame argmax agreement on the frames whose oracle decision is at least 1e-3 away from flipping: the label-level bar of the
        # fp16-operand configuration (tests/test_configs_gpu.py holds the same quantity to >= 0.97); 1.0 by construction on the fp32 path
        safe = valid & ((top2.values[:, :, 0] - top2.values[:, :, 1]) > 1e-3)
        agree = float((blob["argmax"].to(torch.int64)[safe] == top2.indices[:, :, 0][safe]).float().mean()) if "argmax" in blob else None
        out["parity"] = dict(loss_rel_err=abs(loss_h - loss_o) / abs(loss_o), label_mismatches=sum(int(a != b) for a, b in zip(labels_h, labels_o)),
                             frame_argmax_agreement_on_safe_frames=agree, safe_frames=int(safe.sum()),
                             lines=len(labels_o), labels_emitted=sum(len(l) for l in labels_o), cer=cer, hip_loss=loss_h, oracle_loss=loss_o,
                             lens_equal=bool(ln.tolist() == list(blob["lens"])), oracle_decode_margin=margin,
                             oracle_forward_s=round(time.time() - t0, 1),
                             what="one forward of the closed-form parity batch of this workload (seed %d) with closed-form weights (recurrent "
                                  "weights +-0.08, output layer widened so the lines emit labels), same pool samples, dropout off on both "
                                  "sides; oracle = PyTorch-CPU restatement (fp32 throughout)" % wl["parity_seed"])
    x, tgt, widths, tl = make_batch(0, vocab)
    state = vo.init_uniform_state(hp, vocab, seed=0)
    opt = torch.optim.Adam([p for _, p in vo.trainable(state)], lr=1e-3)
    u = (torch.rand(B, 64, 2), torch.rand(B, 128, 2))
    # tiny warm-up (thread pools, oneDNN primitive caches) on 2 short lines, not timed
    vo.train_step(state, hp, opt, x[:2, :, :, :120].contiguous(), [120, 120], tgt[:8], torch.tensor([4, 4], dtype=torch.int32),
                  (u[0][:2], u[1][:2]))
    per_thr = {}

    def one_step(n):
        torch.set_num_threads(n)
        t0 = time.time()
        vo.train_step(state, hp, opt, x, widths.tolist(), tgt, tl, u)
        per_thr.setdefault(n, []).append(time.time() - t0)

    counts = [t for t in CPU_THREAD_SWEEP if t <= n_cores] or [n_cores]

    def fits(est):
        return time.time() - t_start + est <= budget_s

    for n in counts[:3]:                                   # the three counts around oneDNN's sweet spot: always
        if per_thr and not fits(1.3 * max(max(v) for v in per_thr.values())):
            break
        one_step(n)
    best = min(per_thr, key=lambda n: min(per_thr[n]))
    if CPU_TIMED_STEPS > 1 and fits(1.2 * min(per_thr[best])):
        one_step(best)                                     # a second step at the best count
    for n in counts[3:]:                                   # the larger counts for the record, if the budget still allows (measured: 2x slower from 64 on)
        if not fits(2.2 * min(per_thr[best])):
            break
        one_step(n)
    best = min(per_thr, key=lambda n: min(per_thr[n]))
    dt = sum(per_thr[best]) / len(per_thr[best])
    out["cpu_baseline"] = dict(value=round(B / dt, 3), unit="line-images/sec", cores=best, host_cores=n_cores, kind="port",
                               seconds_per_step_by_threads={str(n): [round(t, 1) for t in v] for n, v in sorted(per_thr.items())},
                               sample="timed train steps (fwd+CTC+bwd+clamp+Adam) of the same batch-32 workload on the oracle (PyTorch-CPU "
                                      "restatement): one step at each of torch.set_num_threads(n), n in %s, as far as the %d s budget allowed, "
                                      "a second one at the best n = %d (%s s); os.cpu_count() = %d"
                                      % (list(CPU_THREAD_SWEEP), budget_s, best, "/".join("%.1f" % t for t in per_thr[best]), n_cores))
    return out


def cpu_leg(parity_file, config, limit_s=210):
    """Run the CPU leg in a child process with a hard time limit so a slow host can never stall the bench."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", parity_file or "", config, str(int(limit_s * 0.85))],
                           capture_output=True, text=True, timeout=limit_s, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
        for line in reversed(r.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return dict(cpu_baseline=dict(value=None, unit="line-images/sec", cores=0, kind="port", sample="worker failed: " + r.stderr[-300:]))
    except subprocess.TimeoutExpired:
        return dict(cpu_baseline=dict(value=round(B / (limit_s / 2.0), 3), unit="line-images/sec", cores=0,
                                      host_cores=os.cpu_count(), kind="port",
                                      sample="upper bound: parity forward + one step did not finish within %d s" % limit_s))


# ------------------------------------------------------------------------------------------------ self-launch of N ranks
def launch_ranks(args, argv, limit_s=3600):
    """Start one fresh rank process per GPU and supervise them: the first rank that exits non-zero (or the overall time limit) ends
    the others, so a rank that dies in init or in its first collective cannot leave rank 0 waiting in RCCL/gloo."""
    import socket
    import torch
    n = args.gpus
    have = torch.cuda.device_count()          # does not initialise the GPU in this process
    if have < n and not args.share_gpu:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node" % (n, have))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs, logs = [], []
    out0 = tempfile.TemporaryFile(mode="w+")
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        if args.share_gpu:      # two persistent LSTM sweeps from two processes must not compete for one GPU's CUs
            env.setdefault("VOCR_LSTM_SWEEP", "step")
        err = tempfile.TemporaryFile(mode="w+")
        logs.append(err)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL, stderr=err, text=True))
    t0 = time.time()
    failed = None
    while True:
        rcs = [p.poll() for p in procs]
        bad = [i for i, rc in enumerate(rcs) if rc not in (None, 0)]
        if bad:
            failed = "rank %d exited with code %d" % (bad[0], rcs[bad[0]])
        elif all(rc == 0 for rc in rcs):
            break
        elif time.time() - t0 > limit_s:
            failed = "time limit of %d s reached" % limit_s
        if failed:
            for p in procs:                   # our own children, by handle: terminate, then kill what is left
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.kill()
            break
        time.sleep(0.2)
    out0.seek(0)
    text0 = out0.read()
    line = None
    for cand in reversed(text0.strip().splitlines()):
        if cand.startswith("{"):
            line = cand
            break
    if failed or line is None:
        sys.stderr.write(text0[-2000:])
        for i, lg in enumerate(logs):
            lg.seek(0)
            tail = lg.read()[-1500:]
            if tail.strip():
                sys.stderr.write("\n---- rank %d stderr ----\n%s\n" % (i, tail))
        raise SystemExit("bench.py: %s; rank exit codes %s" % (failed or "no result line", [p.poll() for p in procs]))
    sys.stdout.write(line + "\n")
    sys.stdout.flush()


# ------------------------------------------------------------------------------------------------ one rank
def run_rank(args):
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    device_index = 0 if args.share_gpu else local_rank
    torch.cuda.set_device(device_index)
    use_dist = world > 1 or os.environ.get("VOCR_FORCE_DIST") == "1"      # FORCE: exercise RCCL init/all-reduce on one GPU
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend=args.backend)

    import vistaocr_amd as va
    from vistaocr_amd import _lib
    wl = select_workload(args.config)
    conv_dtype = args.conv_dtype or wl["conv_dtype"]
    hp = dict(wl["hp"], num_lstm_hidden_units=args.hidden)
    if conv_dtype != "fp32":
        hp["conv_dtype"] = conv_dtype
    al = alphabet_of(wl)
    torch.manual_seed(0)                                  # same init on every rank (replicas)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    crit = va.CTCLoss()
    # from here on every rank has its OWN randomness: FractionalMaxPool samples (torch.rand per forward) and
    # inter-layer dropout masks (counter-based, keyed by model.dropout_seed) differ across ranks like the data does
    va.seed_rank(model, rank, base=1234)
    x_host, tgt, widths, tl = make_batch(rank, len(al))
    x_host = x_host.pin_memory()

    # ---- parity leg (--full), GPU side (rank 0, N=1): one forward of the closed-form parity batch with closed-form weights, fixed pool
    # samples and dropout off; the CPU oracle (child process) repeats it and compares loss / greedy labels
    parity_file = None
    want_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    if want_cpu:
        init_state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd_np, xp, wp, tgtp, tlp = parity_inputs(args.hidden, len(al))
        psd = model.state_dict()
        for k, v in sd_np.items():
            psd[k] = torch.from_numpy(v)
        model.load_state_dict(psd)
        model.train()
        model.lstm.eval()
        model.pool_samples = list(parity_samples())
        with torch.no_grad():
            lg, lens = model(torch.from_numpy(xp), torch.from_numpy(wp))
            ploss = float(crit(lg, torch.from_numpy(tgtp), lens, torch.from_numpy(tlp)))
            pstr, plabels = va.decoder.greedy_label_sequences(lg, lens, al)
        model.pool_samples = None
        model.load_state_dict(init_state)               # back to the uniform(-0.08, 0.08) init the timed steps start from
        fd, parity_file = tempfile.mkstemp(suffix=".pt", prefix="vocr_parity_")
        os.close(fd)
        torch.save(dict(hidden=args.hidden, loss=ploss, labels=plabels, strings=pstr, lens=lens.tolist(),
                        argmax=lg.argmax(2).to(torch.int16).cpu()), parity_file)
        del init_state, lg, psd
    model.train()
    opt = va.make_optimizer(model, lr=1e-3)          # flat Adam; all-reduce in two buckets, the big one under the CNN backward
    x_dev = x_host.cuda()
    batch_dev = (x_dev, tgt, widths, tl, {})
    batch_host = (x_host, tgt, widths, tl, {})

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    MFMA_NAMES = ["vocr_conv3x3_fwd", "vocr_conv3x3_wino_fwd", "vocr_conv3x3_wgrad", "vocr_conv3x3_wgrad_wino", "vocr_conv3x3_f16_fwd",
                  "vocr_conv3x3_wgrad_f16", "vocr_conv3x3_h16_fwd", "vocr_conv3x3_wgrad_h16", "vocr_gemm", "vocr_gemm_pair", "vocr_gemm_x6", "vocr_gemm_h3", "vocr_gemm_x6_two_views", "vocr_gemm_h3_two_views", "vocr_lstm_fwd", "vocr_lstm_fwd_range", "vocr_lstm_bwd_bias",
                  "vocr_lstm_fwd_packed", "vocr_lstm_bwd_packed"]

    rank_dt = [0.0, 0.0]          # [min, max] over ranks of the last timed loop's wall time

    def timed(batch, steps, event_every=None):
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            if event_every is not None:
                on = bool(event_every) and i % event_every == 0
                _lib.enable_timing(MFMA_NAMES if on else None, keep=True)
                opt.time_comm(on)
            loss = va.train(batch, model, crit, opt)       # the function the reference calls; returns the loss float
        barrier()
        dt = time.perf_counter() - t0
        rank_dt[0] = rank_dt[1] = dt
        if use_dist:
            # the contract's number is the MAX over ranks; the MIN beside it makes a straggler visible in the one line the driver keeps
            tt = torch.tensor([dt, -dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt[0].item())
            rank_dt[0], rank_dt[1] = -float(tt[1].item()), dt
        return dt, loss

    for _ in range(args.warmup):
        va.train(batch_host, model, crit, opt)
    # Python's cyclic garbage collector, not the GPU, made "the first timed loop of a process 2-4 % slower than the second" in rounds
    # 1-2 (20.09 vs 19.18 ms in round 2's driver run): about 20 steps after start-up its first full collection walks every object of
    # the process for 55-75 ms - one step's worth of 4 (scripts/warmup_curve.py: per-step times are flat at 18.45 ms from step 1 with
    # the collector off, with it on step 21 takes 76 ms).  Everything alive now (modules, parameters, the optimiser) is moved out of
    # the collector's sight; garbage created by the steps themselves is still collected.
    import gc
    gc.collect()
    gc.freeze()
    # Timed loops of exactly K steps each, bracketed by barrier + synchronize.  --full times a side number first: the same K steps with
    # the batch resident in HBM.
    if args.full:
        dt_res, _ = timed(batch_dev, args.steps)
        # HIP events, on the stream each kernel is launched on, around every launch of the MFMA kernel families in every `event_every`-th
        # step of the headline loop only (an event pair costs the queue a few microseconds of overlap: ~70 pairs slow that step by a few
        # percent); the full per-entry-point breakdown comes from a separate un-timed pass below
        _lib.enable_timing(MFMA_NAMES)
    # timed region (headline): the batch comes from pinned host memory inside train()
    dt, final_loss = timed(batch_host, args.steps, event_every=args.event_every if args.full else None)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, final_loss)
    ranks_seen = dist.get_world_size() if use_dist else 1
    if args.full:
        timed_recs = {k: list(v) for k, v in _lib.timing_records().items()}
        comm_ms = opt.comm_times_ms()
        sampled_steps = max(1, len(range(0, args.steps, args.event_every)) if args.event_every else 0)
        _lib.enable_timing(None)
        opt.time_comm(False)
        names = MFMA_NAMES + ["vocr_bn_train_stats", "vocr_bn_relu_apply", "vocr_bn_relu_fracpool2x2_fwd", "vocr_bn_train_relu_apply",
                              "vocr_bn_train_relu_fracpool2x2_fwd", "vocr_bn_relu_bwd",
                              "vocr_fracpool2x2_bwd", "vocr_bn_relu_fracpool2x2_bwd", "vocr_ctc_loss_grad", "vocr_clamp_adam", "vocr_bchw_to_wbch", "vocr_wbch_to_bchw",
                              "vocr_relu_maxpool2_fwd", "vocr_relu_maxpool2_bwd", "vocr_gather_rows", "vocr_dropout_fwd", "vocr_mul", "vocr_f32_to_f16_layouts", "vocr_conv3x3_c1_fwd", "vocr_conv3x3_c1_wgrad",
                              "vocr_gemm_x6_split", "vocr_gemm_h3_split"]
        _lib.enable_timing(names)
        for _ in range(PROFILE_STEPS):
            va.train(batch_dev, model, crit, opt)
        torch.cuda.synchronize()
        prof = _lib.timing_records()
        _lib.enable_timing(None)
        # host side of a step: how long the Python + ctypes layer takes to ENQUEUE one step (train_async(): no readback of the loss), measured
        # on an idle queue over 4 steps - far fewer launches than the queue holds, so nothing here waits for the device.  If this number
        # approaches ms_per_step the step is launch-bound and faster kernels buy nothing.
        torch.cuda.synchronize()
        enq = []
        for _ in range(4):
            t_e = time.perf_counter()
            va.train_async(batch_dev, model, crit, opt)
            enq.append(1000.0 * (time.perf_counter() - t_e))
        torch.cuda.synchronize()
        opt.check_health()
        alone = gemm_alone(args.hidden) if rank == 0 and args.hidden == 512 and args.config == "c1" and not args.no_gemm_alone else None

    out = None
    parity_failed = None
    if rank == 0:
        ms = 1000.0 * dt / args.steps
        value = B * world * args.steps / dt
        out = {
            "metric": "line-images/sec (train, batch 32, 30x600 grey)" if args.config == "c1" else
                      "line-images/sec (train, batch 32) - SIDE line for BASELINE %s, not the headline metric" % {"c4": "configs[3]", "c5": "configs[4]"}[args.config],
            "value": round(value, 2), "unit": "line-images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32" if conv_dtype == "fp32" else "f32 with fp16 conv operands (fp32 accumulate)") +
                     {"bf16x6": " (the LSTM's large GEMMs as bf16x6 products: fp32 operands split exactly into three bf16 planes, six bf16 MFMAs per fp32 "
                                "product, fp32 accumulate; VOCR_LSTM_GEMM=f32 restores the f32-MFMA kernels)",
                      "fp16x3": " - OPT-IN MODE, NOT THE HEADLINE CONFIGURATION: the LSTM's large GEMMs as fp16x3 products (VOCR_LSTM_GEMM=fp16x3: operands "
                                "approximated by two fp16 planes with per-row scales, three fp16 MFMAs per product, fp32 accumulate)",
                      "f32": ""}[lstm_gemm_mode()], "data": "synthetic",
            "config": {"workload": wl["what"] + ", 3xBiLSTM-%d, train() = H2D of the batch + fwd+CTC+bwd+allreduce+clamp+Adam, loss returned as a float" % args.hidden,
                       "name": args.config, "widths": "%d .. %d px, mean %.0f" % (min(wl["widths"]), max(wl["widths"]), sum(wl["widths"]) / float(B)),
                       "conv_dtype": conv_dtype,
                       "global_batch": B * world, "parallelism": "dp%d" % world, "ranks_seen": ranks_seen,
                       "backend": (args.backend + ("/RCCL" if args.backend == "nccl" else "")) if use_dist else "none",
                       "final_loss": round(float(final_loss), 3), "per_rank_rng": "seed 1234 + 1000*rank after an identical init"},
            "ms_per_step_ranks": {"min": round(1000.0 * rank_dt[0] / args.steps, 3), "max": round(1000.0 * rank_dt[1] / args.steps, 3),
                                  "what": "slowest and fastest rank's wall time per step over the timed loop (ms_per_step is the max): a gap = a straggler"},
        }
    if rank == 0 and args.full:
        peak = F32_MFMA_PEAK_TFLOPS

        def fam_stats(recs, per_step_div):
            fam = {}
            for name, lst in recs.items():
                if name not in FAMILY or not lst:
                    continue
                f = fam.setdefault(FAMILY[name], dict(ms=0.0, flop=0.0, exe=0.0, n=0))
                for a, e0, e1 in lst:
                    fl = FLOPS_OF[name](a)
                    f["ms"] += e0.elapsed_time(e1)
                    f["flop"] += fl
                    f["exe"] += fl * executed_share(name, a)
                    f["n"] += 1
            outf = {}
            for k, f in fam.items():
                tf = f["flop"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0
                xf = f["exe"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0
                pk = FAMILY_PEAK.get(k, peak)
                outf[k] = dict(ms_per_step=round(f["ms"] / per_step_div, 3), launches_per_step=f["n"] // per_step_div,
                               avg_launch_ms=round(f["ms"] / max(1, f["n"]), 4), launches_timed=f["n"],
                               algorithmic_gflop_per_step=round(f["flop"] / per_step_div / 1e9, 1), peak=pk,
                               achieved=round(tf, 2), frac=round(tf / pk, 4), executed_achieved=round(xf, 2), executed_frac=round(xf / pk, 4))
            return outf

        fams = fam_stats(timed_recs, sampled_steps)
        dom = max(fams.items(), key=lambda kv: kv[1]["ms_per_step"]) if fams else ("none", dict(achieved=0.0, frac=0.0, executed_frac=0.0,
                                                                                               avg_launch_ms=0.0, launches_per_step=0, launches_timed=0))
        # forward-pass launches of the conv kernel alone on the chip (the series rounds 1-2 reported; data-gradient launches run beside
        # the weight-gradient kernel on the side stream, so their wall durations measure the pair)
        fwd_only = [(a, e0, e1) for n_ in ("vocr_conv3x3_fwd", "vocr_conv3x3_wino_fwd") for (a, e0, e1) in timed_recs.get(n_, []) if a[2] is not None]
        cf_ms = sum(e0.elapsed_time(e1) for _, e0, e1 in fwd_only)
        cf_fl = sum(conv_flops(a) for a, _, _ in fwd_only)
        cf_ex = sum(conv_flops(a) * executed_share(n_, a) for n_ in ("vocr_conv3x3_fwd", "vocr_conv3x3_wino_fwd")
                    for (a, _, _) in timed_recs.get(n_, []) if a[2] is not None)
        conv_fwd = dict(achieved=round(cf_fl / (cf_ms * 1e-3) / 1e12, 2) if cf_ms > 0 else 0.0,
                        executed_achieved=round(cf_ex / (cf_ms * 1e-3) / 1e12, 2) if cf_ms > 0 else 0.0,
                        avg_launch_ms=round(cf_ms / max(1, len(fwd_only)), 4), launches_timed=len(fwd_only),
                        what="forward-pass launches of the conv kernels only (nothing else on the chip); achieved = algorithmic direct-convolution "
                             "FLOPs / time, executed = what the kernels issue: 1/2 of them in the F(4,3) launches (>= 64 output channels), 2/3 in the F(2,3) ones")
        conv_fwd["frac"] = round(conv_fwd["achieved"] / peak, 4)
        conv_fwd["executed_frac"] = round(conv_fwd["executed_achieved"] / peak, 4)
        # whole step: algorithmic and executed MFMA FLOPs from the shapes of the calls the step made (un-timed profile pass)
        step_flop = sum(FLOPS_OF[n_](a) for n_ in MFMA_NAMES for a, _, _ in prof.get(n_, [])) / PROFILE_STEPS
        step_exe = sum(FLOPS_OF[n_](a) * executed_share(n_, a) for n_ in MFMA_NAMES for a, _, _ in prof.get(n_, [])) / PROFILE_STEPS
        traffic, traffic_note = None, None
        try:        # HBM-side bytes per launch from the committed PMC passes (cannot be collected live), keyed by kernel family AND tied to
                    # the kernels they were measured on: the file carries the csrc tree hash of that run (vistaocr_amd.build.tree_hash)
            from vistaocr_amd import build as _build
            tj = json.load(open(os.path.join(ROOT, "profiles", "kernel_traffic.json")))
            ent = tj.get(dom[0])
            if args.config != "c1":
                traffic_note = "profiles/kernel_traffic.json was measured on configs[1]; not applicable to this workload"
            elif tj.get("csrc_tree_hash") != _build.tree_hash():
                traffic_note = ("traffic_stale: profiles/kernel_traffic.json was measured on csrc tree %s, this library is %s - rerun scripts/_prof.sh"
                                % (str(tj.get("csrc_tree_hash"))[:12], _build.tree_hash()[:12]))
            elif ent:
                traffic = int((ent["fetch_KB_per_launch"] + ent["write_KB_per_launch"]) * 1024)
        except Exception as e:
            traffic_note = "profiles/kernel_traffic.json unreadable: %s" % e
        breakdown = {}
        for name, lst in prof.items():
            if lst:
                breakdown[name] = round(sum(e0.elapsed_time(e1) for _, e0, e1 in lst) / PROFILE_STEPS, 3)
        out.update({
            "resident_input": {"value": round(B * world * args.steps / dt_res, 2), "ms_per_step": round(1000.0 * dt_res / args.steps, 3),
                               "what": "same K steps with the image batch already in HBM (no H2D inside train()); runs before the headline loop"},
            "allreduce_ms_per_step": comm_ms,
            "host_enqueue_ms_per_step": {"mean": round(sum(enq) / len(enq), 3), "min": round(min(enq), 3), "share_of_step": round(sum(enq) / len(enq) / ms, 3),
                                         "what": "wall time of train_async() (enqueue only, no loss readback) on an idle queue, 4 steps, no profiler"},
            "roofline": {"bound": "mfma",
                         "kernel": dom[0] + " - the kernel family with the most device time in the step (HIP events around every launch of the "
                                            "MFMA families in every %d-th timed step; families overlap on two streams, so their times add up to more "
                                            "than the step, and a side-stream launch's duration includes waiting for CUs that a persistent LSTM sweep holds: "
                                            "gemm_launches_alone has the same launches alone on the chip)" % max(1, args.event_every),
                         "achieved": dom[1]["achieved"], "peak": dom[1].get("peak", peak), "unit": "TFLOP/s", "frac": dom[1]["frac"],
                         "executed_frac": dom[1]["executed_frac"], "traffic": traffic, "traffic_note": traffic_note,
                         "avg_launch_ms": dom[1]["avg_launch_ms"], "launches_per_step": dom[1]["launches_per_step"],
                         "launches_timed": dom[1]["launches_timed"],
                         "dominant_by_time": dom[0], "families_in_step": fams, "conv_forward_alone": conv_fwd,
                         "gemm_launches_alone": alone,
                         "whole_step": {"flop": round(step_flop), "executed_flop": round(step_exe),
                                        "achieved": round(step_flop / (ms * 1e-3) / 1e12, 2), "frac": round(step_flop / (ms * 1e-3) / 1e12 / peak, 4),
                                        "executed_frac": round(step_exe / (ms * 1e-3) / 1e12 / peak, 4),
                                        "what": "algorithmic / executed MFMA FLOPs of one step (from the shapes of the step's own calls) over ms_per_step, against "
                                                "the f32 matrix peak" + ("" if conv_dtype == "fp32" else " - the fp16-operand conv launches of this configuration run on "
                                                "the 16x faster fp16 pipe, so this fraction mixes two rooflines: read families_in_step")}},
            "ms_per_step_by_entry_point": breakdown,
        })
        if want_cpu:
            out.update(cpu_leg(parity_file, args.config))
            par = out.get("parity")
            if par is not None:
                if conv_dtype == "fp32":        # north_star's bar: greedy labels bit-exact, CTC loss within 1e-3
                    bad = par["label_mismatches"] > 0 or par["loss_rel_err"] > 1e-3 or not par["lens_equal"] or par["labels_emitted"] < 10 * B
                else:                           # fp16 conv operands against the fp32 oracle: the loss bar of tests/test_round2_gpu.py (1e-2); labels are reported
                    agree = par.get("frame_argmax_agreement_on_safe_frames")
                    bad = par["loss_rel_err"] > 1e-2 or not par["lens_equal"] or agree is None or agree < 0.97
                    par["what"] += ("; fp16 conv operands against the fp32 oracle: loss held to 1e-2 and the per-frame argmax to >= 0.97 agreement on the "
                                    "frames whose oracle decision is >= 1e-3 from flipping (the bars of tests/test_configs_gpu.py::test_config5_fp16); "
                                    "whole-line label equality is reported (label_mismatches), not required - one flipped near-tie frame changes a line")
                if bad:
                    parity_failed = "parity leg failed: %s" % json.dumps(par)
    if parity_file and os.path.exists(parity_file):
        os.unlink(parity_file)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # the JSON line is the LAST thing on stdout: flush whatever native libraries (RCCL's version banner) still
        # hold in C stdio buffers first
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)
        if parity_failed:
            sys.stderr.write("bench.py: " + parity_failed + "\n")
            sys.exit(3)


def main():
    if "--cpu-baseline-worker" in sys.argv:
        i = sys.argv.index("--cpu-baseline-worker")
        pf = sys.argv[i + 1] if i + 1 < len(sys.argv) else ""
        cfg = sys.argv[i + 2] if i + 2 < len(sys.argv) else "c1"
        budget = int(sys.argv[i + 3]) if i + 3 < len(sys.argv) else 200
        print(json.dumps(cpu_baseline_worker(pf, cfg, budget)))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements and checks: resident-input loop, kernel events and roofline, per-entry-point breakdown, "
                         "host enqueue time, GEMM launches alone, all-reduce times, parity leg against the CPU oracle and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the loss and the model state the last timed step left as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the parity leg and the CPU baseline")
    ap.add_argument("--no-gemm-alone", action="store_true", help="with --full: skip the alone-on-the-chip GEMM launches (profiling passes that average per launch)")
    ap.add_argument("--event-every", type=int, default=10, help="with --full: HIP events around the dominant kernel in every n-th timed step (0: none)")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--config", default="c1", choices=sorted(WORKLOADS),
                    help="c1 = BASELINE configs[1], the headline metric; c4 / c5 = configs[3] / configs[4] as side lines of the same JSON shape")
    ap.add_argument("--conv-dtype", default=None, choices=["fp32", "fp16"],
                    help="fp16 = BASELINE config 5's fp16-operand conv MFMA (fp32 accumulate); default: what the --config names (c1, c4: fp32)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="gloo: plumbing tests on boxes without N GPUs")
    ap.add_argument("--share-gpu", action="store_true", help="all ranks on device 0 (plumbing test of the launcher; needs --backend gloo)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args, sys.argv[1:])
        return
    run_rank(args)


if __name__ == "__main__":
    main()
