"""GPU: round-2 parity and drop-in cases.

  * BASELINE configs[1] at FULL size (B=32, 30x600, 3xBiLSTM-512, V=96) against the on-box oracle, explicit pool samples and
    explicit inter-layer dropout masks, batch seed chosen on the oracle side for a decode margin >= 1e-3: lens, CTC loss 1e-3, greedy
    labels bit-exact (unconditional), every gradient tensor element-wise to 1e-2;
  * the reference's decode edge-case fixture through every decode entry point of the HIP path;
  * config 5 at its full line size 60x1200 (fp16 conv operands) with the measured agreement printed;
  * CTC on an infeasible alignment; determinism of the weight gradients; train() with torch.optim.Adam;
  * the RCCL exchange inside a real backward (nccl, world_size 1) == the plain run, bit for bit;
  * fit() (validate cadence, plateau -> LR drop -> reload best) on the HIP path; a reference-written checkpoint;
  * the C-ABI all-reduce; bench.py's own N-rank launcher."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import closed_form as cf
from oracle import vista_oracle as vo
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_state(model, sd_np):
    sd = model.state_dict()
    for k, v in sd_np.items():
        sd[k] = torch.from_numpy(v)
    model.load_state_dict(sd)


FULL_SIZE_SEED = 73          # scripts/margin_search.py 2.0 1.0 1 140: oracle decode margin 1.17e-3 with this batch


def test_config1_full_size_vs_oracle():
    """B=32 x 1x30x600, V=96, lstm_input_dim 128, 3xBiLSTM-512 with dropout masks: the bench workload, pinned to the oracle.
    The batch seed is chosen on the ORACLE side so that no valid frame's greedy decision is closer than 1e-3 to flipping (the way
    oracle/gen_golden.py picks its batches); with that, the label sequences are compared bit for bit UNCONDITIONALLY, and every
    gradient tensor element-wise."""
    import vistaocr_amd as va
    from tests import parity_util as pu
    chars = gu.alphabet_chars("english")
    V = len(chars)
    hp = dict(input_line_height=30, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3, num_lstm_hidden_units=512,
              p_lstm_dropout=0.5, num_in_channels=1)
    # recurrent weights from the reference's own init range (+-0.08, cnnlstm.py:158-159): the 0.3-scaled closed form
    # saturates a 512-unit LSTM, which turns fp32 summation-order noise into O(1e-3) logit differences
    sd_np = cf.closed_form_state(hp, V, lstm_scale=0.08, prob_scale=2.0)
    B, T, H = 32, 294, 512
    r = np.random.RandomState(121)
    s1 = torch.from_numpy(r.uniform(0, 0.999, size=(B, 64, 2)).astype(np.float32))
    s2 = torch.from_numpy(r.uniform(0, 0.999, size=(B, 128, 2)).astype(np.float32))
    masks = [torch.from_numpy((r.uniform(size=(T, B, 2 * H)) >= 0.5).astype(np.float32) * 2.0) for _ in range(2)]
    al = va.Alphabet(chars, left_to_right=True)
    torch.set_num_threads(min(32, os.cpu_count() or 1))

    def oracle_logits(seed):
        xs, ws, _, _ = cf.closed_form_batch(B, 1, 30, [600] * B, V, [20] * B, seed=seed)
        with torch.no_grad():
            lo_, ln_ = vo.forward(vo.state_from_numpy(sd_np, requires_grad=False), hp, torch.from_numpy(xs), ws, (s1, s2),
                                  training=True, dropout_masks=masks)
        return lo_, ln_, V

    seed, margin, _ = pu.pick_seed(oracle_logits, FULL_SIZE_SEED, want=1e-3)
    x, w, tgt, tl = cf.closed_form_batch(B, 1, 30, [600] * B, V, [20] * B, seed=seed)

    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    _load_state(model, sd_np)
    model.train()
    model.pool_samples = [s1, s2]
    model.dropout_masks = masks
    logits, lens = model(torch.from_numpy(x), torch.from_numpy(w))
    loss = va.CTCLoss()(logits, torch.from_numpy(tgt), lens, torch.from_numpy(tl))
    loss.backward()
    labels = model.decode_labels(logits, lens)

    osd = vo.state_from_numpy(sd_np)
    lo, ln = vo.forward(osd, hp, torch.from_numpy(x), w, (s1, s2), training=True, dropout_masks=masks)
    lo_loss = vo.ctc_criterion(lo, torch.from_numpy(tgt), ln, torch.from_numpy(tl))
    lo_loss.backward()
    assert tuple(logits.shape) == (T, B, V) and lens.tolist() == ln.tolist() == [T] * B
    rel = abs(float(loss.detach()) - float(lo_loss.detach())) / abs(float(lo_loss.detach()))
    lg = logits.detach().cpu()
    err = float((lg - lo.detach()).abs().max())
    olabels = vo.greedy_decode(lo.detach(), ln, al.idx_to_char, uxxxx=True)[1]
    mism = sum(int(a != b) for a, b in zip(labels, olabels))
    emitted = sum(len(l) for l in olabels)
    print("full-size configs[1] (batch seed %d): loss %.4f vs oracle %.4f (rel %.2e); max |dlogit| %.2e at scale %.1f; oracle decode "
          "margin %.2e; labels emitted %d; label sequences differing: %d of %d"
          % (seed, float(loss.detach()), float(lo_loss.detach()), rel, err, float(lo.detach().abs().max()), margin, emitted, mism, B))
    assert rel <= 1e-3
    assert emitted >= 10 * B, "the label comparison would be vacuous"
    assert err <= margin / 4, "logit error %.2e is not small against the decode margin %.2e" % (err, margin)
    assert mism == 0, "greedy label sequences differ"
    assert labels == olabels
    worst = pu.assert_grads_close(model, osd)
    print("full-size configs[1]: worst per-tensor element-wise gradient error %.2e (%s)" % (worst[1], worst[0]))


def test_reference_decode_edge_cases_on_the_hip_decoder():
    """tests/golden/decode_edges.npz (written by the reference's decode_without_lm / ArgmaxDecoder): threshold 3/96 straddle,
    first-max ties, the duplicated 'u002d' entries 73/91, frames past lens, a label on the last frame."""
    import vistaocr_amd as va
    from vistaocr_amd.decoder import greedy_labels_device
    g = gu.load("decode_edges")
    al = va.Alphabet(gu.alphabet_chars("english"), left_to_right=True)
    logits = torch.from_numpy(g["logits"]).cuda()
    lens = torch.from_numpy(g["lens"])
    want_ux = [str(s) for s in g["strings_uxxxx"]]
    want_u8 = [str(s) for s in g["strings_utf8"]]
    want_labels = gu.split_labels(g)
    hp = dict(input_line_height=30, rds_line_height=30, lstm_input_dim=16, num_lstm_layers=1, num_lstm_hidden_units=16, p_lstm_dropout=0.0)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    assert model.decode_labels(logits, lens) == want_labels
    assert model.decode_without_lm(logits, lens, uxxxx=True) == want_ux
    assert model.decode_without_lm(logits, lens, uxxxx=False) == want_u8
    assert va.ArgmaxDecoder(al).decode(logits, lens, uxxxx=True) == want_ux
    assert greedy_labels_device(logits, lens, al) == want_labels


def test_config5_full_line_size_60x1200_fp16_conv():
    """Config 5 at the size BASELINE.json names (60-px lines ~1200 px wide, rapid_ds to 30, 512-hidden BiLSTM, fp16 conv MFMA
    operands, fp32 CTC).  fp16 rounding is a discontinuity, so the bar is the one SURVEY.md §7 sets for this config."""
    import vistaocr_amd as va
    chars = gu.alphabet_chars("english")
    V = len(chars)
    hp = dict(input_line_height=60, rds_line_height=30, lstm_input_dim=128, num_lstm_layers=3, num_lstm_hidden_units=512,
              p_lstm_dropout=0.5, num_in_channels=1, conv_dtype="fp16")
    sd_np = cf.closed_form_state(hp, V, lstm_scale=0.08, prob_scale=0.5)
    B, widths = 2, [1200, 1117]
    x, w, tgt, tl = cf.closed_form_batch(B, 1, 60, widths, V, [40, 35], seed=13)
    r = np.random.RandomState(113)
    s1 = torch.from_numpy(r.uniform(0, 0.999, size=(B, 64, 2)).astype(np.float32))
    s2 = torch.from_numpy(r.uniform(0, 0.999, size=(B, 128, 2)).astype(np.float32))
    al = va.Alphabet(chars, left_to_right=True)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    _load_state(model, sd_np)
    model.train()
    model.lstm.eval()
    model.pool_samples = [s1, s2]
    logits, lens = model(torch.from_numpy(x), torch.from_numpy(w))
    loss = va.CTCLoss()(logits, torch.from_numpy(tgt), lens, torch.from_numpy(tl))
    osd = vo.state_from_numpy(sd_np, requires_grad=False)
    with torch.no_grad():
        lo, ln = vo.forward(osd, hp, torch.from_numpy(x), w, (s1, s2), training=True, lstm_training=False)
        lo_loss = vo.ctc_criterion(lo, torch.from_numpy(tgt), ln, torch.from_numpy(tl))
    assert lens.tolist() == ln.tolist() == [294, 273]      # 60 -> 30 halves the width first: T(1200) = T30(600)
    rel = abs(float(loss.detach()) - float(lo_loss.detach())) / abs(float(lo_loss.detach()))
    lg = logits.detach().cpu()
    T = lg.shape[0]
    valid = torch.arange(T).unsqueeze(1) < ln.unsqueeze(0)
    top2 = torch.sort(lo, dim=2, descending=True)[0]
    safe = valid & ((top2[:, :, 0] - top2[:, :, 1]) > 1e-3)
    agree = float((lg.argmax(2)[safe] == lo.argmax(2)[safe]).float().mean())
    print("config 5 at 60x1200 (fp16 conv operands): loss rel err %.2e, max |dlogit| %.2e, per-frame label agreement %.4f on %d frames"
          % (rel, float((lg - lo).abs()[valid].max()), agree, int(safe.sum())))
    assert rel <= 1e-2 and agree >= 0.97


def test_ctc_infeasible_alignment_is_inf_like_the_cpu_criterion():
    """T < L + repeats: no alignment exists.  F.ctc_loss(zero_infinity=False) — the criterion this build is pinned to
    (warp-ctc is absent and unpinned) — returns +inf for that sample; so does ctc.hip.  The other samples of
    the batch are unaffected: their gradient rows equal the ones computed without the infeasible neighbour."""
    import vistaocr_amd as va
    T, B, V = 6, 3, 12
    g = torch.Generator().manual_seed(5)
    logits = (torch.rand(T, B, V, generator=g) - 0.5) * 4
    tgt = torch.tensor([1, 2, 3, 4,      5, 5, 5, 5,      7, 8], dtype=torch.int32)       # sample 1: 4 repeats need 7 frames
    tl = torch.tensor([4, 4, 2], dtype=torch.int32)
    lens = torch.tensor([6, 6, 5], dtype=torch.int32)
    crit = va.CTCLoss()
    lg = logits.cuda().requires_grad_(True)
    loss = crit(lg, tgt, lens, tl)
    ref = vo.ctc_criterion(logits, tgt, lens, tl)
    assert torch.isinf(ref).all() and torch.isinf(loss).all() and float(loss.detach()) > 0
    for b in (0, 2):
        li = crit(logits[:, b:b + 1].contiguous().cuda(), tgt[[0, 4, 8][b]:[4, 8, 10][b]], lens[b:b + 1], tl[b:b + 1])
        ri = vo.ctc_criterion(logits[:, b:b + 1], tgt[[0, 4, 8][b]:[4, 8, 10][b]], lens[b:b + 1], tl[b:b + 1])
        assert abs(float(li) - float(ri)) <= 1e-5 * abs(float(ri))
    loss.backward()
    alone = logits[:, 0:1].contiguous().cuda().requires_grad_(True)
    crit(alone, tgt[:4], lens[:1], tl[:1]).backward()
    assert torch.equal(lg.grad[:, 0], alone.grad[:, 0]), "a feasible sample's gradient must not depend on its neighbours"
    assert torch.isfinite(lg.grad[:, 0]).all() and torch.isfinite(lg.grad[:, 2]).all()


def _small_setup(H=64, B=6, seed=3, layers=2):
    import vistaocr_amd as va
    chars = gu.alphabet_chars("english")
    V = len(chars)
    hp = dict(input_line_height=30, rds_line_height=30, lstm_input_dim=64, num_lstm_layers=layers, num_lstm_hidden_units=H,
              p_lstm_dropout=0.5, num_in_channels=1)
    sd_np = cf.closed_form_state(hp, V)
    widths = sorted([300 - (230 // B) * i for i in range(B)], reverse=True)
    x, w, tgt, tl = cf.closed_form_batch(B, 1, 30, widths, V, [8 - (i % 3) for i in range(B)], seed=seed)
    s1, s2 = cf.closed_form_pool_samples(B)
    al = va.Alphabet(chars, left_to_right=True)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    _load_state(model, sd_np)
    model.train()
    model.pool_samples = [torch.from_numpy(s1), torch.from_numpy(s2)]
    batch = (torch.from_numpy(x), torch.from_numpy(tgt), torch.from_numpy(w), torch.from_numpy(tl), {})
    return va, model, batch


@pytest.mark.parametrize("H,B", [(64, 6), (512, 32)])
def test_weight_gradients_are_bitwise_reproducible(H, B):
    """Two identical forward/backward passes from the same state -> identical flat gradient (split-K slabs, column sums,
    conv weight-gradient slabs and the LSTM bias sums all combine in a fixed order; no float atomics across workgroups)."""
    va, model, batch = _small_setup(H=H, B=B)
    opt = va.make_optimizer(model)
    crit = va.CTCLoss()
    grads = []
    for _ in range(2):
        model._dropout_calls = 0                  # same dropout mask both times
        opt.zero_grad()
        logits, lens = model(batch[0], batch[2])
        crit(logits, batch[1], lens, batch[3]).backward()
        opt.all_reduce_grads()                    # joins the side stream
        torch.cuda.synchronize()
        grads.append(opt.flat_g.clone())
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1]), "max |diff| %.3e" % float((grads[0] - grads[1]).abs().max())


def test_second_backward_without_zero_grad_is_refused():
    va, model, batch = _small_setup()
    opt = va.make_optimizer(model)
    crit = va.CTCLoss()
    opt.zero_grad()
    for i in range(2):
        logits, lens = model(batch[0], batch[2])
        loss = crit(logits, batch[1], lens, batch[3])
        if i == 0:
            loss.backward()
        else:
            with pytest.raises(RuntimeError, match="second backward"):
                loss.backward()
    opt.all_reduce_grads()
    torch.cuda.synchronize()


def test_train_accepts_torch_optim_adam_like_the_reference():
    """src/train_cnn_lstm.py:363 hands train() a torch.optim.Adam.  Same two steps through (a) torch.optim.Adam with the
    device clamp and (b) the fused FlatClampAdam: same losses, same weights (Adam arithmetic to 1e-6), and the two models
    live in one process without touching each other's gradients."""
    va, model_a, batch = _small_setup(seed=4)
    _, model_b, _ = _small_setup(seed=4)
    opt_a = torch.optim.Adam(model_a.parameters(), lr=1e-3)
    opt_b = va.make_optimizer(model_b, lr=1e-3)
    crit = va.CTCLoss()
    for step in range(2):
        s1, s2 = cf.closed_form_pool_samples(batch[0].shape[0], seed=5 + step)
        for m in (model_a, model_b):
            m.pool_samples = [torch.from_numpy(s1), torch.from_numpy(s2)]
            m._dropout_calls = 10 * step
        la = va.train(batch, model_a, crit, opt_a)
        lb = va.train(batch, model_b, crit, opt_b)
        assert isinstance(la, float) and abs(la - lb) <= 1e-5 * abs(lb), (step, la, lb)
        if step == 0:
            # same weights, same kernels -> bit-identical gradients; what is compared here is the Adam arithmetic alone
            for (k, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
                assert float((pa.detach() - pb.detach()).abs().max()) <= 1e-6, k
    # after the second step the 1e-9 differences of the first have gone through a forward/backward: an element whose gradient is a
    # small difference of large sums (or pure rounding noise: conv biases in front of a batch-stat BN) may move differently
    n_bad = n_tot = 0
    for (k, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        d = (pa.detach() - pb.detach()).abs()
        n_tot += d.numel()
        n_bad += int((d > 2e-6).sum())
        assert float(d.max()) <= 4.1e-3, k
    assert n_bad <= 5e-2 * n_tot, (n_bad, n_tot)
    # gradients of model_a were clamped in place on the device
    assert max(float(p.grad.abs().max()) for p in model_a.parameters()) <= 5.0


def test_nan_gradient_is_not_hidden_by_the_clamp():
    """torch's clamp_ propagates NaN; fminf/fmaxf would turn it into a finite +-5 update."""
    from vistaocr_amd import ops
    g = torch.tensor([float("nan"), 7.0, -9.0, 0.5], device="cuda")
    ops.clamp_(g, 5.0)
    assert torch.isnan(g[0]) and g[1:].tolist() == [5.0, -5.0, 0.5]
    h = ops.health(g.device)
    assert int(h[1]) == 1
    p = torch.zeros(4, device="cuda")
    m = torch.zeros(4, device="cuda")
    v = torch.zeros(4, device="cuda")
    ops.clamp_adam(p, torch.tensor([float("nan"), 1.0, -1.0, 0.0], device="cuda"), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, 1.0, 1)
    assert torch.isnan(p[0]) and torch.isfinite(p[1:]).all()
    with pytest.raises(RuntimeError, match="NaN gradient"):
        ops.check_health(h.cpu().tolist())
    h.zero_()


_DIST_CODE = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
use_dist = sys.argv[2] == "1"
if use_dist:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[3], RANK="0", WORLD_SIZE="1", VOCR_FORCE_DIST="1",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", device_id=torch.device("cuda", 0))
from tests.test_round2_gpu import _small_setup
from oracle import closed_form as cf
va, model, batch = _small_setup(H=64, B=6, seed=9)
opt = va.make_optimizer(model)
fired = []
model._vocr_hooks["sequence_grads_ready"].append(lambda: fired.append(opt._tail_work is not None))
crit = va.CTCLoss()
losses = []
for step in range(2):
    s1, s2 = cf.closed_form_pool_samples(6, seed=5 + step)
    model.pool_samples = [torch.from_numpy(s1), torch.from_numpy(s2)]
    losses.append(va.train(batch, model, crit, opt))
torch.cuda.synchronize()
torch.save(dict(p=opt.flat_p.cpu(), m=opt.exp_avg.cpu(), losses=losses, fired=fired, split=opt._split), sys.argv[1])
if use_dist:
    dist.destroy_process_group()
"""


def test_rccl_two_bucket_exchange_inside_a_real_backward(tmp_path):
    """make_optimizer's two-bucket all-reduce (big bucket launched from the backward hook, joined with the side stream) over
    RCCL (backend nccl, world_size 1, VOCR_FORCE_DIST=1), two train() steps: bit-identical to the run without a process group."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    outs = []
    for use_dist in ("0", "1"):
        f = os.path.join(tmp_path, "r%s.pt" % use_dist)
        r = subprocess.run([sys.executable, "-c", _DIST_CODE % ROOT, f, use_dist, str(port)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(f))
    a, b = outs
    assert b["fired"] == [True, True] and a["fired"] == [False, False] and b["split"] > 0
    assert a["losses"] == b["losses"]
    assert torch.equal(a["p"], b["p"]) and torch.equal(a["m"], b["m"])


def test_fit_on_the_hip_path(tmp_path):
    """The loop of src/train_cnn_lstm.py:375-470 with the real train()/test_on_val(): GroupedSampler + SortByWidthCollater
    batches, validation + snapshot every 2 iterations, patience 0 so the plateau schedule drops the LR and the best snapshot is
    reloaded; ends when the schedule is exhausted."""
    import vistaocr_amd as va
    from vistaocr_amd import checkpoint
    from vistaocr_amd.loop import GroupedSampler, SortByWidthCollater, fit
    al = va.english_alphabet()
    hp = dict(input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1, num_lstm_hidden_units=32,
              p_lstm_dropout=0.0, num_in_channels=1)
    torch.manual_seed(3)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    r = np.random.RandomState(0)
    widths = [120, 96, 150, 64, 200, 180]

    class DS(torch.utils.data.Dataset):
        size_group_keys = [150, 300]
        size_groups = {150: [0, 1, 2, 3], 300: [4, 5]}
        items = [(torch.from_numpy(r.uniform(0, 1, size=(1, 30, w)).astype(np.float32)), [int(v) for v in r.randint(1, 96, size=4)],
                  {"width": w, "utt-id": "u%d" % i}) for i, w in enumerate(widths)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]
    ds = DS()
    torch.manual_seed(11)
    train_loader = torch.utils.data.DataLoader(ds, batch_size=2, sampler=GroupedSampler(ds, rand=True), collate_fn=SortByWidthCollater)
    val_loader = [SortByWidthCollater([ds[i] for i in (0, 1, 2)]), SortByWidthCollater([ds[i] for i in (3, 4, 5)])]
    opt = va.make_optimizer(model, lr=1e-3)
    seen = []

    def validate(loader, m, crit):
        from vistaocr_amd.loop import test_on_val
        torch.manual_seed(7)                                   # FractionalMaxPool draws samples in eval too
        loss, cer, wer = test_on_val(loader, m, crit)
        seen.append((loss, cer, wer, float(next(m.parameters()).detach().flatten()[0])))
        # a metric that improves once and then plateaus, so that with patience 0 the second non-improving validation
        # lowers the LR (the real CER/WER of an untrained model is ~1.0 throughout)
        fake = [0.9, 0.8, 0.85, 0.86, 0.87, 0.88, 0.89, 0.90, 0.91, 0.92][len(seen) - 1]
        return loss, cer, fake
    prefix = os.path.join(tmp_path, "hip")
    hist = fit(model, va.CTCLoss(), opt, train_loader, val_loader, va.train, prefix, batch_size=2, n_epochs=20,
               snapshot_every_n_iterations=2, patience=0, min_lr=1e-5, validate_fn=validate)
    assert all(np.isfinite(l) and l > 0 for l in hist["loss"]) and all(np.isfinite(s[0]) and 0 <= s[1] for s in seen)
    assert [v[0] for v in hist["val"]][:4] == [2, 4, 6, 8]
    assert hist["lr_drops"][:2] == [6, 8] and hist["stopped_early"]            # patience 0: drop at the 3rd, 4th ... validation
    assert abs(opt.param_groups[0]["lr"] - 1e-5) < 1e-12
    best = checkpoint.load(prefix + "-best_model.pth")
    assert best["iteration"] == 4 and abs(best["val_wer"] - 0.8) < 1e-12
    # "reload best" after the drop at iteration 6: the weights validated at iteration 8 descend from the iteration-4 snapshot
    # (two more train steps), not from the iteration-6 weights: check via a fresh replay
    m2 = va.CnnOcrModel.FromSavedWeights(prefix + "-best_model.pth", verbose=False)
    for k, v in m2.state_dict().items():
        assert torch.equal(v.cpu(), checkpoint.strip_dataparallel_prefix(best["state_dict"])[k]), k
    cur = checkpoint.load(prefix + "-cur_snapshot.pth")
    assert cur["iteration"] == hist["val"][-1][0] and set(cur) == set(best)


def test_reference_written_checkpoint_runs_on_the_gpu(tmp_path):
    """tests/golden/ref_checkpoint.pth.gz (written by the reference's classes): FromSavedWeights -> forward -> same greedy
    strings and logits as the reference model produced."""
    import gzip
    import vistaocr_amd as va
    path = os.path.join(tmp_path, "ref-best_model.pth")
    with gzip.open(os.path.join(gu.GOLDEN, "ref_checkpoint.pth.gz"), "rb") as src, open(path, "wb") as dst:
        dst.write(src.read())
    exp = gu.load("ref_checkpoint_expect")
    model = va.CnnOcrModel.FromSavedWeights(path, verbose=False)
    assert next(model.parameters()).is_cuda
    V = len(model.alphabet)
    B = len(exp["widths"])
    x, w, _, _ = cf.closed_form_batch(B, 1, 30, [int(v) for v in exp["widths"]], V, [4, 3], seed=int(exp["batch_seed"]))
    s1, s2 = cf.closed_form_pool_samples(B)
    model.eval()
    model.pool_samples = [torch.from_numpy(s1), torch.from_numpy(s2)]
    with torch.no_grad():
        logits, lens = model(torch.from_numpy(x), torch.from_numpy(w))
    assert lens.tolist() == exp["lens"].tolist()
    assert float((logits.cpu() - torch.from_numpy(exp["logits"])).abs().max()) < 2e-3
    assert model.decode_without_lm(logits, lens, uxxxx=True) == [str(s) for s in exp["strings_uxxxx"]]


def test_c_abi_allreduce_over_rccl_single_rank():
    """vocr_comm_* / vocr_allreduce_sum_f32 (include/vocr.h): the thin RCCL wrapper a non-torch host uses for the one exchange
    step.  One rank: the sum over ranks is the buffer itself; exercises dlopen, unique id, communicator and a stream-ordered call."""
    import ctypes
    from vistaocr_amd import _lib
    lib = _lib.load()
    uid = ctypes.create_string_buffer(128)
    _lib.check(lib.vocr_comm_unique_id(uid), "vocr_comm_unique_id")
    comm = ctypes.c_void_p()
    _lib.check(lib.vocr_comm_create(ctypes.byref(comm), uid, 1, 0, 0), "vocr_comm_create")
    buf = torch.arange(1 << 20, dtype=torch.float32, device="cuda")
    want = buf.clone()
    _lib.check(lib.vocr_allreduce_sum_f32(comm, buf.data_ptr(), buf.numel(), torch.cuda.current_stream().cuda_stream), "vocr_allreduce_sum_f32")
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    _lib.check(lib.vocr_comm_destroy(comm), "vocr_comm_destroy")
    assert lib.vocr_allreduce_sum_f32(None, None, 4, None) == -1


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the parent spawns two rank processes (here on ONE GPU, gloo
    backend, per-step LSTM launches: a plumbing test of the launcher, the env contract, the two-bucket exchange inside the
    backward and the single JSON line)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--backend", "gloo",
                        "--share-gpu", "--hidden", "256"], capture_output=True, text=True, timeout=900,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["ranks_seen"] == 2 and out["config"]["global_batch"] == 64 and out["scaling"] == "weak"
    assert out["value"] > 0 and "roofline" in out and "cpu_baseline" not in out


def test_bench_plain_run_is_the_headline_only(tmp_path):
    """`python bench.py` without --full: one timed loop of --steps steps and the headline fields, none of the side legs; --dump-outputs
    writes the loss of the last timed step (the one the line's final_loss rounds) and the model state beside it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    out = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert all(k in out for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"))
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert not {"resident_input", "roofline", "parity", "cpu_baseline", "allreduce_ms_per_step", "ms_per_step_by_entry_point"} & set(out)
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and round(float(loss[0]), 3) == out["config"]["final_loss"]
    assert np.isfinite(np.load(tmp_path / "prob_layer.0.weight.npy")).all()
