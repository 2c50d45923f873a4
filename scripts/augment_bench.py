"""Time the device augmentation (vocr_augment_lines) on configs[1]'s batch (32 x 1 x 30 x 600) and on configs[3]'s ragged widths
(bench.py's c4 workload): device time per call of ops.augment_lines with the tables already on the device, geometry only (one affine
map per line) and the full recipe (mesh, affine, block filter, contrast, invert, noise, delete, stripe on every line); the same recipe
in batched torch on the same GPU (grid_sample and elementwise ops; it lives here, not in the product, draws its noise with torch's
generator, and its output is compared with the kernel's with the per-pixel draws off); the host time of DeviceAugmenter.draw plus
packing; and the train() step of configs[1]'s model with and without DeviceAugmenter.synth_input(stripe=True) in front, in alternating
blocks of one process.  A timed window is HIP events around enough back-to-back calls for about 50 ms.
Output: profiles/r15_augment_bench.txt.

    python scripts/augment_bench.py [--repeats 10] [--out profiles/r15_augment_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.grammar_bench import _stats, _windows, clocks      # noqa: E402


def tables(widths, h, full, seed):
    """AugmentParams with every line augmented: an affine map alone, or every stage."""
    from vistaocr_amd.augment import DeviceAugmenter
    opts = dict(p_rotate=1.0, p_crop_x=1.0, p_crop_y=1.0)
    if full:
        opts.update(p_mesh=1.0, p_filter_rand=1.0, p_contrast=1.0, p_invert=1.0, p_noise=1.0, noise_p=0.3, p_delete=1.0, delete_p=0.05,
                    p_stripe=1.0)
    return DeviceAugmenter(seed=seed, **opts).draw(widths, h, 0)


def on_device(params, dev):
    buf, (o_rec, o_mesh) = params.packed()
    d = torch.from_numpy(buf).to(dev)
    return d[:len(params.widths)], d[o_rec:o_mesh], (d[o_mesh:].view(torch.float32) if params.mesh is not None else None)


class TorchRecipe(object):
    """The stages of include/vocr.h on [B, C, H, Wmax] tensors.  Per-line scalars are [B, 1, 1, 1] device tensors."""

    def __init__(self, params, c, wmax, dev):
        rec = params.records
        f = torch.from_numpy(rec.view(np.float32).copy()).to(dev)
        self.f = [f[:, i].reshape(-1, 1, 1, 1) for i in range(17)]
        self.flags = torch.from_numpy(rec[:, 17].astype(np.int64)).to(dev).reshape(-1, 1, 1, 1)
        self.w = torch.from_numpy(params.widths.astype(np.int64)).to(dev).reshape(-1, 1, 1, 1)
        self.gw = torch.from_numpy(rec[:, 18].astype(np.int64)).to(dev).reshape(-1, 1, 1, 1)
        self.r0 = torch.from_numpy(rec[:, 19].astype(np.int64)).to(dev).reshape(-1, 1, 1, 1)
        self.r1 = torch.from_numpy(rec[:, 20].astype(np.int64)).to(dev).reshape(-1, 1, 1, 1)
        self.mesh = torch.from_numpy(params.mesh).to(dev) if params.mesh is not None else None
        self.gh, self.gw_max, self.h, self.wmax, self.c = params.gh, params.gw_max, params.height, wmax, c
        self.oy = torch.arange(self.h, device=dev, dtype=torch.float32).reshape(1, 1, -1, 1)
        self.ox = torch.arange(wmax, device=dev, dtype=torch.float32).reshape(1, 1, 1, -1)
        self.valid = self.ox < self.w
        self.any_filter = bool((rec[:, 17] & 2).any())

    def run(self, x, draws=True):
        f, wf = self.f, self.w.float()
        px, py = self.ox.expand(x.shape[0], 1, self.h, self.wmax), self.oy.expand(x.shape[0], 1, self.h, self.wmax)
        if self.mesh is not None:
            u, v = px * (self.gw.float() / wf), py * (float(self.gh) / self.h)
            grid = torch.stack([2 * u / self.gw_max - 1, 2 * v / self.gh - 1], dim=-1)[:, 0]
            d = F.grid_sample(self.mesh, grid, mode="bilinear", padding_mode="border", align_corners=True)
            on = (self.flags & 1).bool()
            px, py = px + torch.where(on, d[:, 0:1], 0.0), py + torch.where(on, d[:, 1:2], 0.0)
        xs = torch.minimum(torch.clamp(f[0] * px + f[1] * py + f[2], min=0.0), wf - 1)
        ys = torch.clamp(f[3] * px + f[4] * py + f[5], 0.0, self.h - 1.0)
        grid = torch.stack([2 * xs / max(self.wmax - 1, 1) - 1, 2 * ys / max(self.h - 1, 1) - 1], dim=-1)[:, 0]
        v = F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=True)
        if self.any_filter:
            r = F.pad(torch.where(self.valid, v, 0.0), (1, 0, 1, 0))
            flt = f[10] + f[6] * r[:, :, :-1, :-1] + f[7] * r[:, :, :-1, 1:] + f[8] * r[:, :, 1:, :-1] + f[9] * r[:, :, 1:, 1:]
            mn = torch.where(self.valid, flt, float("inf")).amin(dim=(1, 2, 3), keepdim=True)
            mx = torch.where(self.valid, flt, float("-inf")).amax(dim=(1, 2, 3), keepdim=True)
            den = mx - mn
            v = torch.where((self.flags & 2).bool(), torch.where(den > 0, (flt - mn) / den, 0.0), v)
        v = torch.where(f[11] != 1.0, (v - 0.5) * f[11] + 0.5, v)
        v = torch.where((self.flags & 4).bool(), 1.0 - v, v)
        if draws:
            v = torch.where(torch.rand_like(v) < f[12], v + f[13] * torch.randn_like(v), v)
            v = torch.where(torch.rand_like(v) < f[14], f[15], v)
        oy = self.oy.long()
        v = torch.where((oy >= self.r0) & (oy < self.r1), f[16], v)
        return torch.where(self.valid, v.clamp(0.0, 1.0), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per measurement")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="train() steps per block")
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_augment_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    import bench
    import vistaocr_amd as va
    from vistaocr_amd import ops
    dev = "cuda"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; clocks before: %s" % (torch.cuda.get_device_name(0), clocks()))
    say("vocr_augment_lines.  A timed window: HIP events around n back-to-back calls, n chosen for a window of about 50 ms, ms per call = "
        "window / n; %d windows after %d warm-up calls; median / min / max.  kernel: ops.augment_lines with x, widths and the tables "
        "already on the device (its checks, the output allocation, the launches; no copy, no synchronise inside a window).  torch: the "
        "same stages as grid_sample + elementwise ops on the same tensors, noise from torch's generator.  |diff|: largest difference "
        "of the two outputs with the per-pixel draws off (fp32 both; torch normalises its sampling grid to [-1, 1] and back)." % (args.repeats, args.warmup))
    fmt = "%-31s %-9s | %8s %8s %8s | %8s %8s %8s | %7s | %9s"
    say(fmt % ("batch", "recipe", "kernel", "min", "max", "torch", "min", "max", "ratio", "|diff|"))
    draw_ms = {}
    for name in ("c1", "c4"):
        wl = bench.WORKLOADS[name]
        widths, h = wl["widths"], wl["himg"]
        g = torch.Generator().manual_seed(11)
        x = torch.rand(len(widths), 1, h, max(widths), generator=g)
        for i, w in enumerate(widths):
            x[i, :, :, w:] = 0.0
        xd = x.to(dev)
        label = "%s 32x1x%dx%d%s" % ({"c1": "configs[1]", "c4": "configs[3]"}[name], h, max(widths), "" if name == "c1" else " ragged")
        for full in (False, True):
            params = tables(widths, h, full, 3)
            wd, pd, md = on_device(params, dev)
            run = lambda: ops.augment_lines(xd, wd, pd, md, params.gh, params.gw_max, params.with_filter)
            k = _stats(_windows(run, args.warmup, args.repeats))
            tr = TorchRecipe(params, 1, max(widths), dev)
            t = _stats(_windows(lambda: tr.run(xd), args.warmup, args.repeats))
            quiet = params.records.copy()
            quiet[:, 12] = quiet[:, 14] = 0
            qd = torch.from_numpy(quiet.view(np.int32).reshape(-1)).to(dev)
            yk = ops.augment_lines(xd, wd, qd, md, params.gh, params.gw_max, params.with_filter)
            diff = float((yk - tr.run(xd, draws=False)).abs().max())
            say(fmt % (label, "full" if full else "geometry", "%.4f" % k[0], "%.4f" % k[1], "%.4f" % k[2], "%.4f" % t[0], "%.4f" % t[1],
                       "%.4f" % t[2], "%.1fx" % (t[0] / k[0]), "%.2g" % diff))
        for what, aug in (("synth_input(stripe=True)", va.DeviceAugmenter.synth_input(stripe=True, seed=1)),
                          ("every stage on", None)):
            reps = 200
            t0 = time.perf_counter()
            for s in range(reps):
                p = aug.draw(widths, h, s) if aug is not None else tables(widths, h, True, s)
                p.packed()
            draw_ms[(name, what)] = (time.perf_counter() - t0) / reps * 1e3
    say("")
    say("widths of configs[3]'s batch: %d .. %d" % (max(bench.WORKLOADS["c4"]["widths"]), min(bench.WORKLOADS["c4"]["widths"])))
    for (name, what), ms in draw_ms.items():
        say("host, %s, %s: DeviceAugmenter.draw + AugmentParams.packed (pure numpy, one thread%s): %.3f ms per batch (mean of 200)"
            % ({"c1": "configs[1]", "c4": "configs[3]"}[name], what, "" if what.startswith("synth") else "; includes building the augmenter", ms))

    # the train() step of configs[1]'s model, host clock around blocks of steps that end in a synchronise
    wl = bench.select_workload("c1")
    al = bench.alphabet_of(wl)
    torch.manual_seed(0)
    model = va.CnnOcrModel(alphabet=al, verbose=False, **wl["hp"])
    model.train()
    opt = va.make_optimizer(model, lr=1e-3)
    crit = va.CTCLoss()
    x, tgt, widths, tl = bench.make_batch(0, len(al))
    batch = (x.pin_memory(), tgt, widths, tl, {})
    aug = va.DeviceAugmenter.synth_input(stripe=True, seed=1)

    def block(augmented, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            va.train(aug(batch) if augmented else batch, model, crit, opt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    block(False, 10), block(True, 10)
    res = {False: [], True: []}
    for _ in range(args.blocks):
        for augmented in (False, True):
            res[augmented].append(block(augmented, args.steps))
    say("")
    say("train() of configs[1]'s model (bench.py's c1 workload: the batch in pinned host memory, copied to the device every step), host "
        "clock over blocks of %d steps ending in a synchronise, %d alternating blocks each after 10 warm-up steps; ms per step, median "
        "(all blocks):" % (args.steps, args.blocks))
    say("  plain                                   %.3f  (%s)" % (float(np.median(res[False])), " ".join("%.3f" % v for v in res[False])))
    say("  DeviceAugmenter.synth_input(stripe=True) %.3f  (%s)" % (float(np.median(res[True])), " ".join("%.3f" % v for v in res[True])))
    params = aug.draw(widths, 30, 0)
    wd, pd, md = on_device(params, dev)
    xd = x.to(dev)
    k = _stats(_windows(lambda: ops.augment_lines(xd, wd, pd, md, params.gh, params.gw_max, params.with_filter), args.warmup, args.repeats))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100):
        aug.apply(xd, widths, params)
    e1.record()
    e1.synchronize()
    say("  the preset's tables on this batch: ops.augment_lines %.4f ms per call on the device (min %.4f, max %.4f); "
        "DeviceAugmenter.apply, which adds the packed upload of the tables, %.4f ms per call between HIP events (100 back-to-back calls)"
        % (k[0], k[1], k[2], e0.elapsed_time(e1) / 100))
    say("clocks after: %s" % clocks())
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
