"""What device-side gradient norms cost the training step.  ONE process, alternating rounds, the benchmark's training geometry (C2, B = 128, bf16,
two-pass optimizer): the step with clip=None (the path without GradClip) against GradClip() (measure only: the per-tensor log) and
GradClip(max_norm=1.0), each with FusedAdamW.step(overlap=False) and overlap=True.  Device events around BLOCK steps, ROUNDS blocks per variant;
min and median of the blocks' ms per step.  Never imported by the package or by bench.py.

    python scripts/grad_clip_probe.py > profiles/grad_clip.txt"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd.optim import FusedAdamW, GradClip  # noqa: E402
from mode_diffusion_policy_amd.utils import rand_log_logistic  # noqa: E402

BLOCK, ROUNDS, WARM = 50, 3, 3
dev = torch.device("cuda:0")
_, den = bench.build_model(dev, "bf16"); m = den.inner_model; den.train()
B = 128
g = torch.Generator().manual_seed(1)
img = torch.randn(B, 2, 2048, generator=g).to(dev); goal = torch.randn(B, 1, 512, generator=g).to(dev)
acts = torch.randn(B, 10, 7, generator=g).to(dev); noise = torch.randn(B, 10, 7, generator=g).to(dev)
lib = L.load()
kw = dict(lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
opts = {"clip=None": FusedAdamW(m, **kw), "measure only": FusedAdamW(m, clip=GradClip(), **kw), "max_norm=1.0": FusedAdamW(m, clip=GradClip(max_norm=1.0), **kw)}


def steps(n, opt, overlap):
    for _ in range(n):
        sig = rand_log_logistic((B,), loc=math.log(0.5), scale=0.5, min_value=1e-3, max_value=80.0, device=dev)
        loss, _ = den.loss({"state_images": img}, acts, goal, noise, sig)
        loss.backward()
        opt.step(overlap=overlap)


variants = [(name, ov) for ov in (False, True) for name in opts]
ms = {v: [] for v in variants}
for rnd in range(ROUNDS):
    for name, ov in variants:
        lib.mode_set_option(b"bwd_coexec", 1 if ov else 0)          # as bench.py --mode train sets it for the two-pass step
        steps(WARM, opts[name], ov)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); steps(BLOCK, opts[name], ov); e1.record()
        torch.cuda.synchronize()
        ms[(name, ov)].append(e0.elapsed_time(e1) / BLOCK)
n_par = sum(p.numel() for p in m.parameters())
print(f"training step, C2 ({n_par / 1e6:.0f} M parameters), B = {B}, bf16, two-pass optimizer; {ROUNDS} alternating blocks of {BLOCK} steps per variant; ms per step")
print(f"{'variant':<16}{'overlap':<9}{'min':>8}{'median':>8}   blocks")
for (name, ov), v in ms.items():
    print(f"{name:<16}{str(ov):<9}{min(v):8.3f}{statistics.median(v):8.3f}   {' '.join(f'{x:.3f}' for x in v)}")
for name in opts:
    if name != "clip=None":
        c = opts[name].clip
        print(f"{name}: last total_norm {float(c.total_norm):.4g}, coef {float(c.coef):.4g}, skipped {int(c.skipped)}, {len(c.names)} tensors, {c._partial.numel()} chunks")
