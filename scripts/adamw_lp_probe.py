"""What bf16 moments do to the training step's time and memory.  ONE process, alternating rounds, the benchmark's training geometry (C2, B = 128, bf16,
two-pass optimizer): FusedAdamW(moment_dtype="fp32") against moment_dtype="bf16", each with step(overlap=False) and overlap=True - device events
around BLOCK steps, ROUNDS blocks per variant, min and median of the blocks' ms per step; then the isolated AdamW launch over the arena's decay region
(every parameter but the biases and gains: one launch) in us and TB/s for both at the library's default grid and at "adamw_blocks" 256 / 512 / 1024, and
the bytes each optimizer allocated.  Never imported by the package or by bench.py.

    python scripts/adamw_lp_probe.py > profiles/adamw_lp.txt"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd.optim import FusedAdamW, _adamw_launch  # noqa: E402
from mode_diffusion_policy_amd.utils import rand_log_logistic  # noqa: E402

BLOCK, ROUNDS, WARM = 50, 3, 3
LAUNCHES, LAUNCH_ROUNDS = 10, 5
dev = torch.device("cuda:0")
_, den = bench.build_model(dev, "bf16"); m = den.inner_model; den.train()
B = 128
g = torch.Generator().manual_seed(1)
img = torch.randn(B, 2, 2048, generator=g).to(dev); goal = torch.randn(B, 1, 512, generator=g).to(dev)
acts = torch.randn(B, 10, 7, generator=g).to(dev); noise = torch.randn(B, 10, 7, generator=g).to(dev)
lib = L.load()
kw = dict(lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
opts, alloc = {}, {}
for name in ("fp32", "bf16"):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    opts[name] = FusedAdamW(m, moment_dtype=name, **kw)
    torch.cuda.synchronize()
    alloc[name] = torch.cuda.memory_allocated() - before


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
print(f"{'moments':<10}{'overlap':<9}{'min':>8}{'median':>8}   blocks")
for (name, ov), v in ms.items():
    print(f"{name:<10}{str(ov):<9}{min(v):8.3f}{statistics.median(v):8.3f}   {' '.join(f'{x:.3f}' for x in v)}")

# ---- the isolated launch: the decay region of the arena in ONE launch (weights, gradients and moments as the steps above left them; lr = 0 and no
#      decay, so the weights stay put while every byte still moves), alternating between the two optimizers
ar = m.engine.arena
n = ar.bounds["decay"]
gp = dict(opts["fp32"].param_groups[0], lr=0.0, weight_decay=0.0)
GRIDS = (0, 256, 512, 1024)                                           # the "adamw_blocks" option: 0 = the library's default (256 for fp32 moments, 512 for bf16)
us = {(name, k): [] for name in opts for k in GRIDS}
for rnd in range(LAUNCH_ROUNDS + 1):
    for k in GRIDS:
        lib.mode_set_option(b"adamw_blocks", k)
        for name, opt in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                _adamw_launch(lib, ar.flat, ar.grad, opt.exp_avg, opt.exp_avg_sq, 0, n, gp, opt.step_count, moment_dtype=opt.moment_dtype,
                              round_seed=opt.round_seed, grad_scale=1.0, lp=ar.lp)
            e1.record()
            torch.cuda.synchronize()
            if rnd:                                                   # round 0 warms up
                us[(name, k)].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
lib.mode_set_option(b"adamw_blocks", 0)
print(f"\nisolated AdamW launch over the decay region ({n / 1e6:.1f} M elements, bf16 shadow written, no EMA); {LAUNCH_ROUNDS} alternating rounds of {LAUNCHES} launches; us per launch")
print(f"{'moments':<10}{'adamw_blocks':>13}{'B/elem':>7}{'min':>9}{'median':>9}{'TB/s':>7}   rounds")
for name, bpe in (("fp32", 30), ("bf16", 22)):
    for k in GRIDS:
        v = us[(name, k)]
        med = statistics.median(v)
        print(f"{name:<10}{k if k else 'default':>13}{bpe:>7}{min(v):9.1f}{med:9.1f}{n * bpe / med / 1e6:7.2f}   {' '.join(f'{x:.1f}' for x in v)}")
r = statistics.median(us[("bf16", 0)]) / statistics.median(us[("fp32", 0)])
print(f"bf16 / fp32 launch time at the defaults: {r:.3f} (byte count: {22 / 30:.3f})")

print("\nbytes allocated by constructing the optimizer (both moments)")
for name, opt in opts.items():
    print(f"{name:<10}{alloc[name] / 2**20:10.1f} MiB   exp_avg {opt.exp_avg.numel() * opt.exp_avg.element_size() / 2**20:.1f} MiB, {opt.exp_avg.dtype}")
