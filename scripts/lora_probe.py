"""What LoRA adapters cost and save at the benchmark's training geometry (C2, B = 128, bf16).  ONE process, alternating rounds, medians (the method of
scripts/grad_clip_probe.py): the full fine-tune step (two-pass FusedAdamW) on one model against the adapter step (forward, backward, projection,
FlatAdamW on the adapter, merge) at r = 4 / 16 / 64 on a second model with the same weights; the merge and the projection isolated, against their byte
counts; the state a task carries; the task switch under a captured rollout graph.  Never imported by the package or by bench.py.

    python scripts/lora_probe.py > profiles/lora.txt"""
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mode_diffusion_policy_amd import LoraAdapter, rollout  # noqa: E402
from mode_diffusion_policy_amd.lora import target_shapes  # noqa: E402
from mode_diffusion_policy_amd.optim import FlatAdamW, FusedAdamW  # noqa: E402
from mode_diffusion_policy_amd.utils import rand_log_logistic  # noqa: E402

BLOCK, ROUNDS, WARM, ISO = 20, 3, 3, 10
RANKS = (4, 16, 64)
dev = torch.device("cuda:0")
_, den_full = bench.build_model(dev, "bf16"); den_full.train()
_, den_ad = bench.build_model(dev, "bf16"); den_ad.train()
m_full, m = den_full.inner_model, den_ad.inner_model
B = 128
g = torch.Generator().manual_seed(1)
img = torch.randn(B, 2, 2048, generator=g).to(dev); goal = torch.randn(B, 1, 512, generator=g).to(dev)
acts = torch.randn(B, 10, 7, generator=g).to(dev); noise = torch.randn(B, 10, 7, generator=g).to(dev)
opt_full = FusedAdamW(m_full, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
ads = {r: LoraAdapter(m, rank=r, seed=r) for r in RANKS}
opts = {r: FlatAdamW(ads[r].parameters(), lr=1e-4, weight_decay=0.0) for r in RANKS}


def loss_backward(den):
    sig = rand_log_logistic((B,), loc=math.log(0.5), scale=0.5, min_value=1e-3, max_value=80.0, device=dev)
    loss, _ = den.loss({"state_images": img}, acts, goal, noise, sig)
    loss.backward()


def full_steps(n):
    for _ in range(n):
        loss_backward(den_full)
        opt_full.step(overlap=False)


def adapter_steps(r):
    def run(n):
        for _ in range(n):
            opts[r].zero_grad()
            loss_backward(den_ad)                                # the forward's engine access re-merges after the previous step
            opts[r].step()
    return run


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(n); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


ms = {"full fine-tune": []}
for r in RANKS:
    ms[f"adapter r={r}"], ms[f"  merge r={r}"], ms[f"  projection r={r}"] = [], [], []
eng = m.engine
flat = torch.randn(eng.arena.bounds["total"], device=dev)       # a dense gradient buffer for the isolated projection
for rnd in range(ROUNDS):
    full_steps(WARM)
    ms["full fine-tune"].append(timed(full_steps, BLOCK))
    for r in RANKS:
        ad = ads[r].attach()
        run = adapter_steps(r)
        run(WARM)
        ms[f"adapter r={r}"].append(timed(run, BLOCK))
        params = list(ad.parameters())
        ms[f"  merge r={r}"].append(timed(lambda n: [ad._merge_into(eng) for _ in range(n)], ISO))
        ms[f"  projection r={r}"].append(timed(lambda n: [ad.project(eng, flat, params) for _ in range(n)], ISO))

shapes = target_shapes(m)
elems = m.num_layers * sum(G * rows * cols for G, rows, cols in shapes.values())
n_par = sum(p.numel() for p in m.parameters())
print(f"LoRA at C2 ({n_par / 1e6:.0f} M parameters, {elems / 1e6:.0f} M in the adapted matrices), B = {B}, bf16; {ROUNDS} alternating rounds, blocks of {BLOCK} steps "
      f"({ISO} calls for the isolated kernels); ms per step / call")
print(f"{'variant':<22}{'min':>8}{'median':>8}   blocks")
for name, v in ms.items():
    print(f"{name:<22}{min(v):8.3f}{statistics.median(v):8.3f}   {' '.join(f'{x:.3f}' for x in v)}")
print("isolated kernels against their byte counts (merge: 4 B read + 2 B written per element of the adapted matrices; projection: 4 B read per element,"
      " its dA partials in the workspace not counted)")
for r in RANKS:
    tm, tp = statistics.median(ms[f"  merge r={r}"]), statistics.median(ms[f"  projection r={r}"])
    part = 4 * m.num_layers * sum(G * -(-rows // 64) * r * cols for G, rows, cols in shapes.values())
    print(f"r={r:<3} merge {6 * elems / tm / 1e9:7.2f} TB/s   projection {4 * elems / tp / 1e9:7.2f} TB/s (+ {2 * part / 2 ** 20:.0f} MiB of partials written and read)")
print("state a task carries (fp32 moments; the full fine-tune: the whole arena)")
full_n = m_full.engine.arena.bounds["no_decay"]
print(f"{'full fine-tune':<16} optimizer state {8 * full_n / 2 ** 20:9.1f} MiB   checkpoint {4 * n_par:>13,d} B   data-parallel exchange {4 * full_n:>13,d} B")
for r in RANKS:
    n = sum(p.numel() for p in ads[r].parameters())
    print(f"{'adapter r=' + str(r):<16} optimizer state {8 * n / 2 ** 20:9.1f} MiB   checkpoint {4 * n:>13,d} B   data-parallel exchange {4 * n:>13,d} B   "
          f"({100 * n / n_par:.2f} % of the model)")

# ---- task switch: two resident adapters under one captured rollout graph; attach() of the other one up to the end of the next replanning step
den_ad.eval()
a, b = ads[16], LoraAdapter(m, rank=16, seed=99)
with torch.no_grad():
    b.B_w1.normal_(0, 0.01)
a.attach()
pol = rollout.ChunkedRolloutPolicy(den_ad, act_window_size=10, multistep=10, action_dim=7)
emb, gl = {"state_images": img}, goal
for _ in range(3):
    pol.denoise_actions(emb, gl)
graph = m._route_cache["graph"]["graph"]


def wall(switch):
    out = []
    for i in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if switch:
            (b if i % 2 == 0 else a).attach()
        pol.denoise_actions(emb, gl)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


same, swap = wall(False), wall(True)
assert m._route_cache["graph"]["graph"] is graph
print(f"task switch, r = 16, graphed 10-step DDIM chunk at B = {B} (wall ms incl. synchronize, 10 calls): same task median {statistics.median(same):.3f}, "
      f"attach() of a resident adapter + next chunk median {statistics.median(swap):.3f} (same graph object: no recapture)")
