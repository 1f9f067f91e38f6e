"""What LoraAdapter(grad="factored") costs against grad="dense" and against the full fine-tune step at the benchmark's training geometry (C2, B = 128,
bf16).  The protocol of scripts/lora_probe.py: ONE process, alternating rounds, medians.  The adapter step (forward, backward, FlatAdamW on the adapter,
merge) in both gradient modes at r = 4 / 16 / 64 on one model, the full fine-tune step (two-pass FusedAdamW) on a second model with the same weights; the
factored launch of every target kind isolated, against the bytes of X and dY it has to read; the peak memory of a step in both modes; and how far the two
modes' gradients lie apart on the same batch and seed.  Never imported by the package or by bench.py.

    python scripts/lora_fact_probe.py > profiles/lora_fact.txt"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mode_diffusion_policy_amd import LoraAdapter  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd.lora import target_shapes  # noqa: E402
from mode_diffusion_policy_amd.optim import FlatAdamW, FusedAdamW  # noqa: E402
from mode_diffusion_policy_amd.utils import rand_log_logistic  # noqa: E402

BLOCK, ROUNDS, WARM, ISO = 20, 3, 3, 10
RANKS = (4, 16, 64)
MODES = ("dense", "factored")
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
    for mode in MODES:
        ms[f"adapter r={r} {mode}"] = []
for rnd in range(ROUNDS):
    full_steps(WARM)
    ms["full fine-tune"].append(timed(full_steps, BLOCK))
    for r in RANKS:
        ad = ads[r].attach()
        run = adapter_steps(r)
        for mode in MODES:
            ad.grad = mode
            run(WARM)
            ms[f"adapter r={r} {mode}"].append(timed(run, BLOCK))

n_par = sum(p.numel() for p in m.parameters())
print(f"LoRA gradient modes at C2 ({n_par / 1e6:.0f} M parameters), B = {B}, bf16; {ROUNDS} alternating rounds, blocks of {BLOCK} steps "
      f"({ISO} calls for the isolated launches); ms per step / call")
print(f"{'variant':<26}{'min':>8}{'median':>8}   blocks")
for name, v in ms.items():
    print(f"{name:<26}{min(v):8.3f}{statistics.median(v):8.3f}   {' '.join(f'{x:.3f}' for x in v)}")
full = statistics.median(ms["full fine-tune"])
for r in RANKS:
    d, f = (statistics.median(ms[f"adapter r={r} {mode}"]) for mode in MODES)
    print(f"r={r:<3} factored / dense = {f / d:.3f} ({'faster' if f < d else 'NOT faster'} than dense);  factored / full fine-tune = {f / full:.3f} "
          f"({'below' if f < full else 'above'} the full fine-tune step)")

# ---- the factored launch of one layer, per target kind, on synthetic operands of the chain's shapes: N = B T token rows, N k sorted rows in E even groups
lib = L.load()
T_, k_, E_ = m.seq_len, m.top_k, m.num_experts
N, NK = B * T_, B * T_ * k_
shapes = target_shapes(m)
rows_of = {"wqkv": N, "wo": N, "w1": NK, "w2": NK}
offs = torch.tensor([NK * e // E_ for e in range(E_ + 1)], dtype=torch.int32, device=dev)
perm = (torch.randperm(NK, device=dev) % N).to(torch.int32)
scale = torch.ones(1, device=dev)
print("isolated mode_lora_fact_grad per layer and kind (down + up + finish), against the bytes of X and dY read ONCE (the launch reads them twice; T, U and "
      "the row-block shares in the workspace not counted)")
per_layer = {r: 0.0 for r in RANKS}
for kind, (G, rows, cols) in shapes.items():
    M_ = rows_of[kind]
    X = torch.randn(N if kind == "w1" else M_, cols, device=dev).bfloat16(); dY = torch.randn(M_, rows, device=dev).bfloat16()
    for r in RANKS:
        A = torch.randn(G, r, cols, device=dev); Bm = torch.randn(G, rows, r, device=dev)
        dA, dB = torch.empty_like(A), torch.empty_like(Bm)
        d = L.ModeLoraFactDesc(G=G, rows=rows, cols=cols, r=r, M=M_, dtype=L.MODE_BF16, X=X.data_ptr(), ld_x=cols, x_rows=perm.data_ptr() if kind == "w1" else None,
                               dY=dY.data_ptr(), ld_dy=rows, group_offsets=offs.data_ptr() if G > 1 else None, A=A.data_ptr(), B=Bm.data_ptr(),
                               scale=scale.data_ptr(), dA=dA.data_ptr(), dB=dB.data_ptr())
        ws = torch.empty(lib.mode_lora_fact_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def call(n):
            for _ in range(n):
                L.check(lib.mode_lora_fact_grad(C.byref(d), ws.data_ptr(), ws.numel(), st), "lora_fact_grad")
        call(3)
        t = statistics.median(timed(call, ISO) for _ in range(ROUNDS))
        nbytes = 2 * M_ * (rows + cols)
        per_layer[r] += t
        print(f"{kind:<5} G={G} [{rows:>5} x {cols:>4}] M={M_:<5} r={r:<3} {t * 1e3:8.1f} us   {nbytes / t / 1e9:6.2f} TB/s of {nbytes / 2 ** 20:6.1f} MiB   "
              f"workspace {ws.numel() / 2 ** 20:6.1f} MiB")
for r in RANKS:
    print(f"r={r:<3} all four kinds of one layer {per_layer[r] * 1e3:8.1f} us, of {m.num_layers} layers {per_layer[r] * m.num_layers:7.3f} ms")

# ---- peak memory of one adapter step per mode (r = 16; both models and both optimizers resident throughout, so the DIFFERENCE is the mode's)
ad = ads[16]
peaks = {}
for mode in MODES:
    ad.detach()                                                   # drops the model's LoRA buffers of the other mode
    ad.grad = mode
    ad.attach()
    run = adapter_steps(16)
    run(2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    run(2)
    torch.cuda.synchronize()
    peaks[mode] = torch.cuda.max_memory_allocated()
    held = sum(t.numel() * t.element_size() for t in m.engine._lora_bufs.values())
    print(f"peak torch.cuda.max_memory_allocated() of an adapter step, r = 16, grad={mode:<9} {peaks[mode] / 2 ** 20:10.1f} MiB   "
          f"(LoRA buffers held by the engine: {held / 2 ** 20:8.1f} MiB in {sorted(m.engine._lora_bufs)})")
print(f"dense - factored = {(peaks['dense'] - peaks['factored']) / 2 ** 20:.1f} MiB")

# ---- the two modes on the same weights, batch and seed: rel-L2 of every adapter tensor's gradient, factored against dense
for r in RANKS:
    ad = ads[r].attach()
    with torch.no_grad():
        for _, _, b in ad.pairs():
            b.normal_(0, 0.02)
    got = {}
    for mode in MODES:
        ad.grad = mode
        opts[r].zero_grad()
        torch.manual_seed(123)
        loss_backward(den_ad)
        torch.cuda.synchronize()
        got[mode] = {n: p.grad.double().clone() for n, p in ad.named_parameters()}
    worst = max((float((got["factored"][n] - got["dense"][n]).norm() / got["dense"][n].norm()), n) for n in got["dense"])
    print(f"r={r:<3} factored vs dense gradients, same batch and seed: worst rel-L2 {worst[0]:.2e} at {worst[1]}")
    opts[r].zero_grad()
