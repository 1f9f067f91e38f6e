"""Cost of a control step of a VectorEnvPolicy fed raw camera frames, on the benchmarked model (C2 geometry, bf16, 10-step DDIM chunks,
act_window_size = multistep = 10) with two FiLM-ResNet-50 encoders at 224 x 224 (T = 1, bf16 autocast), the environments' phases spread evenly:
(a) ``policy.embed`` of every environment's frames, then ``step`` on the embeddings (the route before raw frames were accepted), (b) ``step`` on
the frames (only the replanning environments' rows are gathered and encoded).  Per control step: host clock around the step and a device
synchronise; median and mean over the timed steps after warm-up.  Also the device memory each bucket's capture takes in (b) (reserved-memory
growth across the bucket's warm-up: its encoder graph, its chunk graph, their buffers).

    python scripts/vector_env_frames_probe.py [steps] [num_envs ...]   -> profiles/vector_env_frames.txt"""
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import rollout  # noqa: E402

W, HW = 10, 224


def build(dev):
    torch.manual_seed(0)
    C2 = bench.C2
    m = M.MoDeDiT(obs_dim=C2["obs_dim"], goal_dim=C2["goal_dim"], device=str(dev), goal_conditioned=True, action_dim=7, embed_dim=C2["embed_dim"],
                  embed_pdrob=0, attn_pdrop=0.3, n_layers=C2["n_layers"], n_heads=C2["n_heads"], goal_seq_len=1, obs_seq_len=1, action_seq_len=W,
                  mlp_pdrop=0.1, goal_drop=0.1, num_experts=C2["num_experts"], top_k=C2["top_k"], compute_dtype="bf16")
    encs = [M.FiLMResNet50Policy(C2["goal_dim"]).to(dev).eval() for _ in range(2)]
    return M.GCDenoiser(m.to(dev).eval(), bench.SIGMA_DATA).eval(), encs


def timed(step, n_steps, warm):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n_steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), statistics.fmean(ts)


def release():
    """Free what a dropped policy held (its graphs sit in reference cycles) before the next one measures its own memory."""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def spread(pol, st, goal, n):
    phase = np.arange(n) % W
    for t in range(W):                                            # environment e joins at step e % W: the phases are spread evenly
        pol.step(st(), goal, active=phase <= t)


def run(den, encs, n, n_steps, dev):
    g = torch.Generator().manual_seed(n)
    frames = {"rgb_obs": {"rgb_static": torch.randn(n, 1, 3, HW, HW, generator=g).to(dev), "rgb_gripper": torch.randn(n, 1, 3, HW, HW, generator=g).to(dev)}}
    goal = torch.randn(n, bench.C2["goal_dim"], generator=g).to(dev)
    kw = dict(act_window_size=W, multistep=W, action_dim=7, sigma_max=80.0, static_resnet=encs[0], gripper_resnet=encs[1])
    rows, per_step = {}, []

    a = rollout.VectorEnvPolicy(den, n, **kw)
    a.warmup(a.embed(frames, goal), goal)
    spread(a, lambda: a.embed(frames, goal), goal, n)
    rows["(a) embed all rows, then step on embeddings"] = timed(lambda: a.step(a.embed(frames, goal), goal), n_steps, 2 * W)
    del a
    release()

    b = rollout.VectorEnvPolicy(den, n, **kw)
    mem, run_chunk = {}, b._run_chunk

    def counted(mb, m):
        torch.cuda.synchronize()
        r0 = torch.cuda.memory_reserved()
        run_chunk(mb, m)
        torch.cuda.synchronize()
        mem[mb] = (torch.cuda.memory_reserved() - r0) / 2 ** 20
    b._run_chunk = counted
    b.warmup(frames, goal)
    b._run_chunk = run_chunk
    spread(b, lambda: frames, goal, n)

    def step_b():
        b.step(frames, goal)
        per_step.append(len(b.replanned))
    rows["(b) step on frames"] = timed(step_b, n_steps, 2 * W)
    del b
    release()
    return rows, float(np.mean(per_step[2 * W:])), mem


def main():
    dev = torch.device("cuda:0")
    n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    envs = [int(v) for v in sys.argv[2:]] or [32, 256]
    den, encs = build(dev)
    C2 = bench.C2
    print(f"Control step of a VectorEnvPolicy on raw frames, C2 geometry (D {C2['embed_dim']}, {C2['n_layers']} layers, {C2['num_experts']} experts, "
          f"top-{C2['top_k']}), bf16, 10-step DDIM, act_window_size = multistep = {W}, two FiLM-ResNet-50 at {HW} x {HW} (T = 1, bf16 autocast), "
          f"phases spread evenly; ms per control step over {n_steps} steps after {2 * W} warm-up steps (host clock around step + device synchronise)")
    for n in envs:
        rows, m_mean, mem = run(den, encs, n, n_steps, dev)
        print(f"\nnum_envs = {n}: {m_mean:.2f} environments replan per step on average (buckets {rollout._buckets(n)})")
        print(f"{'case':48s} {'median ms':>10s} {'mean ms':>9s}")
        for name, (med, mean) in rows.items():
            print(f"{name:48s} {med:10.3f} {mean:9.3f}")
        (am, _), (bm, _) = rows.values()
        print(f"(b) - (a): {bm - am:+.3f} ms median ({bm / am:.3f}x)")
        print("device memory per bucket in (b), MiB reserved by its warm-up: " + ", ".join(f"{k}: {v:.0f}" for k, v in sorted(mem.items())))


if __name__ == "__main__":
    main()
