"""Cost of a control step of 32 environments on the benchmarked model (C2 geometry, bf16, 10-step DDIM chunks, act_window_size = multistep = 10):
(a) ChunkedRolloutPolicy in lockstep (every 10th step replans all 32), (b) VectorEnvPolicy in lockstep, (c) VectorEnvPolicy with the environments'
phases spread evenly (3-4 of them replan on every step), (d) 32 separate B = 1 ChunkedRolloutPolicy objects stepped in turn, their phases spread
like (c).  Per control step: host clock around the step(s) and a device synchronise; median and mean over the timed steps after warm-up.

    python scripts/vector_env_probe.py [steps]   -> profiles/vector_env.txt"""
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

B, W = 32, 10


def build(dev):
    torch.manual_seed(0)
    C2 = bench.C2
    m = M.MoDeDiT(obs_dim=C2["obs_dim"], goal_dim=C2["goal_dim"], device=str(dev), goal_conditioned=True, action_dim=7, embed_dim=C2["embed_dim"],
                  embed_pdrob=0, attn_pdrop=0.3, n_layers=C2["n_layers"], n_heads=C2["n_heads"], goal_seq_len=1, obs_seq_len=1, action_seq_len=W,
                  mlp_pdrop=0.1, goal_drop=0.1, num_experts=C2["num_experts"], top_k=C2["top_k"], compute_dtype="bf16")
    return M.GCDenoiser(m.to(dev).eval(), bench.SIGMA_DATA).eval()


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


def main():
    dev = torch.device("cuda:0")
    n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    den = build(dev)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 2, bench.C2["obs_dim"], generator=g).to(dev)
    goal = torch.randn(B, bench.C2["goal_dim"], generator=g).to(dev)
    st = {"state_images": img}
    kw = dict(act_window_size=W, multistep=W, action_dim=7, sigma_max=80.0)
    rows = {}

    a = rollout.ChunkedRolloutPolicy(den, **kw)
    rows["(a) ChunkedRolloutPolicy, lockstep"] = timed(lambda: a.step(st, goal), n_steps, 2 * W)

    b = rollout.VectorEnvPolicy(den, B, **kw)
    b.warmup(st, goal)
    rows["(b) VectorEnvPolicy, lockstep"] = timed(lambda: b.step(st, goal), n_steps, 2 * W)

    c = rollout.VectorEnvPolicy(den, B, **kw)
    c.warmup(st, goal)
    phase = np.arange(B) % W
    for t in range(W):                                            # environment e joins at step e % W: the phases are spread evenly
        c.step(st, goal, active=phase <= t)
    per_step = []

    def step_c():
        c.step(st, goal)
        per_step.append(len(c.replanned))
    rows["(c) VectorEnvPolicy, phases spread"] = timed(step_c, n_steps, 2 * W)
    m_mean = float(np.mean(per_step[2 * W:]))

    solo = [rollout.ChunkedRolloutPolicy(den, **kw) for _ in range(B)]
    for p in solo:
        p.step({"state_images": img[:1]}, goal[:1])               # capture the B = 1 chunk (the model keeps one graph per batch size: shared by all 32)
    for e, p in enumerate(solo):
        p.reset()
        for _ in range(e % W):
            p.step({"state_images": img[e:e + 1]}, goal[e:e + 1])

    def step_d():
        for e, p in enumerate(solo):
            p.step({"state_images": img[e:e + 1]}, goal[e:e + 1])
    rows["(d) 32 x ChunkedRolloutPolicy(B = 1), phases spread"] = timed(step_d, n_steps, 2 * W)

    print(f"Control step of {B} environments, C2 geometry (D {bench.C2['embed_dim']}, {bench.C2['n_layers']} layers, {bench.C2['num_experts']} experts, "
          f"top-{bench.C2['top_k']}), bf16, 10-step DDIM, act_window_size = multistep = {W}; ms per control step over {n_steps} steps after "
          f"{2 * W} warm-up steps (host clock around step + device synchronise)")
    print(f"{'case':56s} {'median ms':>10s} {'mean ms':>9s}")
    for name, (med, mean) in rows.items():
        print(f"{name:56s} {med:10.3f} {mean:9.3f}")
    print(f"(c): {m_mean:.2f} environments replan per step on average (buckets {rollout._buckets(B)})")


if __name__ == "__main__":
    main()
