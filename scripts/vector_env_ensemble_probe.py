"""Cost of temporal ensembling in VectorEnvPolicy: a control step of 32 environments on the benchmarked model (C2 geometry, bf16, 10-step DDIM
chunks, act_window_size = 10) with temporal_ensemble = 0.01 against the same policy without the option, each pair in one process:
(1) multistep = 1: all 32 environments replan on every step, 10 live plans each - the chunk is the same, the epilogue differs;
(2) multistep = 3 with the environments' phases spread over the stride (10-11 of them replan on every step), 4 live plans;
(3) multistep = 3 in lockstep, the steps WITHOUT a replan only: the one-launch path, new kernel against old.
Per control step: host clock around the step and a device synchronise; median, mean, 10th and 90th percentile over the timed steps after
warm-up (the protocol of scripts/vector_env_probe.py).  The policies are built and timed one after the other, not interleaved: a new policy's
first chunk re-resolves the model's routing cache, after which an older policy's chunks would rebuild their schedule state inside the timed steps.

    python scripts/vector_env_ensemble_probe.py [steps]   -> profiles/vector_env_ensemble.txt"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mode_diffusion_policy_amd import rollout  # noqa: E402
from vector_env_probe import B, W, build  # noqa: E402

M_ENS = 0.01


def stats(ts):
    q = np.percentile(ts, [10, 90])
    return statistics.median(ts), statistics.fmean(ts), float(q[0]), float(q[1])


def timed(pol, st, goal, n_steps, warm, keep=lambda pol: True):
    """``n_steps`` timed control steps for which ``keep(pol)`` holds after the step (the others run untimed in between)."""
    for _ in range(warm):
        pol.step(st, goal)
    torch.cuda.synchronize()
    ts = []
    while len(ts) < n_steps:
        t0 = time.perf_counter()
        pol.step(st, goal)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if keep(pol):
            ts.append(dt)
    return stats(ts)


def main():
    dev = torch.device("cuda:0")
    n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    den = build(dev)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 2, bench.C2["obs_dim"], generator=g).to(dev)
    goal = torch.randn(B, bench.C2["goal_dim"], generator=g).to(dev)
    st = {"state_images": img}

    def make(s, ens, spread):
        pol = rollout.VectorEnvPolicy(den, B, act_window_size=W, multistep=s, action_dim=7, sigma_max=80.0, temporal_ensemble=M_ENS if ens else None)
        pol.warmup(st, goal)
        if spread:                                                # environment e joins at step e % s: the phases are spread evenly
            for t in range(s):
                pol.step(st, goal, active=np.arange(B) % s <= t)
        return pol

    rows = []
    for name, s, spread, keep in (("(1) multistep 1, all 32 replan every step", 1, False, lambda p: True),
                                  ("(2) multistep 3, phases spread", 3, True, lambda p: True),
                                  ("(3) multistep 3, lockstep: steps without a replan", 3, False, lambda p: not p.replanned)):
        for ens in (False, True):
            pol = make(s, ens, spread)
            rows.append((name, "ensembled" if ens else "baseline", timed(pol, st, goal, n_steps, 2 * W, keep)))
            del pol

    print(f"Control step of {B} environments, C2 geometry (D {bench.C2['embed_dim']}, {bench.C2['n_layers']} layers, {bench.C2['num_experts']} experts, "
          f"top-{bench.C2['top_k']}), bf16, 10-step DDIM, act_window_size = {W}, temporal_ensemble = {M_ENS} against None; ms per control step over "
          f"{n_steps} steps after {2 * W} warm-up steps (host clock around step + device synchronise)")
    print(f"{'case':52s} {'policy':>10s} {'median ms':>10s} {'mean ms':>9s} {'p10 ms':>8s} {'p90 ms':>8s}")
    for name, kind, (med, mean, p10, p90) in rows:
        print(f"{name:52s} {kind:>10s} {med:10.3f} {mean:9.3f} {p10:8.3f} {p90:8.3f}")
    for i in range(0, len(rows), 2):
        (name, _, b), (_, _, e) = rows[i], rows[i + 1]
        print(f"{name}: ensembled median - baseline median = {e[0] - b[0]:+.3f} ms; baseline p10-p90 spread = {b[3] - b[2]:.3f} ms")


if __name__ == "__main__":
    main()
