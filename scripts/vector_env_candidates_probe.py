"""Cost of a replanning control step of VectorEnvPolicy with candidate selection (C2 geometry, bf16, 10-step DDIM, act_window_size = 10,
multistep = 5, lockstep: every 5th step all environments replan), for num_envs in {1, 8, 32} and candidates N in {1, 2, 4, 8}, next to the same
policy built without the keyword (twice: two policies of the same code, whose difference is the same-code spread).  A chunk of an N arm runs at
batch num_envs * N, and every timed replan scores its candidates against a previous plan.  All arms live in one process and take turns, one
replanning step each per round; per replanning step: host clock around step + a device synchronise, after two untimed rounds (the first
captures the arm's chunk).  Median and mean ms over the rounds, and each arm's ratio to the policy without the keyword.

    python scripts/vector_env_candidates_probe.py [rounds] [--out FILE]        -> profiles/vector_env_candidates.txt (or FILE)

Nothing here says what candidate selection does to task success: there is no trained checkpoint and no simulator in this repository."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, S, STEPS = 10, 5, 10
SIZES, NS = (1, 8, 32), (1, 2, 4, 8)


def build(dev):
    import torch
    import bench
    import mode_diffusion_policy_amd as M
    torch.manual_seed(0)
    C2 = bench.C2
    m = M.MoDeDiT(obs_dim=C2["obs_dim"], goal_dim=C2["goal_dim"], device=str(dev), goal_conditioned=True, action_dim=7, embed_dim=C2["embed_dim"],
                  embed_pdrob=0, attn_pdrop=0.3, n_layers=C2["n_layers"], n_heads=C2["n_heads"], goal_seq_len=1, obs_seq_len=1, action_seq_len=W,
                  mlp_pdrop=0.1, goal_drop=0.1, num_experts=C2["num_experts"], top_k=C2["top_k"], compute_dtype="bf16")
    return M.GCDenoiser(m.to(dev).eval(), bench.SIGMA_DATA).eval()


def inputs(dev, n):
    import torch
    import bench
    g = torch.Generator().manual_seed(1)
    return ({"state_images": torch.randn(n, 2, bench.C2["obs_dim"], generator=g).to(dev)}, torch.randn(n, bench.C2["goal_dim"], generator=g).to(dev))


def measure(arms, rounds):
    """arms: {name: (policy, observation, goal)}.  One replanning step of every arm per round, in turn; the S - 1 steps that follow it are not
    timed.  Returns {name: (median ms, mean ms)}."""
    import torch
    ts = {name: [] for name in arms}
    for r in range(rounds + 2):
        for name, (pol, st, goal) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pol.step(st, goal)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert len(pol.replanned) == pol.num_envs, name
            if r >= 2:
                ts[name].append(dt)
            for _ in range(S - 1):
                pol.step(st, goal)
    return {name: (statistics.median(v), statistics.fmean(v)) for name, v in ts.items()}


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 60
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "vector_env_candidates.txt")
    import torch
    import bench
    from mode_diffusion_policy_amd import rollout
    dev = torch.device("cuda:0")
    den = build(dev)
    arms = {}
    for n in SIZES:
        st, goal = inputs(dev, n)
        for name, kw in [("without (a)", {}), ("without (b)", {})] + [(f"N = {N}", dict(candidates=N)) for N in NS]:
            pol = rollout.VectorEnvPolicy(den, n, act_window_size=W, multistep=S, action_dim=7, sigma_max=80.0, num_sampling_steps=STEPS, **kw)
            arms[(n, name)] = (pol, st, goal)
    res = measure(arms, rounds)
    C2 = bench.C2
    lines = [f"Replanning control step of VectorEnvPolicy, C2 geometry (D {C2['embed_dim']}, {C2['n_layers']} layers, {C2['num_experts']} experts, "
             f"top-{C2['top_k']}), bf16, {STEPS}-step DDIM, act_window_size = {W}, multistep = {S}, lockstep; ms per replanning step over {rounds} "
             f"rounds (all arms in one process, one replanning step each per round, in turn; host clock around step + device synchronise, after 2 "
             f"untimed rounds).  'without': the policy built without the keyword (two of them).  An N arm's chunk runs at batch num_envs * N and "
             f"selects against the previous plan (coherence_decay = 0.5); N = 1 is the policy without the keyword by construction.",
             f"{'num_envs':>8s} {'candidates':>11s} {'chunk batch':>11s} {'median ms':>10s} {'mean ms':>9s} {'/ without':>9s}"]
    for n in SIZES:
        base = statistics.fmean(res[(n, f"without ({c})")][0] for c in "ab")
        for (nn, name), (med, mean) in res.items():
            if nn == n:
                N = int(name.split()[-1]) if name.startswith("N") else 1
                lines.append(f"{n:8d} {name:>11s} {n * N:11d} {med:10.3f} {mean:9.3f} {med / base:9.3f}")
        a, b = res[(n, "without (a)")][0], res[(n, "without (b)")][0]
        lines.append(f"{'':8s} same-code spread, without (a) vs without (b): {abs(a - b):.3f} ms = {100 * abs(a - b) / base:.2f} % of that replan")
    lines += ["", "Not measured: what candidate selection does to task success (no trained checkpoint, no simulator here)."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
