"""Cost of a replanning control step of VectorEnvPolicy with warm-started replans (C2 geometry, bf16, 10-step DDIM, act_window_size = 10,
multistep = 5, lockstep: every 5th step all environments replan), for num_envs 1 and 32 and warm_start None (twice: two policies of the same
code, whose difference is the same-code spread) and k in {3, 5, 7} (every timed replan of those arms is warm).  All arms live in one process and
take turns, one replanning step each per round; per replanning step: host clock around step + a device synchronise, after warmup and two
untimed rounds.  Median and mean ms over the rounds, and each arm's ratio to the cold replan next to (n - k) / n.

    python scripts/vector_env_warm_probe.py [rounds]                      -> profiles/vector_env_warm_start.txt
    python scripts/vector_env_warm_probe.py [rounds] --parent DIR [runs]  also: the cold replan of the checkout in DIR (built, e.g. the parent
        commit; it needs no copy of this script) against this tree's, each measured in fresh processes that take turns, `runs` of each
    python scripts/vector_env_warm_probe.py [rounds] --cold-json           one process of that comparison: the policy built without the keyword

Nothing here says what warm-started plans do to task success: there is no trained checkpoint and no simulator in this repository."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("MODE_PROBE_TREE") or HERE
sys.path.insert(0, ROOT)

W, S, STEPS = 10, 5, 10
SIZES, KS = (1, 32), (3, 5, 7)


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


def measure(arms, rounds):
    """arms: {name: (policy, observation, goal, rows expected in replanned_warm)}.  One replanning step of every arm per round, in turn; the
    S - 1 steps that follow it are not timed.  Returns {name: (median ms, mean ms)}."""
    import torch
    ts = {name: [] for name in arms}
    for r in range(rounds + 2):
        for name, (pol, st, goal, warm) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pol.step(st, goal)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert len(pol.replanned) == pol.num_envs, name
            if r >= 2:
                assert len(getattr(pol, "replanned_warm", [])) == warm, name
                ts[name].append(dt)
            for _ in range(S - 1):
                pol.step(st, goal)
    return {name: (statistics.median(v), statistics.fmean(v)) for name, v in ts.items()}


def inputs(dev, n):
    import torch
    import bench
    g = torch.Generator().manual_seed(1)
    return ({"state_images": torch.randn(n, 2, bench.C2["obs_dim"], generator=g).to(dev)}, torch.randn(n, bench.C2["goal_dim"], generator=g).to(dev))


def cold_json(rounds):
    """The cold replan of the tree this process imports (MODE_PROBE_TREE, else this script's): one JSON line {num_envs: [median, mean]}."""
    import torch
    from mode_diffusion_policy_amd import rollout
    dev = torch.device("cuda:0")
    den = build(dev)
    arms = {}
    for n in SIZES:
        st, goal = inputs(dev, n)
        pol = rollout.VectorEnvPolicy(den, n, act_window_size=W, multistep=S, action_dim=7, sigma_max=80.0, num_sampling_steps=STEPS)
        pol.warmup(st, goal)
        arms[str(n)] = (pol, st, goal, 0)
    print(json.dumps(measure(arms, rounds)))


def against(parent, rounds, runs):
    """Fresh processes, taking turns: the checkout in ``parent`` and this tree, ``runs`` of each.  {tree: {num_envs: [medians of the runs]}}."""
    out = {"parent": {str(n): [] for n in SIZES}, "this tree": {str(n): [] for n in SIZES}}
    pair = (("parent", os.path.abspath(parent)), ("this tree", HERE))
    for run in range(runs):
        for tree, root in pair[::-1] if run % 2 else pair:        # (the order flips every run: neither tree always follows the other)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), str(rounds), "--cold-json"], env=dict(os.environ, MODE_PROBE_TREE=root),
                                 cwd=root, check=True, capture_output=True, text=True, timeout=300)
            for n, (med, _) in json.loads(res.stdout.strip().splitlines()[-1]).items():
                out[tree][n].append(med)
            print(f"{tree}: {res.stdout.strip().splitlines()[-1]}", file=sys.stderr, flush=True)
    return out


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 60
    if "--cold-json" in args:
        return cold_json(rounds)
    cmp = None
    if "--parent" in args:                                        # (before this process opens the device)
        i = args.index("--parent")
        cmp = against(args[i + 1], rounds, int(args[i + 2]) if len(args) > i + 2 else 3)
    import torch
    import bench
    from mode_diffusion_policy_amd import rollout
    dev = torch.device("cuda:0")
    den = build(dev)
    arms = {}
    for n in SIZES:
        st, goal = inputs(dev, n)
        for name, k in [("None (a)", None), ("None (b)", None)] + [(f"k = {k}", k) for k in KS]:
            pol = rollout.VectorEnvPolicy(den, n, act_window_size=W, multistep=S, action_dim=7, sigma_max=80.0, num_sampling_steps=STEPS, warm_start=k)
            pol.warmup(st, goal)
            arms[(n, name)] = (pol, st, goal, 0 if k is None else n)
    res = measure(arms, rounds)
    C2 = bench.C2
    print(f"Replanning control step of VectorEnvPolicy, C2 geometry (D {C2['embed_dim']}, {C2['n_layers']} layers, {C2['num_experts']} experts, "
          f"top-{C2['top_k']}), bf16, {STEPS}-step DDIM, act_window_size = {W}, multistep = {S}, lockstep; ms per replanning step over {rounds} rounds "
          f"(all arms in one process, one replanning step each per round, in turn; host clock around step + device synchronise, after warmup "
          f"and 2 untimed rounds).  Every timed replan of a k arm is warm: {STEPS} - k denoiser steps.")
    print(f"{'num_envs':>8s} {'warm_start':>10s} {'median ms':>10s} {'mean ms':>9s} {'/ cold':>7s} {'(n - k) / n':>11s}")
    for n in SIZES:
        cold = statistics.fmean(res[(n, f"None ({c})")][0] for c in "ab")
        for (nn, name), (med, mean) in res.items():
            if nn == n:
                k = int(name.split()[-1]) if name.startswith("k") else 0
                print(f"{n:8d} {name:>10s} {med:10.3f} {mean:9.3f} {med / cold:7.3f} {(STEPS - k) / STEPS:11.2f}")
        a, b = res[(n, "None (a)")][0], res[(n, "None (b)")][0]
        print(f"{'':8s} same-code spread, None (a) vs None (b): {abs(a - b):.3f} ms = {100 * abs(a - b) / cold:.2f} % of the cold replan")
    if cmp is not None:
        print()
        print("Cold replan (the policy built without the keyword) of the parent commit against this tree's: fresh processes taking turns (the "
              "order within a pair flips every run), the median ms per replanning step of each process")
        for n in SIZES:
            p, t = cmp["parent"][str(n)], cmp["this tree"][str(n)]
            spread = max(max(p) - min(p), max(t) - min(t))
            print(f"{n:8d} parent    " + " ".join(f"{v:7.3f}" for v in p) + f"   median {statistics.median(p):7.3f}")
            print(f"{n:8d} this tree " + " ".join(f"{v:7.3f}" for v in t) + f"   median {statistics.median(t):7.3f}")
            print(f"{'':8s} this tree - parent: {statistics.median(t) - statistics.median(p):+.3f} ms; same-code spread between processes "
                  f"(largest max - min of either tree): {spread:.3f} ms")
    print()
    print("Not measured: what warm-started plans do to task success (no trained checkpoint, no simulator here).")


if __name__ == "__main__":
    main()
