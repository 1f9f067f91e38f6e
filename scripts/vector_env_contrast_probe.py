"""Cost of a replanning control step of VectorEnvPolicy with forward contrast (C2 geometry, bf16, 10-step DDIM, act_window_size = 10,
multistep = 5, lockstep: every 5th step all environments replan), for num_envs in {1, 8, 32}: candidates=4, candidates=8 (twice: two policies of
the same code, whose difference is the same-code spread) and candidates=4 with contrast=4, whose chunk runs at the batch of candidates=8.  All
arms live in one process and take turns, one replanning step each per round; per replanning step: host clock around step + a device
synchronise, after two untimed rounds (the first captures the arm's chunk).  Median and mean ms over the rounds and the quartiles' distance.

Then the two selection kernels alone at act_window_size x action_dim = 10 x 7 on 32 rows: mode_env_select at N = 8 beside mode_env_select_bid
at (N, M) = (4, 4) - the same 8 rows per environment - and (8, 8); 200 launches between two events, the arms in turn, median over the rounds.

    python scripts/vector_env_contrast_probe.py [rounds] [--out FILE]        -> profiles/vector_env_contrast.txt (or FILE)

Nothing here says what forward contrast does to task success: there is no trained checkpoint and no simulator in this repository."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vector_env_candidates_probe import S, STEPS, W, build, inputs  # noqa: E402

SIZES = (1, 8, 32)
ARMS = [("N = 4", dict(candidates=4)), ("N = 8 (a)", dict(candidates=8)), ("N = 8 (b)", dict(candidates=8)),
        ("N = 4, M = 4", dict(candidates=4, contrast=4))]
LAUNCHES, KROWS, A = 200, 32, 7


def measure(arms, rounds):
    """One replanning step of every arm per round, in turn (the S - 1 steps behind it untimed).  Returns {name: [ms per round]}."""
    import time
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
    return ts


def kernels(dev, rounds):
    """us per launch of the two selection kernels on KROWS rows with previous plans: {name: [us per round]}."""
    import torch
    from mode_diffusion_policy_amd import _lib as L
    from mode_diffusion_policy_amd import rollout
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(2)
    n = KROWS
    prev = torch.randn(n, W, A, generator=g).to(dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    mask = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    wt = torch.from_numpy(rollout.coherence_weights(0.5, W - S)).to(dev)
    lam = torch.ones(1, device=dev)
    keep, calls = [], {}
    for name, N, M in (("mode_env_select N = 8", 8, 0), ("mode_env_select_bid (4, 4)", 4, 4), ("mode_env_select_bid (8, 8)", 8, 8)):
        chunk = torch.randn(n, N + M, W, A, generator=g).to(dev)
        out = [torch.empty(n, W, A, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, N, device=dev),
               torch.empty(n, N + M, device=dev), torch.empty(n, N, device=dev)]
        base = dict(rows=rows.data_ptr(), has_prev=mask.data_ptr(), count=None, chunk=chunk.data_ptr(), plan=prev.data_ptr(), weights=wt.data_ptr(),
                    chosen=out[0].data_ptr(), selected=out[1].data_ptr(), scores=out[2].data_ptr(), m_b=n, num_envs=n, W=W, A=A, shift=S, N=N)
        if M:
            d = L.ModeEnvBidDesc(lambda_=lam.data_ptr(), bc=out[3].data_ptr(), fc=out[4].data_ptr(), M=M, K=min(N, M), **base)
            calls[name] = (lib.mode_env_select_bid, d)
        else:
            d = L.ModeEnvSelectDesc(**base)
            calls[name] = (lib.mode_env_select, d)
        keep.append((chunk, out))
    ts = {name: [] for name in calls}
    for r in range(rounds + 2):
        for name, (fn, d) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                L.check(fn(C.byref(d), stream), name)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ts[name].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return ts


def _iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if args and args[0].isdigit() else 60
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "vector_env_contrast.txt")
    import torch
    import bench
    from mode_diffusion_policy_amd import rollout
    dev = torch.device("cuda:0")
    den = build(dev)
    arms = {}
    for n in SIZES:
        st, goal = inputs(dev, n)
        for name, kw in ARMS:
            pol = rollout.VectorEnvPolicy(den, n, act_window_size=W, multistep=S, action_dim=7, sigma_max=80.0, num_sampling_steps=STEPS, **kw)
            arms[(n, name)] = (pol, st, goal)
    res = measure(arms, rounds)
    C2 = bench.C2
    lines = [f"Replanning control step of VectorEnvPolicy with forward contrast, C2 geometry (D {C2['embed_dim']}, {C2['n_layers']} layers, "
             f"{C2['num_experts']} experts, top-{C2['top_k']}), bf16, {STEPS}-step DDIM, act_window_size = {W}, multistep = {S}, lockstep; ms per "
             f"replanning step over {rounds} rounds (all arms in one process, one replanning step each per round, in turn; host clock around step + "
             f"device synchronise, after 2 untimed rounds).  'N = 8 (a)' and '(b)' are two policies of the same code.  'N = 4, M = 4': candidates=4, "
             f"contrast=4 (contrast_weight 1, contrast_topk 4), the chunk batch of candidates=8; every timed replan has a previous plan.",
             f"{'num_envs':>8s} {'arm':>13s} {'chunk batch':>11s} {'median ms':>10s} {'mean ms':>9s} {'q3 - q1':>8s} {'/ N = 8':>8s}"]
    for n in SIZES:
        med = {name: statistics.median(res[(n, name)]) for name, _ in ARMS}
        base = (med["N = 8 (a)"] + med["N = 8 (b)"]) / 2
        for name, kw in ARMS:
            v = res[(n, name)]
            rows_per = kw["candidates"] + kw.get("contrast", 0)
            lines.append(f"{n:8d} {name:>13s} {n * rows_per:11d} {med[name]:10.3f} {statistics.fmean(v):9.3f} {_iqr(v):8.3f} {med[name] / base:8.3f}")
        spread = abs(med["N = 8 (a)"] - med["N = 8 (b)"])
        diff = med["N = 4, M = 4"] - base
        lines.append(f"{'':8s} same-code spread, N = 8 (a) vs (b): {spread:.3f} ms = {100 * spread / base:.2f} %;  (4, 4) - mean of N = 8: {diff:+.3f} ms "
                     f"= {100 * diff / base:+.2f} %")
    kt = kernels(dev, rounds)
    lines += ["", f"The selection kernels alone, {KROWS} rows of {W} x {A} with previous plans, shift {S}: us per launch, {LAUNCHES} launches between two "
              f"events, the arms in turn, over {rounds} rounds after 2 untimed.",
              f"{'kernel':>28s} {'median us':>10s} {'mean us':>9s} {'q3 - q1':>8s}"]
    for name, v in kt.items():
        lines.append(f"{name:>28s} {statistics.median(v):10.3f} {statistics.fmean(v):9.3f} {_iqr(v):8.3f}")
    lines += ["", "Not measured: what forward contrast does to task success (no trained checkpoint, no simulator here)."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
