"""Cost of hindsight goal relabelling (data.WindowStream(goal="hindsight"), mode_data_relabel_goals in csrc/data_stream.hip) on the MI355X, in the
protocol of scripts/data_stream_probe.py: B = 128, W = 10, A = 7, G = 512, with CALVIN's cameras (static 200 x 200 and gripper 84 x 84 uint8 ->
224 x 224 bf16, shifts pad 10) and without, a store of ``--episodes`` episodes of 48 .. 80 steps with one goal embedding per step.

  (a) goal="episode"                      ``WindowStream.batch`` as it was: one launch (two with cameras)
  (p) goal="episode", parent commit       the same call through the package and library of a built checkout of the parent commit (``--parent ROOT``),
                                          loaded into this process under another name; left out ("not measured") without ``--parent``
  (b) goal="hindsight", fp32 step_goals   one launch more; horizon 16 .. 48 steps, hindsight_prob 0.5
  (c) goal="hindsight", bf16 step_goals
  (d) (a) + the relabel in torch          the same relabel with torch indexing on the device behind (a): randint, rand, minimum, a row gather, where

Per call: host clock around ``--iters`` back-to-back calls (enqueue) and around them plus a device synchronise (wall); the arms alternate over
``--rounds`` rounds in ONE process, each round starting one arm later than the one before (with a fixed order (a), always right behind (d) and
its temporaries, read 3 us more enqueue than (p) without cameras; taking turns at every place, the two lie inside each other's range); medians of
the rounds and their [min .. max].  Before timing, (a) and (p) are compared bit for bit on one batch.

    python scripts/hindsight_goal_probe.py [--iters 100] [--rounds 10] [--parent ROOT] [--out profiles/hindsight_goals.txt]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import data  # noqa: E402

B, W, A, G = 128, 10, 7, 512
CAMS = ((200, 200), (84, 84))
OUT, PAD = (224, 224), 10
HORIZON, PROB = (16, 48), 0.5


def load_parent(root):
    """The parent commit's package (and, through its _lib, its own libmode_hip.so) under the name ``mode_parent``."""
    path = os.path.join(os.path.abspath(root), "mode_diffusion_policy_amd")
    spec = importlib.util.spec_from_file_location("mode_parent", os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mode_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def build_store(pkg, dev, episodes, cams, step_goal_dtype=None, seed=0):
    """The same episodes for every store (one seed); step_goal_dtype None: a store without step_goals (all the parent commit can hold)."""
    rng = np.random.default_rng(seed)
    st = pkg.data.EpisodeStore(A, G, device=dev) if step_goal_dtype is None else pkg.data.EpisodeStore(A, G, device=dev, step_goal_dtype=step_goal_dtype)
    for _ in range(episodes):
        L = int(rng.integers(48, 81))
        a, g, sg = rng.standard_normal((L, A)).astype(np.float32), rng.standard_normal(G).astype(np.float32), rng.standard_normal((L, G)).astype(np.float32)
        fr = [rng.integers(0, 256, (L, h, w, 3), dtype=np.uint8) for h, w in CAMS] if cams else [None, None]
        if step_goal_dtype is None:
            st.add_episode(a, g, *fr)
        else:
            st.add_episode(a, g, *fr, step_goals=sg)
    return st.finalize("minmax")


def torch_relabel(st, begin64, b):
    """The relabel of mode_data_relabel_goals with torch indexing on the device (its own random draws)."""
    dev = st.device
    idx, ep = b["index"].long(), b["episode"].long()
    last = begin64[ep + 1] - 1
    r = torch.minimum(idx + torch.randint(HORIZON[0], HORIZON[1] + 1, (B,), device=dev), last)
    kind = torch.rand(B, device=dev) < PROB
    b["latent_goal"] = torch.where(kind[:, None], st.step_goals[r].float(), b["latent_goal"])
    b["goal_index"], b["goal_offset"], b["goal_kind"] = r.int(), (r - idx).int(), kind.float()
    return b


def clock(fn, iters):
    """(enqueue us per call, wall us per call) of `iters` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / iters * 1e6, (time.perf_counter() - t0) / iters * 1e6


def section(dev, parent, episodes, iters, rounds, cams, say):
    transforms = lambda pkg: (pkg.CameraTransform(OUT, shift_pad=PAD), pkg.CameraTransform(OUT, shift_pad=PAD)) if cams else None
    kw = lambda pkg: dict(seed=0, pad="hold", camera_transforms=transforms(pkg), frame_dtype=torch.bfloat16)
    st32 = build_store(M, dev, episodes, cams, torch.float32)
    st16 = build_store(M, dev, episodes, cams, torch.bfloat16)
    begin64 = st32.ep_begin.long()
    plain = data.WindowStream(st32, B, W, **kw(M))
    hind32 = data.WindowStream(st32, B, W, goal="hindsight", goal_horizon=HORIZON, hindsight_prob=PROB, **kw(M))
    hind16 = data.WindowStream(st16, B, W, goal="hindsight", goal_horizon=HORIZON, hindsight_prob=PROB, **kw(M))
    arms = {"(a) goal='episode'": lambda i: plain.batch(i)}
    if parent is not None:
        stp = build_store(parent, dev, episodes, cams)
        old = parent.data.WindowStream(stp, B, W, **kw(parent))
        arms["(p) goal='episode', parent commit"] = lambda i: old.batch(i)
        x, y = plain.batch(5), old.batch(5)
        flat = lambda b: {**{k: v for k, v in b.items() if torch.is_tensor(v)}, **{f"{n}.{k}": v for n in ("rgb_obs", "shifts") for k, v in b.get(n, {}).items()}}
        x, y = flat(x), flat(y)
        assert set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x), "goal='episode' differs from the parent commit"
        say(f"   goal='episode' batch(5) vs the parent commit: the same {len(x)} tensors, bit for bit")
    arms["(b) goal='hindsight', fp32 step_goals"] = lambda i: hind32.batch(i)
    arms["(c) goal='hindsight', bf16 step_goals"] = lambda i: hind16.batch(i)
    arms["(d) (a) + the relabel in torch"] = lambda i: torch_relabel(st32, begin64, plain.batch(i))
    for fn in arms.values():
        clock(fn, 5)
    got = {k: [] for k in arms}
    order = list(arms)
    for r in range(rounds):
        for k in order[r % len(order):] + order[: r % len(order)]:
            got[k].append(clock(arms[k], iters))
    S = st32.num_steps
    say(f"\n== batch(): B = {B}, W = {W}, A = {A}, G = {G}, {st32.num_episodes} episodes / {S} steps, horizon {HORIZON[0]} .. {HORIZON[1]}, hindsight_prob {PROB}, "
        f"{'cameras 200 x 200 + 84 x 84 uint8 -> 224 x 224 bf16, shifts pad 10' if cams else 'no cameras'}; us per call, median of {rounds} "
        f"alternating, rotating rounds of {iters} calls [min .. max]")
    say(f"   step_goals: {S} x {G} x 4 = {S * G * 4 / 2 ** 20:.1f} MiB fp32, {S * G * 2 / 2 ** 20:.1f} MiB bf16 on the device")
    say(f"{'variant':42s} {'wall (calls + synchronise)':>36s} {'host enqueue':>34s}")
    for k, v in got.items():
        e, w = [x[0] for x in v], [x[1] for x in v]
        say(f"{k:42s} {statistics.median(w):12.1f} [{min(w):9.1f} .. {max(w):9.1f}] {statistics.median(e):12.1f} [{min(e):9.1f} .. {max(e):9.1f}]")
    if parent is None:
        say(f"{'(p) goal=' + repr('episode') + ', parent commit':42s} not measured (no --parent)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hindsight_goals.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hindsight_goal_probe.py measures on an MI355X: no device found, nothing measured")
    dev = torch.device("cuda:0")
    parent = load_parent(args.parent) if args.parent else None
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"command: python scripts/hindsight_goal_probe.py --iters {args.iters} --rounds {args.rounds} --episodes {args.episodes}"
            f"{' --parent <a built checkout of the parent commit>' if parent is not None else ''}")
        say(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
        for cams in (True, False):
            section(dev, parent, args.episodes, args.iters, args.rounds, cams, say)


if __name__ == "__main__":
    main()
