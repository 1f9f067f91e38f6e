"""Cost of the ordered draws of the training batch stream (data.WindowStream(order="epoch") / (episode_weights=),
mode_data_sample_windows_ordered in csrc/data_stream.hip) on the MI355X, in the protocol of scripts/data_stream_probe.py: B = 128, W = 10, A = 7,
G = 512, a store of ``--episodes`` episodes of 48 .. 80 steps (2344 of them: about 150 k steps), with CALVIN's cameras (static 200 x 200 and
gripper 84 x 84 uint8 -> 224 x 224 bf16, shifts pad 10) and without.  The frames of every episode are slices of one random 80-step clip: the host
never holds 21 GB, the device does.

  (a) defaults                            ``WindowStream.batch`` as it was: ``mode_data_sample_windows`` (two launches with cameras)
  (p) defaults, parent commit             the same call through the package and library of a built checkout of the parent commit (``--parent ROOT``),
                                          loaded into this process under another name; left out ("not measured") without ``--parent``
  (e) order="epoch"                       ``mode_data_sample_windows_ordered`` in place of that launch; two int64 [B] outputs more
  (w) episode_weights                     the same entry point; four groups of episodes mixed 4 : 3 : 2 : 1 (``data.mixture_weights``)

Per call: host clock around ``--iters`` back-to-back calls (enqueue) and around them plus a device synchronise (wall); the arms alternate over
``--rounds`` rounds in ONE process, each round starting one arm later than the one before; medians of the rounds and their [min .. max].  Before
timing, (a) and (p) are compared bit for bit on one batch, and one epoch of (e) is checked to visit every window once.

    python scripts/sample_order_probe.py [--iters 100] [--rounds 10] [--episodes 2344] [--parent ROOT] [--out profiles/sample_order.txt]"""
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
GROUP_WEIGHTS = (4.0, 3.0, 2.0, 1.0)


def load_parent(root):
    """The parent commit's package (and, through its _lib, its own libmode_hip.so) under the name ``mode_parent``."""
    path = os.path.join(os.path.abspath(root), "mode_diffusion_policy_amd")
    spec = importlib.util.spec_from_file_location("mode_parent", os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mode_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def build_store(pkg, dev, episodes, cams, seed=0):
    """The same episodes for every store (one seed)."""
    rng = np.random.default_rng(seed)
    clip = [rng.integers(0, 256, (80, h, w, 3), dtype=np.uint8) for h, w in CAMS] if cams else None
    st = pkg.data.EpisodeStore(A, G, device=dev)
    for _ in range(episodes):
        L = int(rng.integers(48, 81))
        a, g = rng.standard_normal((L, A)).astype(np.float32), rng.standard_normal(G).astype(np.float32)
        st.add_episode(a, g, *([c[80 - L:] for c in clip] if cams else [None, None]))
    return st.finalize("minmax")


def clock(fn, iters):
    """(enqueue us per call, wall us per call) of `iters` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / iters * 1e6, (time.perf_counter() - t0) / iters * 1e6


def flat(b):
    return {**{k: v for k, v in b.items() if torch.is_tensor(v)}, **{f"{n}.{k}": v for n in ("rgb_obs", "shifts") for k, v in b.get(n, {}).items()}}


def section(dev, parent, episodes, iters, rounds, cams, say):
    transforms = lambda pkg: (pkg.CameraTransform(OUT, shift_pad=PAD), pkg.CameraTransform(OUT, shift_pad=PAD)) if cams else None
    kw = lambda pkg: dict(seed=0, pad="hold", camera_transforms=transforms(pkg), frame_dtype=torch.bfloat16)
    st = build_store(M, dev, episodes, cams)
    S, n = st.num_steps, st.num_steps
    say(f"\n== batch(): B = {B}, W = {W}, A = {A}, G = {G}, {st.num_episodes} episodes / {S} steps (n = {n} window starts, {n / B:.1f} steps per epoch), "
        f"{'cameras 200 x 200 + 84 x 84 uint8 -> 224 x 224 bf16, shifts pad 10' if cams else 'no cameras'}; us per call, median of {rounds} "
        f"alternating, rotating rounds of {iters} calls [min .. max]")
    plain = data.WindowStream(st, B, W, **kw(M))
    epoch = data.WindowStream(st, B, W, order="epoch", **kw(M))
    groups = np.arange(st.num_episodes) % len(GROUP_WEIGHTS)
    mixed = data.WindowStream(st, B, W, episode_weights=data.mixture_weights(st, groups, GROUP_WEIGHTS), **kw(M))
    arms = {"(a) defaults": lambda i: plain.batch(i)}
    if parent is not None:
        stp = build_store(parent, dev, episodes, cams)
        old = parent.data.WindowStream(stp, B, W, **kw(parent))
        arms["(p) defaults, parent commit"] = lambda i: old.batch(i)
        x, y = flat(plain.batch(5)), flat(old.batch(5))
        assert set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x), "the default batch differs from the parent commit"
        say(f"   defaults, batch(5) vs the parent commit: the same {len(x)} tensors, bit for bit")
    arms['(e) order="epoch"'] = lambda i: epoch.batch(i)
    arms["(w) episode_weights, 4 groups 4 : 3 : 2 : 1"] = lambda i: mixed.batch(i)
    # one epoch of (e), without the cameras' launch: every window start once
    bare = data.WindowStream(st, B, W, seed=0, order="epoch", noise=False)
    bs = [bare.batch(t) for t in range((2 * n - 1) // B + 1)]
    index, ep = torch.cat([b["index"] for b in bs]), torch.cat([b["epoch"] for b in bs])
    for e in (0, 1):
        assert torch.equal(torch.sort(index[ep == e]).values, torch.arange(n, device=dev, dtype=torch.int32)), "an epoch misses or repeats a window"
    say(f"   order=\"epoch\": epochs 0 and 1 visit each of the {n} starts exactly once")
    drawn = torch.cat([mixed.batch(t)["episode"] for t in range(200)]).cpu().numpy()
    share = np.bincount(groups[drawn], minlength=len(GROUP_WEIGHTS)) / drawn.size
    say(f"   episode_weights: group shares of {drawn.size} draws {', '.join(f'{s:.3f}' for s in share)} (asked: "
        f"{', '.join(f'{w / sum(GROUP_WEIGHTS):.3f}' for w in GROUP_WEIGHTS)})")
    for fn in arms.values():
        clock(fn, 5)
    got = {k: [] for k in arms}
    order = list(arms)
    for r in range(rounds):
        for k in order[r % len(order):] + order[: r % len(order)]:
            got[k].append(clock(arms[k], iters))
    say(f"{'variant':46s} {'wall (calls + synchronise)':>36s} {'host enqueue':>34s}")
    for k, v in got.items():
        e, w = [x[0] for x in v], [x[1] for x in v]
        say(f"{k:46s} {statistics.median(w):12.1f} [{min(w):9.1f} .. {max(w):9.1f}] {statistics.median(e):12.1f} [{min(e):9.1f} .. {max(e):9.1f}]")
    if parent is None:
        say(f"{'(p) defaults, parent commit':46s} not measured (no --parent)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=2344)
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_order.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_order_probe.py measures on an MI355X: no device found, nothing measured")
    dev = torch.device("cuda:0")
    parent = load_parent(args.parent) if args.parent else None
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"command: python scripts/sample_order_probe.py --iters {args.iters} --rounds {args.rounds} --episodes {args.episodes}"
            f"{' --parent <a built checkout of the parent commit>' if parent is not None else ''}")
        say(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
        for cams in (False, True):
            section(dev, parent, args.episodes, args.iters, args.rounds, cams, say)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
