"""GPU: mode_data_relabel_goals through ctypes and through data.WindowStream / data.WindowSweep(goal="hindsight") against the numpy restatement of
include/mode_hip.h (tests/goal_refs.py).  Everything the kernel does is an integer draw or a copy: every comparison is bit equality.

latent_goal [B, G] is contiguous in the descriptor (there is no row stride), so the sentinels around it are the canary rows of hip_helpers.Guarded
before and after it, and - in the unaligned cases - a buffer in which it starts one element in: sentinel elements directly before its first and
after its last column, which also takes the kernel off its 16-byte path."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import goal_refs as GR  # noqa: E402
import hip_helpers as H  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import data  # noqa: E402
from oracle.weights import make_inputs  # noqa: E402
from test_gpu_train import build_train  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
W = 4
LENGTHS = GR.episode_lengths(W)                                                  # 1, 3, 4, 7: 15 steps
BEGIN = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
S, E = int(BEGIN[-1]), len(LENGTHS)
SEED, STEP = 11, 5
HORIZONS = ((0, 0), (1, 1), (0, 6), (3, 9), (GR.LAST, GR.LAST))
THRESHES = (0, 2 ** 31, 2 ** 32)
SENTINEL = -77
_ROWS = {}


def rows(B):
    """index, episode [B] int32 of the stream's batch (pad="hold") on the test store, and an ids table with values on both sides of 2^31."""
    if B not in _ROWS:
        b = R.sample_windows(R.make_store(W, 3, 5, seed=2), W, B, SEED, STEP, "hold")
        ids = ((np.arange(B, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(0x7FFFFFFE)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        _ROWS[B] = (b["index"], b["episode"], ids)
    return _ROWS[B]


def step_goal_bits(G, bf16):
    """[S, G] stored bits (uint32 | uint16) with a NaN payload, -0, a denormal and an infinity among them, and the fp32 rows a copy must give."""
    x = np.concatenate(GR.step_goal_table(R.make_store(W, 3, G, seed=2), G))
    if bf16:
        bits = GR.bf16_bits(x)
        for i, v in enumerate((0x7FC1, 0x8000, 0x0001, 0x7F80, 0xFF80)):
            bits[(3 * i + 2) % S, (5 * i) % G] = v
        return bits, GR.bf16_expand(bits)
    bits = x.view(np.uint32).copy()
    for i, v in enumerate((0x7FC00123, 0x80000000, 0x00000001, 0x7F800000, 0xFFFFFFFF)):
        bits[(3 * i + 2) % S, (5 * i) % G] = v
    return bits, bits.view(np.float32)


def ints(n):
    return torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")


def ints_intact(t):
    return bool((t[:4] == SENTINEL).all()) and bool((t[-4:] == SENTINEL).all())


class Case:
    """The device side of one (G, dtype): the store's tables and, per launch, the pre-filled latent_goal and the sentinel-framed outputs."""

    def __init__(self, G, bf16, src_off=0):
        self.G, self.bf16 = G, bf16
        bits, self.expanded = step_goal_bits(G, bf16)
        flat = torch.from_numpy(bits.view(np.int16 if bf16 else np.int32).reshape(-1))
        self.src = torch.zeros(flat.numel() + 16, dtype=flat.dtype, device="cuda")       # src_off elements in: off the 16-byte alignment
        self.src[src_off: src_off + flat.numel()].copy_(flat)
        self.src_ptr = self.src.data_ptr() + src_off * flat.element_size()
        assert self.src.data_ptr() % 16 == 0
        self.ep_begin = torch.from_numpy(BEGIN.astype(np.int32)).cuda()
        self.goals = np.random.default_rng(G).standard_normal((E, G)).astype(np.float32)

    def launch(self, B, lo, hi, thresh, use_ids, dst_off=0, skip=None, seed=SEED, step=STEP, over=None):
        """-> (status, desc outputs as numpy, sentinels intact, ref); over: descriptor fields set after everything was sized for the good one."""
        index, episode, ids = rows(B)
        G = self.G
        pre = self.goals[episode]
        if dst_off:
            buf = torch.full((B * G + 32,), H.CANARY, dtype=torch.float32, device="cuda")
            lg = buf[16 + dst_off: 16 + dst_off + B * G].view(B, G)
            intact = lambda: bool((buf[: 16 + dst_off] == H.CANARY).all()) and bool((buf[16 + dst_off + B * G:] == H.CANARY).all())
        else:
            g = H.Guarded(B, G)
            lg, intact = g.t, g.intact
        lg.copy_(torch.from_numpy(pre))
        out = dict(goal_index=ints(B), goal_offset=ints(B), goal_kind=torch.full((B + 8,), float(SENTINEL), device="cuda"))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        t_index, t_episode, t_ids = dev(index), dev(episode), dev(ids.view(np.int32))
        d = L.ModeDataGoalDesc(step_goals=self.src_ptr, ep_begin=H.p(self.ep_begin), index=H.p(t_index), episode=H.p(t_episode),
                               ids=H.p(t_ids) if use_ids else None, thresh=thresh, goal_dtype=L.MODE_BF16 if self.bf16 else L.MODE_F32, S=S, E=E, G=G, B=B,
                               seed=seed, step=step, lo=lo, hi=hi, latent_goal=lg.data_ptr(),
                               **{k: None if k == skip else v[4:].data_ptr() for k, v in out.items()})
        for k, v in (over or {}).items():
            setattr(d, k, v)
        rc = L.load().mode_data_relabel_goals(C.byref(d), H.stream())
        torch.cuda.synchronize()
        got = {k: v[4:-4].cpu().numpy() for k, v in out.items()}
        got["latent_goal"] = lg.cpu().numpy()
        ok = intact() and ints_intact(out["goal_index"]) and ints_intact(out["goal_offset"]) and \
            bool((out["goal_kind"][:4] == SENTINEL).all()) and bool((out["goal_kind"][-4:] == SENTINEL).all())
        ref = GR.relabel(BEGIN, index, episode, seed, step, lo, hi, thresh, ids=ids if use_ids else None)
        ref["latent_goal"] = GR.relabelled_goals(pre, self.expanded, ref)
        ref["pre"] = pre
        return rc, got, ok, ref


def check(got, ref, what, skip=None):
    for k in ("goal_index", "goal_offset", "goal_kind"):
        if k == skip:
            assert (got[k] == SENTINEL).all(), (what, k)                                  # an absent output is not written
        else:
            assert R.same_bits(got[k], ref[k]), (what, k)
    assert R.same_bits(got["latent_goal"], ref["latent_goal"]), (what, "latent_goal")
    off = ref["goal_kind"] == 0
    assert R.same_bits(got["latent_goal"][off], ref["pre"][off]), (what, "rows that keep their episode goal")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("G", [1, 5, 8, 512, 4096])
def test_relabel_matches_the_reference_bit_for_bit(G, bf16):
    c = Case(G, bf16)
    relabelled = kept = 0
    for B in (1, 7, 130):
        for use_ids in (False, True):
            for lo, hi in HORIZONS:
                for thresh in THRESHES:
                    what = f"G={G} bf16={bf16} B={B} ids={use_ids} horizon=({lo}, {hi}) thresh={thresh}"
                    rc, got, ok, ref = c.launch(B, lo, hi, thresh, use_ids)
                    assert rc == 0 and ok, what
                    check(got, ref, what)
                    n = int(ref["goal_kind"].sum())
                    assert n == (0 if thresh == 0 else B if thresh == 2 ** 32 else n)
                    relabelled += n
                    kept += B - n
                    if thresh == 2 ** 32 and lo == GR.LAST:
                        assert np.array_equal(got["goal_index"], BEGIN[rows(B)[1].astype(np.int64) + 1] - 1), what
    assert relabelled > 0 and kept > 0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("G", [1, 5, 8, 512])
def test_unaligned_tables_take_the_element_path(G, bf16):
    """step_goals or latent_goal one element off a 16-byte boundary: the same bits, and the elements directly around latent_goal stay."""
    for src_off, dst_off in ((1, 0), (0, 1), (1, 3)):
        c = Case(G, bf16, src_off=src_off)
        for lo, hi in HORIZONS:
            what = f"G={G} bf16={bf16} src+{src_off} dst+{dst_off} horizon=({lo}, {hi})"
            rc, got, ok, ref = c.launch(7, lo, hi, 2 ** 31, False, dst_off=dst_off)
            assert rc == 0 and ok, what
            check(got, ref, what)


def test_every_optional_output_may_be_absent():
    for bf16 in (False, True):
        c = Case(8, bf16)
        for skip in ("goal_index", "goal_offset", "goal_kind"):
            rc, got, ok, ref = c.launch(7, 0, 6, 2 ** 31, True, skip=skip)
            assert rc == 0 and ok
            check(got, ref, f"without {skip}", skip=skip)


def test_a_row_is_a_function_of_seed_step_and_id():
    c = Case(8, False)
    _, g7, _, _ = c.launch(7, 0, 6, 2 ** 31, False)
    _, g130, _, _ = c.launch(130, 0, 6, 2 ** 31, False)
    for k in g7:
        assert R.same_bits(g7[k], g130[k][:7]), k                                        # rows [:7] of B = 130 == the B = 7 launch
    _, other, _, ref = c.launch(130, 0, 6, 2 ** 31, False, step=STEP + 1)
    assert not np.array_equal(other["goal_offset"], g130["goal_offset"]) and not np.array_equal(other["goal_kind"], g130["goal_kind"])
    check(other, ref, "step + 1")
    _, wrap, ok, ref = c.launch(130, 0, 6, 2 ** 31, True, seed=2 ** 32 - 5, step=2 ** 32 - 1)       # seed + 4, seed + 5 and step + 1 wrap modulo 2^32
    assert ok
    check(wrap, ref, "wrapping keys")


def test_a_store_past_two_to_the_31_elements():
    """One episode of 2^19 + 8 steps, G = 4096, bf16 (4.3 GB): the goal rows' element offsets pass 2^31."""
    G, B, S_big = 4096, 3, 2 ** 19 + 8
    table = torch.empty(S_big, G, dtype=torch.bfloat16, device="cuda")
    tail = torch.randn(8, G, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(torch.bfloat16)
    table[-8:] = tail
    begin = torch.tensor([0, S_big], dtype=torch.int32, device="cuda")
    index = torch.tensor([S_big - 8, S_big - 6, S_big - 3], dtype=torch.int32, device="cuda")
    episode = torch.zeros(B, dtype=torch.int32, device="cuda")
    lg, gi = H.Guarded(B, G), ints(B)
    d = L.ModeDataGoalDesc(step_goals=table.data_ptr(), ep_begin=begin.data_ptr(), index=index.data_ptr(), episode=episode.data_ptr(), ids=None,
                           thresh=2 ** 32, goal_dtype=L.MODE_BF16, S=S_big, E=1, G=G, B=B, seed=0, step=0, lo=4, hi=4, latent_goal=lg.t.data_ptr(),
                           goal_index=gi[4:].data_ptr(), goal_offset=None, goal_kind=None)
    assert L.load().mode_data_relabel_goals(C.byref(d), H.stream()) == 0
    torch.cuda.synchronize()
    assert lg.intact() and ints_intact(gi) and gi[4:-4].tolist() == [S_big - 4, S_big - 2, S_big - 1]
    assert torch.equal(lg.t, tail[[4, 6, 7]].float())
    del table
    torch.cuda.empty_cache()


def test_bad_descriptors_are_refused_before_any_launch():
    c = Case(8, False)
    lib = L.load()
    assert lib.mode_data_relabel_goals(None, H.stream()) == BAD_ARG
    cases = [(dict(**{k: None}), BAD_ARG) for k in ("step_goals", "ep_begin", "index", "episode", "latent_goal")]
    cases += [(dict(**{k: v}), BAD_ARG) for k in ("S", "E", "G", "B") for v in (0, -1)]
    cases += [(dict(E=S + 1), BAD_ARG), (dict(lo=-1), BAD_ARG), (dict(lo=4, hi=3), BAD_ARG), (dict(thresh=2 ** 32 + 1), BAD_ARG), (dict(thresh=2 ** 64 - 1), BAD_ARG),
              (dict(goal_dtype=2), BAD_ARG), (dict(goal_dtype=-1), BAD_ARG), (dict(B=65536), UNSUPPORTED), (dict(G=4097), UNSUPPORTED)]
    for over, want in cases:
        rc, got, ok, ref = c.launch(7, 0, 6, 2 ** 32, True, over=over)
        assert rc == want and ok, over
        assert R.same_bits(got["latent_goal"], ref["pre"]) and all((got[k] == SENTINEL).all() for k in ("goal_index", "goal_offset", "goal_kind")), over
    rc, got, ok, ref = c.launch(7, 0, 6, 2 ** 32, True)                               # the descriptor these were derived from is a good one
    assert rc == 0 and ok and not R.same_bits(got["latent_goal"], ref["pre"])


# ---------------------------------------------------------------------------------------------------------------- data.py, end to end
WE, AE, BE = 10, 7, 8


def e2e_store(G, dtype=torch.float32, step_goals=True):
    eps = R.make_store(WE, AE, G, seed=3)                                          # episodes of 1, 9, 10 and 13 steps
    sg = GR.step_goal_table(eps, G)
    st = data.EpisodeStore(AE, G, step_goal_dtype=dtype)
    for e, s in zip(eps, sg):
        st.add_episode(e[0], e[1], step_goals=s if step_goals else None)
    return eps, np.concatenate(sg), st.finalize("minmax")


@pytest.fixture(scope="module")
def tiny():
    cfg, sd, m = build_train("c1e4", 210, "bf16")
    return cfg, m, M.GCDenoiser(m, 0.5).train()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_hindsight_stream_batch_equals_the_reference(dtype):
    G, seed, t = 512, 7, 3
    eps, sg, st = e2e_store(G, dtype)
    assert st.step_goals.dtype == dtype and tuple(st.step_goals.shape) == (33, G)
    if dtype == torch.bfloat16:
        sg = GR.bf16_expand(GR.bf16_bits(sg))
    stream = data.WindowStream(st, BE, WE, seed=seed, goal="hindsight", goal_horizon=(0, 6), hindsight_prob=0.5)
    b = stream.batch(t)
    lo, hi, scale = R.minmax(eps)
    base = R.sample_windows(eps, WE, BE, seed, t, "hold", (lo, scale))
    begin = np.concatenate([[0], np.cumsum(R.episode_lengths(WE))])
    ref = GR.relabel(begin, base["index"], base["episode"], seed, t, 0, 6, 2 ** 31)
    assert 0 < ref["goal_kind"].sum() < BE                                           # this batch mixes both kinds of goal
    for k in ("index", "episode", "action_mask"):
        assert np.array_equal(b[k].cpu().numpy(), base[k]), k
    for k in ("goal_index", "goal_offset", "goal_kind"):
        assert b[k].shape == (BE,) and R.same_bits(b[k].cpu().numpy(), ref[k]), k
    assert b["goal_index"].dtype == torch.int32 and b["goal_offset"].dtype == torch.int32 and b["goal_kind"].dtype == torch.float32
    assert R.same_bits(b["latent_goal"].cpu().numpy(), GR.relabelled_goals(base["latent_goal"], sg, ref))
    on = b["goal_kind"] == 1
    assert torch.equal(b["latent_goal"][on], st.step_goals[b["goal_index"][on].long()].float())
    assert torch.equal(b["latent_goal"][~on], st.goals[b["episode"][~on].long()])
    # batch(t) asked twice, and out of order
    later, again = stream.batch(t + 4), stream.batch(t)
    fresh = data.WindowStream(st, BE, WE, seed=seed, goal="hindsight", goal_horizon=(0, 6), hindsight_prob=0.5).batch(t)
    assert set(again) == set(b) == set(fresh)
    for k in b:
        assert torch.equal(again[k], b[k]) and torch.equal(fresh[k], b[k]), k
    assert not torch.equal(later["goal_offset"], b["goal_offset"])


def test_training_steps_on_a_hindsight_batch_give_finite_losses(tiny):
    cfg, m, den = tiny
    eps, sg, st = e2e_store(cfg.goal_dim)
    stream = data.WindowStream(st, BE, WE, seed=7, goal="hindsight", goal_horizon=(0, 6), hindsight_prob=0.5)
    img = make_inputs(cfg, BE, 31)["state_images"].cuda()
    for t in (3, 4):
        b = stream.batch(t)
        sig = M.utils.rand_log_logistic((BE,), loc=float(np.log(0.5)), scale=0.5, min_value=1e-3, max_value=80.0, u=b["u"])
        total, act, _ = M.training_step(den, {"vis": {"perceptual_emb": {"state_images": img}, "latent_goal": b["latent_goal"], "actions": b["actions"],
                                                      "action_mask": b["action_mask"], "noise": b["noise"], "sigmas": sig}})
        total.backward()
        assert torch.isfinite(total) and float(total) > 0
    m.zero_grad(set_to_none=True)


def test_validator_on_a_hindsight_sweep_of_the_last_step(tiny):
    cfg, m, den = tiny
    eps, sg, st = e2e_store(cfg.goal_dim)
    feats = torch.randn(st.num_steps, cfg.n_img_tokens, cfg.obs_dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    embed = lambda b: {"state_images": feats[b["index"].long()]}
    sweep = data.WindowSweep(st, BE, WE, seed=5, goal="hindsight", goal_horizon="last")
    val = M.Validator(den, sweep, embed)
    res = val.run()
    assert torch.isfinite(res["mse"]) and float(res["mse"]) > 0
    seen = {}
    for i in range(len(val)):
        b = val.batch(i)
        last = st.ep_begin.long()[b["episode"].long() + 1] - 1
        assert torch.equal(b["goal_index"].long(), last) and bool((b["goal_kind"] == 1).all())       # padding rows too
        assert torch.equal(b["goal_offset"], (last - b["index"].long()).int())
        assert torch.equal(b["latent_goal"], st.step_goals[last])
        for g, r in zip(b["window"].tolist(), b["goal_index"].tolist()):
            seen[g] = r
    # a window's goal belongs to the window: the same at another batch size, with a drawn horizon and a drawn kind
    per = []
    for B in (3, 8):
        sw = data.WindowSweep(st, B, WE, seed=5, goal="hindsight", goal_horizon=(0, 6), hindsight_prob=0.5)
        got = {}
        for i in range(len(sw)):
            b = sw.batch(i, draw=2)
            for j, g in enumerate(b["window"].tolist()):
                row = (int(b["goal_index"][j]), float(b["goal_kind"][j]), b["latent_goal"][j].cpu().numpy().tobytes())
                assert got.setdefault(g, row) == row
        per.append(got)
    assert per[0] == per[1] and len(per[0]) == 33 and len({v[1] for v in per[0].values()}) == 2
    assert den.training


def test_episode_goal_stream_ignores_step_goals():
    """goal="episode" on a store WITH step_goals: exactly the keys and bits of the same store built without them."""
    _, _, with_sg = e2e_store(512)
    _, _, without = e2e_store(512, step_goals=False)
    assert without.step_goals is None
    a, b = data.WindowStream(with_sg, BE, WE, seed=7).batch(3), data.WindowStream(without, BE, WE, seed=7).batch(3)
    assert set(a) == set(b) == {"actions", "action_mask", "latent_goal", "index", "episode", "noise", "u"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = data.WindowSweep(with_sg, BE, WE, seed=7).batch(1), data.WindowSweep(without, BE, WE, seed=7).batch(1)
    assert set(a) == set(b) and "goal_index" not in a and all(torch.equal(a[k], b[k]) for k in a)
