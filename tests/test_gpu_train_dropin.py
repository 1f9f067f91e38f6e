"""GPU: the training side of the drop-in boundary.

The reference's ``training_step`` feeds the denoiser ``perceptual_emb`` straight from TRAINABLE FiLM-ResNets (mode/models/mode_agent.py:404-411,
548-567) and is wrapped by Lightning in torch ``DistributedDataParallel(find_unused_parameters=True)`` (mode/training_calvin.py:92-103).  So the
HIP backward must (1) return d state_images / d goals, (2) hand the parameter gradients to autograd so that accumulate hooks fire.  Checked
here against the oracle's autograd (the oracle is a differentiable functional restatement: input gradients come for free there).

Tolerances: fp32 compute mode 2e-3 per tensor (observed ~1e-5); bf16: DESIGN §5's stated gradient tolerance (4e-2 per tensor, the reference's
own fp32-vs-autocast gap)."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import get_config, make_inputs, make_state_dict  # noqa: E402
from test_gpu_train import BF16_GRAD_TOL, build_train, rel  # noqa: E402


def _encoder(cfg, raw_dim, seed):
    """A trainable stand-in for the perceptual encoders: raw features -> (B, n_img, obs_dim) tokens."""
    torch.manual_seed(seed)
    enc = torch.nn.Linear(raw_dim, cfg.n_img_tokens * cfg.obs_dim)
    with torch.no_grad():
        enc.weight.mul_(3.0)
    return enc


@pytest.mark.parametrize("cfgname,B,dtype,goal_route", [("c1e4", 8, "fp32", False), ("c1e4", 8, "bf16", False), ("c1e4", 8, "fp32", True),
                                                        ("c1e4", 8, "bf16", True), ("c2block", 128, "fp32", False), ("c2block", 128, "bf16", False)])
def test_input_gradients_through_trainable_encoder_vs_oracle(cfgname, B, dtype, goal_route):
    """state_images produced by a trainable encoder, goals requiring grad: the encoder's weight gradients, d state_images and d goals of the HIP
    chain against the oracle's autograd (with use_goal_in_routing the goal gradient also runs through the conditioning / router path)."""
    cfg, sd, m = build_train(cfgname, 210, dtype, use_goal_in_routing=goal_route)
    cfg.use_goal_in_routing = goal_route
    raw_dim = 24
    inp = make_inputs(cfg, B, 77)
    raw = torch.from_numpy(np.random.RandomState(5).standard_normal((B, raw_dim)).astype(np.float32))
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(3))
    # ---- oracle (CPU autograd)
    enc_ref = _encoder(cfg, raw_dim, 1)
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    img_ref = enc_ref(raw).view(B, cfg.n_img_tokens, cfg.obs_dim)
    img_ref.retain_grad()
    goal_ref = inp["goals"].clone().requires_grad_(True)
    ref_loss, _ = O.denoiser_loss(sdg, cfg, 0.5, img_ref, inp["actions"], goal_ref, inp["noise"], sig)
    ref_loss.backward()
    # ---- HIP chain behind autograd (default grad_mode: every gradient goes through autograd)
    enc = _encoder(cfg, raw_dim, 1).cuda()
    den = M.GCDenoiser(m, 0.5).train()
    img = enc(raw.cuda()).view(B, cfg.n_img_tokens, cfg.obs_dim)
    img.retain_grad()
    goal = inp["goals"].cuda().requires_grad_(True)
    loss, _ = den.loss({"state_images": img}, inp["actions"].cuda(), goal, inp["noise"].cuda(), sig.cuda())
    loss.backward()
    tol_l, tol = (1e-4, 2e-3) if dtype == "fp32" else (1e-2, BF16_GRAD_TOL)
    assert abs(float(loss) - float(ref_loss)) < tol_l * abs(float(ref_loss))
    errs = dict(d_img=rel(img.grad, img_ref.grad), d_goal=rel(goal.grad, goal_ref.grad), enc_w=rel(enc.weight.grad, enc_ref.weight.grad),
                enc_b=rel(enc.bias.grad, enc_ref.bias.grad), tok_w=rel(m.tok_emb.weight.grad, sdg["tok_emb.weight"].grad))
    print(f"{cfgname} B={B} {dtype} goal_route={goal_route}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert float(img_ref.grad.norm()) > 0 and float(goal_ref.grad.norm()) > 0
    for k, v in errs.items():
        assert v < tol, (k, v)


def test_goal_gradient_passes_through_the_goal_mask():
    """goal_drop > 0: the element-wise Bernoulli mask of preprocess_goals (modedit.py:882-893) is part of the autograd graph - masked elements get
    an exactly zero gradient, the others the chain's d goals."""
    cfg, sd, m = build_train("c1e4", 210, "fp32", goal_drop=0.5)
    inp = {k: v.cuda() for k, v in make_inputs(cfg, 8, 3).items()}
    goal = inp["goals"].clone().requires_grad_(True)
    torch.manual_seed(4)
    F = m({"state_images": inp["state_images"]}, inp["actions"], goal, torch.full((8,), 0.7, device="cuda"))
    torch.manual_seed(4)
    mask = torch.bernoulli(torch.full_like(inp["goals"], 0.5))                  # the draw preprocess_goals made
    F.square().mean().backward()
    assert float(goal.grad.abs().max()) > 0
    assert float((goal.grad * mask).abs().max()) == 0.0 and float((goal.grad * (1 - mask)).abs().min()) >= 0.0
    assert int((goal.grad != 0).sum()) == int((mask == 0).sum())


def _two_losses(den, inp, sig):
    a = den.loss({"state_images": inp["state_images"][:8]}, inp["actions"][:8], inp["goals"][:8], inp["noise"][:8], sig[:8])[0]
    b = den.loss({"state_images": inp["state_images"][8:]}, inp["actions"][8:], inp["goals"][8:], inp["noise"][8:], sig[8:])[0]
    return a, b


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_autograd_mode_fires_hooks_and_accumulates_like_autograd(dtype):
    """Default ``grad_mode='autograd'``: AccumulateGrad runs for every trainable parameter (hooks fire exactly once per backward pass, also when
    two forwards share one backward like the reference's multi-modality training_step, mode_agent.py:386-440), repeated backwards accumulate,
    and the result is bit-identical to the arena mode's in-place accumulation."""
    cfg, sd, m = build_train("c1e4", 210, dtype)
    assert m.grad_mode == "autograd"
    inp = {k: v.cuda() for k, v in make_inputs(cfg, 16, 3).items()}
    sig = O.rand_log_logistic((16,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(9)).cuda()
    den = M.GCDenoiser(m, 0.5).train()
    fired = {}
    hooks = [p.register_post_accumulate_grad_hook(lambda p_, n_=n: fired.__setitem__(n_, fired.get(n_, 0) + 1)) for n, p in m.named_parameters()]
    a, b = _two_losses(den, inp, sig)
    (a + b).backward()                                                          # ONE autograd pass over two HIP nodes
    trainable = [n for n, _ in m.named_parameters() if n != "gripper_embed.weight"]
    assert sorted(fired) == sorted(trainable) and set(fired.values()) == {1}
    assert m.gripper_embed.weight.grad is None
    one_pass = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True); fired.clear()
    a, b = _two_losses(den, inp, sig)
    a.backward(); b.backward()                                                  # two passes: the second accumulates
    assert set(fired.values()) == {2}
    for h in hooks:
        h.remove()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, one_pass[n]), n
    # arena mode on the same weights: in-place accumulation in the flat gradient arena gives the same bits
    cfg2, _, m2 = build_train("c1e4", 210, dtype)
    m2.grad_mode = "arena"
    den2 = M.GCDenoiser(m2, 0.5).train()
    a, b = _two_losses(den2, inp, sig)
    a.backward(); b.backward()
    ar = m2.engine.arena
    for n, p in m2.named_parameters():
        if n != "gripper_embed.weight":
            assert p.grad.data_ptr() == ar.g_by_name[n].data_ptr(), n           # p.grad IS the arena slice
            assert torch.equal(p.grad, one_pass[n]), n
    with pytest.raises(ValueError):
        m2.grad_mode = "bogus"
        a, _ = _two_losses(den2, inp, sig)
        a.backward()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["default", "stochastic", "token_routing", "goal_routing", "no_noise_token", "c2block"])
def test_autograd_mode_backward_writes_every_gradient_element(variant, dtype, monkeypatch):
    """``grad_mode='autograd'`` hands out views of an UNINITIALISED per-backward buffer (round-3 advisor finding): the chain must write every element of
    every tensor it returns.  MODE_DEBUG_GRAD_COVERAGE=1 pre-fills the buffer with NaN and raises on anything left behind - run over the layouts the
    library ships (conditioning / token / goal routing, with and without the noise token, multinomial routing + dropouts, the wide block)."""
    monkeypatch.setenv("MODE_DEBUG_GRAD_COVERAGE", "1")
    over = {"default": {}, "stochastic": dict(use_argmax=False, attn_pdrop=0.3, mlp_pdrop=0.1), "token_routing": dict(cond_router=False),
            "goal_routing": dict(use_goal_in_routing=True), "no_noise_token": dict(use_noise_token_as_input=False), "c2block": {}}[variant]
    cfg, sd, m = build_train("c2block" if variant == "c2block" else "c1e4", 210, dtype, **over)
    B = 24
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 3).items()}
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(9)).cuda()
    den = M.GCDenoiser(m, 0.5).train()
    loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], sig)
    (loss + 0.01 * m.load_balancing_loss() + 0.001 * m.compute_router_z_loss()).backward()
    for n, p in m.named_parameters():
        if n != "gripper_embed.weight":
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("overlap", [False, True])
def test_accumulated_backwards_then_overlapped_step_with_reducer(overlap):
    """Two backwards before the optimizer step (arena mode), then ``FusedAdamW.step(overlap=..., reducer=...)``: the per-block events the optimizer /
    reducer gate on must be re-recorded behind the accumulation, otherwise block slices could be consumed before the second backward's sum
    landed.  Reference semantics: one step on the SUM of the two gradients."""
    from mode_diffusion_policy_amd.ddp import ArenaGradReducer
    from mode_diffusion_policy_amd.optim import FusedAdamW
    res = []
    for variant in ("two_backwards", "summed_loss"):
        cfg, sd, m = build_train("c1e4", 210, "bf16")
        inp = {k: v.cuda() for k, v in make_inputs(cfg, 16, 3).items()}
        sig = O.rand_log_logistic((16,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(9)).cuda()
        den = M.GCDenoiser(m, 0.5).train()
        opt = FusedAdamW(m, lr=1e-3)
        red = ArenaGradReducer.for_model(m)
        for _ in range(2):
            a, b = _two_losses(den, inp, sig)
            if variant == "two_backwards":
                a.backward(); b.backward()
                opt.step(overlap=overlap, reducer=red)
            else:
                (a + b).backward()
                opt.step()
        torch.cuda.synchronize()
        res.append({n: p.detach().clone() for n, p in m.named_parameters()})
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n


# ---------------------------------------------------------------------------------------------- torch DDP the way Lightning wraps the agent
class _Agent(torch.nn.Module):
    """What Lightning hands to DistributedDataParallel: one module owning a trainable encoder and the denoiser; forward = the training loss."""

    def __init__(self, enc, den):
        super().__init__()
        self.enc, self.model = enc, den

    def forward(self, raw, actions, goals, noise, sigma):
        cfg_img = self.model.inner_model
        img = self.enc(raw).view(raw.shape[0], cfg_img.n_img_tokens, cfg_img.obs_dim)
        return self.model.loss({"state_images": img}, actions, goals, noise, sigma)[0]


def _make_agent(dtype):
    cfg, sd, m = build_train("c1e4", 210, dtype)
    den = M.GCDenoiser(m, 0.5).train()
    return cfg, sd, _Agent(_encoder(cfg, 24, 1).cuda(), den)


def _ddp_data(cfg, B):
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 55).items()}
    raw = torch.from_numpy(np.random.RandomState(5).standard_normal((B, 24)).astype(np.float32)).cuda()
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(9)).cuda()
    return inp, raw, sig


def _torch_ddp_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch.nn.parallel import DistributedDataParallel as DDP
        from mode_diffusion_policy_amd.ddp import optimizer_param_groups
        torch.cuda.set_device(0)
        cfg, sd, agent = _make_agent("fp32")
        ddp = DDP(agent, device_ids=[0], find_unused_parameters=True)          # strategy="ddp_find_unused_parameters_true" (training_calvin.py:98)
        opt = torch.optim.AdamW(optimizer_param_groups(agent, 0.05), lr=1e-3, betas=(0.9, 0.95))
        B = 16
        inp, raw, sig = _ddp_data(cfg, B)
        sl = slice(rank * B // world, (rank + 1) * B // world)
        grads = None
        for step in range(2):
            opt.zero_grad(set_to_none=True)
            loss = ddp(raw[sl], inp["actions"][sl], inp["goals"][sl], inp["noise"][sl], sig[sl])
            loss.backward()
            if step == 0:
                grads = {n: p.grad.detach().cpu().clone() for n, p in agent.named_parameters() if p.grad is not None}
            opt.step()
        torch.cuda.synchronize()
        torch.save(dict(grads=grads, params={n: p.detach().cpu() for n, p in agent.named_parameters()}), os.path.join(outdir, f"t{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_torch_ddp_world2_equals_single_process_on_concatenated_batch(tmp_path):
    """The reference's own data parallelism - torch DistributedDataParallel with find_unused_parameters (mode/training_calvin.py:92-103) around
    a module that owns a trainable encoder and the HIP denoiser, torch AdamW - reduces correctly: every rank ends with the gradients / weights
    of a single process that saw the whole batch (the dead gripper_embed is reported unused, un-routed experts carry exact zeros)."""
    import torch.multiprocessing as mp
    from mode_diffusion_policy_amd.ddp import optimizer_param_groups
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_torch_ddp_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    w = [torch.load(tmp_path / f"t{r}.pt") for r in range(2)]
    cfg, sd, agent = _make_agent("fp32")
    opt = torch.optim.AdamW(optimizer_param_groups(agent, 0.05), lr=1e-3, betas=(0.9, 0.95))
    inp, raw, sig = _ddp_data(cfg, 16)
    grads = None
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        loss = agent(raw, inp["actions"], inp["goals"], inp["noise"], sig)
        loss.backward()
        if step == 0:
            grads = {n: p.grad.detach().cpu().clone() for n, p in agent.named_parameters() if p.grad is not None}
        opt.step()
    assert set(w[0]["grads"]) == set(grads) and "model.inner_model.gripper_embed.weight" not in grads
    checked = 0
    for n, g in grads.items():
        assert torch.equal(w[0]["grads"][n], w[1]["grads"][n]), n               # all ranks hold the same reduced gradient
        if float(g.norm()) > 1e-7:
            assert rel(w[0]["grads"][n], g) < 2e-3, (n, rel(w[0]["grads"][n], g))
            checked += 1
    assert checked > 50 and "enc.weight" in grads
    for n, p in agent.named_parameters():
        assert torch.equal(w[0]["params"][n], w[1]["params"][n]), n


# ---------------------------------------------------------------------------------------------- bench.py's data-parallel training leg
def _bench_leg_worker(rank, world, port, outdir):
    import json
    import sys
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench
        torch.cuda.set_device(0)
        cfg, sd, m = build_train("c1e4", 210, "bf16", attn_pdrop=0.3, mlp_pdrop=0.1, goal_drop=0.1, use_argmax=False)
        den = M.GCDenoiser(m, 0.5)
        out = bench.train_leg(den, torch.device("cuda", 0), world, rank, dist, steps=3, warmup=1, B=8)                    # default: overlapped all-reduce
        torch.cuda.synchronize()
        out["_w_sum"] = float(m.engine.arena.flat.double().sum())
        z = bench.train_leg(den, torch.device("cuda", 0), world, rank, dist, steps=3, warmup=1, B=8, zero1="bf16")     # then the sharded optimizer
        torch.cuda.synchronize()
        out["_zero1"] = dict(z, _w_sum=float(m.engine.arena.flat.double().sum()))
        json.dump(out, open(os.path.join(outdir, f"b{rank}.json"), "w"))
    finally:
        dist.destroy_process_group()


def test_bench_train_leg_world2_dry_run_and_rccl_world1(tmp_path):
    """`bench.py --gpus N` runs `train_leg` on every rank so that a multi-GPU record shows the gradient exchange (BASELINE configs[3]).  Exactly that
    function: (a) world 2 on ONE GPU over gloo (two RCCL ranks cannot share a device) - the all-reduce default, then ZeRO-1 on the same model, all keys
    present, both ranks end with the same weights after each; (b) world 1 under RCCL, the way the driver launches N = 1 through torch.distributed.run."""
    import json
    import sys
    import torch.distributed as dist
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_bench_leg_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    r = [json.load(open(tmp_path / f"b{i}.json")) for i in range(2)]
    keys = {"train_ms_per_step", "train_samples_per_s", "dp_mode", "exposed_exchange_and_optimizer_ms", "rccl_ranks", "dp_ranks", "dp_backend"}
    assert keys <= set(r[0]) and r[0]["dp_ranks"] == 2 and r[0]["dp_mode"] == "allreduce" and r[0]["dp_backend"] == "gloo" and r[0]["rccl_ranks"] is None
    assert r[0]["train_global_batch"] == 16 and r[0]["train_ms_per_step"] == r[1]["train_ms_per_step"]      # MAX over ranks, whole-job rate
    assert r[0]["_w_sum"] == r[1]["_w_sum"]                                                                 # ranks end with identical weights
    z = [x["_zero1"] for x in r]
    assert keys <= set(z[0]) and z[0]["dp_mode"] == "zero1:bf16" and z[0]["dp_ranks"] == 2 and z[0]["_w_sum"] == z[1]["_w_sum"] != r[0]["_w_sum"]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench
        cfg, sd, m = build_train("c1e4", 210, "bf16", attn_pdrop=0.3, mlp_pdrop=0.1, goal_drop=0.1, use_argmax=False)
        out = bench.train_leg(M.GCDenoiser(m, 0.5), torch.device("cuda", 0), 1, 0, dist, steps=2, warmup=1, B=8)
        assert out["rccl_ranks"] == 1 and out["dp_backend"] == "nccl" and out["dp_mode"] == "single" and out["train_ms_per_step"] > 0
    finally:
        dist.destroy_process_group()


def test_bench_main_world2_end_to_end_through_torch_distributed_run(tmp_path):
    """The WHOLE of bench.py the way the driver launches N = 2 - ``python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 --full`` - on this
    one-GPU box: both ranks on cuda:0, the collective on gloo (MODE_BENCH_SHARE_GPU / MODE_BENCH_BACKEND), a 1-layer model (MODE_BENCH_DRYRUN_LAYERS:
    the gloo exchange goes through host memory).  Checks the control flow a SCALE run takes and nothing else: rendezvous, replica headline with
    MAX-over-ranks timing, all-reduce training leg first (rank count verified before timing), ZeRO-1 leg second under its own keys, ONE JSON line on
    stdout from rank 0, clean exit of both ranks."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MODE_BENCH_SHARE_GPU="1", MODE_BENCH_BACKEND="gloo", MODE_BENCH_DRYRUN_LAYERS="1", MODE_BENCH_TRAIN_STEPS="2",
               MODE_TRAIN_LEG_TIMEOUT="200", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MODE_DP_ZERO1", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"]
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["dry_run"] is True and r["n_gpus"] == 2 and r["scaling"] == "weak" and r["config"]["global_batch"] == 256 and r["value"] > 0
    assert r["dp_mode"] == "allreduce" and r["dp_ranks"] == 2 and r["dp_backend"] == "gloo" and r["train_global_batch"] == 256 and r["train_ms_per_step"] > 0
    assert r["zero1_dp_mode"] == "zero1:bf16" and r["zero1_dp_ranks"] == 2 and r["zero1_ms_per_step"] > 0
    assert r["bf16wire_dp_mode"] == "allreduce" and r["bf16wire_dp_comm_dtype"] == "bf16" and r["bf16wire_ms_per_step"] > 0      # third leg: bf16 on the wire
    assert "train_leg_error" not in r and "zero1_leg_error" not in r and "bf16wire_leg_error" not in r
    assert "[bench] headline done" in p.stderr and "[bench] train leg done" in p.stderr and "[bench] zero1 leg done" in p.stderr
    assert "[bench] bf16wire leg done" in p.stderr
    # the scaling anchor: every rank's two-pass step WITHOUT the exchange, and each leg's throughput against N x that
    assert r["train_twopass_local_ms_per_step"] > 0 and "[bench] twopass leg done" in p.stderr and r["scaling_claim_leg"] == "bf16wire"
    for k in ("scaling_vs_twopass_n1", "zero1_scaling_vs_twopass_n1", "bf16wire_scaling_vs_twopass_n1"):
        assert 0.0 < r[k] <= 2.0 * 1.5, (k, r[k])                                # = N x local / leg; two ranks SHARE one GPU here, so only sanity is checked
    assert abs(r["scaling_vs_twopass_n1"] - 2 * r["train_twopass_local_ms_per_step"] / r["train_ms_per_step"]) < 2e-3
    assert r["fused_expert_step"] is False and "train_twopass_ms_per_step" not in r     # (N = 1 only: the fused-epilogue step and its two-pass anchor)


def test_bench_dump_outputs_reproducible_across_step_counts(tmp_path):
    """``bench.py --dump-outputs DIR``: the last timed step's action chunk lands in DIR/actions.npy (float32, [B, 10, 7]); the seeded inputs make it
    identical for any --steps / --warmup, and the JSON line reports the --steps it was given and, without --full, nothing measured outside the
    headline's timed steps (1-layer dry-run model: plumbing, not a measurement)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MODE_BENCH_DRYRUN_LAYERS="1")
    outs = []
    for steps, warmup, d in ((2, 1, "a"), (5, 2, "b")):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
               "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        r = json.loads(lines[0])
        assert r["steps"] == steps and r["ms_per_step"] > 0
        assert not {"roofline", "layer_kernels", "train_ms_per_step", "agent_b1_replan_ms_graphed_encoders", "cpu_baseline"} & set(r), sorted(r)
        a = np.load(tmp_path / d / "actions.npy")
        assert a.dtype == np.float32 and a.shape == (128, 10, 7) and np.isfinite(a).all()
        outs.append(a)
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- cond_router=False: token routing in TRAINING
def _tok_model(dtype, **over):
    import dataclasses
    cfg, sd, m = build_train("c1e4", 232, dtype, cond_router=False, **over)
    return dataclasses.replace(cfg, cond_router=False), sd, m


def test_token_routing_training_vs_reference_fixture(golden):
    """F16 = the REAL reference with ``cond_router=False`` in train mode (deterministic config: top-k routing, dropouts off) and both auxiliary
    losses on: every block routes each token on its own ln_2 state, so the router gradient also flows INTO the token stream.  fp32 compute mode:
    expert ids of every token identical, loss terms and every gradient (incl. d state_images) against the reference's autograd."""
    g = golden("F16_c1e4_tokroute_loss_grad")
    cfg, sd, m = _tok_model("fp32")
    B = int(g["B"])
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, int(g["seed"]) + 1).items()}
    den = M.GCDenoiser(m, 0.5).train()
    img = inp["state_images"].clone().requires_grad_(True)
    act, _ = den.loss({"state_images": img}, inp["actions"], inp["goals"], inp["noise"], torch.from_numpy(g["sigma"]).cuda())
    assert torch.equal(m._last_topk.cpu().long().sort(-1).values, torch.from_numpy(g["idx"]).long().reshape(cfg.n_layers, -1, cfg.top_k).sort(-1).values)
    lb, z = m.load_balancing_loss(), m.compute_router_z_loss()
    total = act + float(g["gamma"]) * lb + float(g["delta"]) * z
    for got, key in ((act, "act"), (lb, "lb"), (z, "z"), (total, "total")):
        assert abs(float(got) - float(g[key])) < 1e-4 * abs(float(g[key])), key
    total.backward()
    assert rel(img.grad, g["dimg"]) < 2e-3
    grads = {n: p.grad for n, p in m.named_parameters()}
    gn = dict(zip(g["gn_keys"].tolist(), g["gn_vals"].tolist()))
    for n, ref in gn.items():
        if ref > 1e-6:
            assert abs(float(grads[n].norm()) - ref) / ref < 1e-3, (n, float(grads[n].norm()), ref)
    for key in g.files:
        if key.startswith("g:") and gn[key[2:]] > 1e-6:
            assert rel(grads[key[2:]], g[key]) < 2e-3, key
        if key.startswith("gs:") and gn[key[3:]] > 1e-6:
            assert float((grads[key[3:]].reshape(-1)[:2048].cpu() - torch.from_numpy(g[key])).norm()) < 2e-3 * gn[key[3:]], key


@pytest.mark.parametrize("dtype,argmax", [("fp32", False), ("bf16", False), ("bf16", True)])
def test_token_routing_training_vs_oracle_shared_randomness(dtype, argmax):
    """Stochastic token-routing training (per-token multinomial draw between the two phases of every layer, attention + expert dropout) and the
    bf16 mode against the oracle's autograd with SHARED randomness: the ids the HIP chain fixed are handed to the oracle (in bf16 the top-k of a
    near-tied token may differ from an fp32 router's - see tests/tolerances.py - so the comparison is conditional on identical routing)."""
    from tolerances import GRAD, LOSS
    torch.manual_seed(5)
    cfg, sd, m = _tok_model(dtype, attn_pdrop=0.0 if argmax else 0.3, mlp_pdrop=0.0 if argmax else 0.1, use_argmax=argmax)
    B = 12
    inp = make_inputs(cfg, B, 91)
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(5))
    c = {k: v.cuda() for k, v in inp.items()}
    den = M.GCDenoiser(m, 0.5).train()
    img = c["state_images"].clone().requires_grad_(True)
    act, _ = den.loss({"state_images": img}, c["actions"], c["goals"], c["noise"], sig.cuda())
    total = act + 0.01 * m.load_balancing_loss() + 0.001 * m.compute_router_z_loss()
    total.backward()
    idx = m._last_topk.cpu().long()                                             # [L, B*T, k]
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    img_ref = inp["state_images"].clone().requires_grad_(True)
    drop = None if argmax else dict(seed=m._last_seed, attn_p=0.3, mlp_p=0.1)
    rt, ra, rl, rz = O.training_total_loss(sdg, cfg, 0.5, img_ref, inp["actions"], inp["goals"], inp["noise"], sig, 0.01, 0.001,
                                           topk_idx=[idx[l].view(B, cfg.seq_len, cfg.top_k) for l in range(cfg.n_layers)], dropout=drop)
    rt.backward()
    assert abs(float(total) - float(rt)) < LOSS[dtype] * abs(float(rt)), (float(total), float(rt))
    errs = {n: rel(p.grad, sdg[n].grad) for n, p in m.named_parameters() if sdg[n].grad is not None and float(sdg[n].grad.norm()) > 1e-7}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"token routing train {dtype} argmax={argmax}: loss {abs(float(total) - float(rt)) / abs(float(rt)):.1e}, d img {rel(img.grad, img_ref.grad):.1e}, worst grad {worst[1]:.1e} ({worst[0]})")
    assert rel(img.grad, img_ref.grad) < GRAD[dtype]
    assert worst[1] < GRAD[dtype], worst
    assert len(errs) > 50 and any("router" in n for n in errs)


@pytest.mark.parametrize("mode", ["autograd", "arena"])
def test_training_steps_do_not_accumulate_device_memory(mode):
    """Every training forward allocates its activation stash (1.5 GiB at C2 / B = 128).  It must be released by reference counting as soon as the step's
    graph dies: rounds 1-2 kept the node's OUTPUTS reachable from its ctx (output -> grad_fn -> ctx -> run -> output, a cycle through the C++ node that
    Python's collector cannot traverse), which pinned every step's stash forever - 285 GiB after ~190 steps, with 2-4x slower steps on the way there
    (allocator misses).  Cyclic collector off: only reference counts may free the memory."""
    import gc
    cfg, sd, m = build_train("c1e4", 210, "bf16")
    den = M.GCDenoiser(m, 0.5).train()
    from mode_diffusion_policy_amd.optim import FusedAdamW
    opt = FusedAdamW(m, lr=1e-4) if mode == "arena" else torch.optim.AdamW(m.parameters(), lr=1e-4)
    assert m.grad_mode == mode
    B = 16
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 3).items()}
    sig = torch.full((B,), 0.7, device="cuda")

    def step():
        loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], sig)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        seen = []
        for _ in range(6):
            step()
            torch.cuda.synchronize()
            seen.append(torch.cuda.memory_allocated())
    finally:
        if was:
            gc.enable()
    assert max(seen) <= base + (1 << 20), (base, seen)                         # steady: nothing of a finished step stays allocated
