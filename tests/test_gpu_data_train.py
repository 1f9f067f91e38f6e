"""GPU: a training step fed by data.WindowStream - the masked loss and its parameter gradients against the oracle's autograd on the same
actions / noise / sigma, the reproducibility of a run from (seed, step), and the memory of repeated batch() calls."""
import gc
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import data, utils  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import make_inputs  # noqa: E402
from test_gpu_train import build_train, rel  # noqa: E402
from tolerances import FP32_GRAD, FP32_LOSS  # noqa: E402

W, A, G, B = 10, 7, 512, 8


def make_stream(seed=7):
    st = data.EpisodeStore(A, G)
    for e in R.make_store(W, A, G, seed=5):                                       # episodes of 1, 9, 10 and 13 steps: most windows run past an end
        st.add_episode(e[0], e[1])
    return data.WindowStream(st.finalize("minmax"), B, W, seed=seed, pad="hold")


def step_batch(stream, t, img):
    b = stream.batch(t)
    sig = utils.rand_log_logistic((B,), loc=math.log(0.5), scale=0.5, min_value=1e-3, max_value=80.0, u=b["u"])
    return b, sig, {"lang": {"perceptual_emb": {"state_images": img}, "latent_goal": b["latent_goal"], "actions": b["actions"],
                             "action_mask": b["action_mask"], "noise": b["noise"], "sigmas": sig}}


def test_training_step_on_a_stream_batch_vs_oracle_autograd():
    cfg, sd, m = build_train("c1e4", 210, "fp32")
    den = M.GCDenoiser(m, 0.5).train()
    img = make_inputs(cfg, B, 31)["state_images"]
    b, sig, batch = step_batch(make_stream(), 3, img.cuda())
    mask = b["action_mask"].cpu()
    assert 0 < int((mask == 0).sum()) < mask.numel() and bool((mask[:, 0] == 1).all())       # some rows are padded, every window has a real step
    assert sig.dtype == torch.float32 and sig.is_cuda and float(sig.min()) >= 1e-3 and float(sig.max()) <= 80.0
    total, act, _ = M.training_step(den, batch)
    total.backward()
    # the oracle: the same scalings and target, the masked mean written in torch
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    a, nz, s = b["actions"].cpu(), b["noise"].cpu(), sig.cpu()
    c_skip, c_out, c_in = (t.reshape(-1, 1, 1) for t in O.edm_scalings(s, 0.5))
    noised = a + nz * s.reshape(-1, 1, 1)
    out = O.dit_forward(sdg, cfg, img, noised * c_in, b["latent_goal"].cpu().unsqueeze(1), s)
    target = (a - c_skip * noised) / c_out
    ref_loss = (mask.unsqueeze(2) * (out - target).pow(2)).sum() / (A * mask.sum())
    ref_loss.backward()
    assert torch.equal(total, act) and abs(float(total) - float(ref_loss)) < FP32_LOSS * abs(float(ref_loss))
    checked, worst = 0, (0.0, "")
    for n, p in m.named_parameters():
        r = sdg[n].grad
        if r is None or float(r.norm()) < 1e-7:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6, n           # un-routed experts / dead parameter
            continue
        e = rel(p.grad, r)
        worst = max(worst, (e, n)); checked += 1
        assert e < FP32_GRAD, (n, e)
    print(f"stream-fed training step: loss {float(total):.5f} (oracle {float(ref_loss):.5f}), worst gradient rel-L2 {worst[0]:.2e} ({worst[1]}), {checked} tensors")
    assert checked > 40


def test_a_run_is_reproducible_from_seed_and_step():
    """Two runs from scratch - a new store, stream, model and optimizer from the same seeds - give bit-identical losses for steps 0..2; a run
    resumed at step 2 from the first run's weights sees step 2's batch again."""
    def run(steps, state=None):
        cfg, sd, m = build_train("c1e4", 210, "fp32")
        if state is not None:
            m.load_state_dict(state)
        den = M.GCDenoiser(m, 0.5).train()
        img = make_inputs(cfg, B, 31)["state_images"].cuda()
        stream = make_stream()
        opt = torch.optim.SGD(m.parameters(), lr=1e-3)
        losses, states = [], []
        for t in steps:
            states.append({k: v.detach().clone() for k, v in m.state_dict().items()})
            total, _, _ = M.training_step(den, step_batch(stream, t, img)[2])
            total.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            losses.append(total.detach().clone())
        return losses, states
    l1, states = run(range(3))
    l2, _ = run(range(3))
    assert all(torch.equal(x, y) for x, y in zip(l1, l2)), (l1, l2)
    assert not torch.equal(l1[0], l1[1])
    l3, _ = run([2], state=states[2])
    assert torch.equal(l3[0], l1[2])


def test_batch_calls_hold_no_memory():
    st = data.EpisodeStore(A, G)
    for e in R.make_store(W, A, G, seed=5, cams=((12, 10), (9, 9))):
        st.add_episode(*e)
    st.finalize()
    tr = (M.CameraTransform((8, 8), shift_pad=2), M.CameraTransform((8, 8)))
    stream = data.WindowStream(st, 64, W, camera_transforms=tr)
    for t in range(3):
        stream.batch(t)
    torch.cuda.synchronize()
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        stream.batch(3)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        seen = []
        for t in range(200):
            stream.batch(4 + t)
            if t % 20 == 19:
                torch.cuda.synchronize()
                seen.append(torch.cuda.memory_allocated())
    finally:
        if was:
            gc.enable()
    torch.cuda.synchronize()
    assert max(seen) <= base, (base, seen)
