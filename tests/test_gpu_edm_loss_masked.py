"""GPU: mode_edm_loss_masked element by element (dF, per_sample) and in the scalar loss against the fp64 reference of tests/data_refs.py, inside the
bound derived there from the kernel's stated summation order; and GCDenoiser.loss's launch path with and without the new keywords."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from oracle.weights import make_inputs  # noqa: E402
from test_gpu_train import build_train  # noqa: E402

KINDS = ("mask", "weight", "both", "one_sample_masked", "all_masked", "nan_under_zero_mask")


def make_case(B, W, A, kind, seed):
    rng = np.random.default_rng(seed)
    F, a, n = (rng.standard_normal((B, W, A)).astype(np.float32) for _ in range(3))
    sigma = np.exp(rng.uniform(math.log(2e-3), math.log(80.0), B)).astype(np.float32)
    sigma[0] = 2e-3
    sigma[-1] = 80.0 if B > 1 else sigma[-1]
    mask = (rng.random((B, W)) < 0.6).astype(np.float32)
    mask[:, 0] = 1.0                                                              # a window always starts on a real step
    weight = rng.uniform(0.25, 4.0, B).astype(np.float32)
    if kind == "mask":
        weight = None
    elif kind == "weight":
        mask = None
    elif kind == "one_sample_masked":
        mask[B // 2] = 0.0
    elif kind == "all_masked":
        mask[:] = 0.0
    elif kind == "nan_under_zero_mask":
        mask[0, W - 1] = 0.0
        F[0, W - 1, A - 1] = np.nan
        F[0, W - 1, 0] = np.inf
    return F, a, n, sigma, mask, weight


def launch(F, a, n, sigma, mask, weight, sd=0.5, per_sample=True):
    B, W, A = a.shape
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()
    Fd, ad, nd, sg, md, wd = (dev(x) for x in (F, a, n, sigma, mask, weight))
    dF, loss, per = H.Guarded(B, W * A), H.Guarded(1, 4), H.Guarded(1, B)
    rc = L.load().mode_edm_loss_masked(H.p(Fd), H.p(ad), H.p(nd), H.p(sg), sd, B, W, A, H.p(md), H.p(wd), H.p(loss.t), H.p(dF.t),
                                       H.p(per.t) if per_sample else None, H.stream())
    torch.cuda.synchronize()
    return rc, dF, loss, per


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,A", [(4, 3), (10, 7)])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_masked_loss_against_fp64(B, W, A, kind):
    F, a, n, sigma, mask, weight = make_case(B, W, A, kind, seed=B * 100 + W)
    ref = R.masked_loss(F, a, n, sigma, 0.5, mask, weight)
    rc, dF, loss, per = launch(F, a, n, sigma, mask, weight)
    rc2, dF2, loss2, _ = launch(F, a, n, sigma, mask, weight, per_sample=False)
    assert rc == 0 and rc2 == 0 and dF.intact() and loss.intact() and per.intact()
    assert torch.equal(dF.t, dF2.t) and torch.equal(loss.t[0, :1], loss2.t[0, :1]) and bool(torch.isnan(loss.t[0, 1:]).all())     # deterministic; one scalar written
    g_dF, g_loss, g_per = dF.t.cpu().numpy().reshape(B, W, A).astype(np.float64), float(loss.t[0, 0]), per.t[0].cpu().numpy().astype(np.float64)
    c = (np.ones((B, W)) if mask is None else mask) * (np.ones(B) if weight is None else weight)[:, None]
    dead = np.broadcast_to((c == 0)[:, :, None], (B, W, A))
    raw = dF.t.cpu().numpy().reshape(B, W, A).view(np.uint32)
    assert not raw[dead].any()                                                     # c = 0: exactly +0.0, whatever F holds there
    assert np.isfinite(g_dF).all() and math.isfinite(g_loss)
    e_dF, e_loss = np.abs(g_dF - ref["dF"]), abs(g_loss - ref["loss"])
    live = ref["b_dF"] > 0
    r_dF = float((e_dF[live] / ref["b_dF"][live]).max()) if live.any() else 0.0
    r_loss = e_loss / ref["b_loss"] if ref["b_loss"] > 0 else 0.0
    if kind == "nan_under_zero_mask":                                              # the sample's own mean ignores the weight: only its masked steps
        assert mask[0, W - 1] == 0.0 and math.isfinite(g_per[0])
    e_per = np.abs(g_per - ref["per_sample"])
    lp = ref["b_per_sample"] > 0
    r_per = float((e_per[lp] / ref["b_per_sample"][lp]).max()) if lp.any() else 0.0
    print(f"edm_masked B={B} W={W} A={A} {kind}: loss {ref['loss']:.4e} |err| {e_loss:.2e} (err / bound {r_loss:.3f}); dF worst err / bound {r_dF:.3f}; "
          f"per_sample worst err / bound {r_per:.3f}")
    assert (e_dF <= ref["b_dF"]).all(), r_dF
    assert e_loss <= ref["b_loss"], r_loss
    assert (e_per <= ref["b_per_sample"]).all(), r_per
    if kind == "all_masked":
        assert g_loss == 0.0 and not raw.any() and not g_per.any()
    if kind == "one_sample_masked":
        assert g_per[B // 2] == 0.0 and not raw[B // 2].any()


def test_masked_loss_refuses_bad_arguments():
    F, a, n, sigma, mask, weight = make_case(3, 4, 3, "both", 0)
    dev = lambda x: torch.from_numpy(x).cuda()
    t = [dev(x) for x in (F, a, n, sigma)]
    dF, loss = H.Guarded(3, 12), H.Guarded(1, 4)
    lib = L.load()
    args = lambda **kw: [kw.get("F", H.p(t[0])), kw.get("a", H.p(t[1])), kw.get("n", H.p(t[2])), kw.get("s", H.p(t[3])), 0.5, kw.get("B", 3), kw.get("W", 4),
                         kw.get("A", 3), None, None, kw.get("loss", H.p(loss.t)), kw.get("dF", H.p(dF.t)), None, H.stream()]
    for kw in (dict(F=None), dict(a=None), dict(n=None), dict(s=None), dict(loss=None), dict(dF=None), dict(B=0), dict(W=0), dict(A=-1)):
        assert lib.mode_edm_loss_masked(*args(**kw)) == -1, kw
    torch.cuda.synchronize()
    assert dF.intact() and loss.intact() and bool(torch.isnan(dF.t).all()) and bool(torch.isnan(loss.t).all())


def test_denoiser_loss_launch_paths():
    """Without the keywords den.loss is mode_edm_loss on the chain's output - the bits of a direct call; with them it is mode_edm_loss_masked, and
    the gradient that reaches the chain is that kernel's dF."""
    cfg, sd, m = build_train("c1e4", 210, "fp32")
    den = M.GCDenoiser(m, 0.5).train()
    B = 8
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 3).items()}
    sg = torch.exp(torch.linspace(math.log(0.05), math.log(20.0), B)).cuda()
    st = {"state_images": inp["state_images"]}
    calls = []
    lib = L.load()
    real = {n: getattr(lib, n) for n in ("mode_edm_loss", "mode_edm_loss_masked")}

    class Spy:                                                                    # counts the calls, forwards them unchanged
        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            calls.append(self.name)
            return real[self.name](*a)
    try:
        for n in real:
            setattr(lib, n, Spy(n))
        loss, F = den.loss(st, inp["actions"], inp["goals"], inp["noise"], sg)
        assert calls == ["mode_edm_loss"]
        mask = torch.ones(B, 10, device="cuda"); mask[:, 6:] = 0; mask[3, 1:] = 0
        wgt = torch.linspace(0.5, 2.0, B).cuda()
        lm, Fm = den.loss(st, inp["actions"], inp["goals"], inp["noise"], sg, action_mask=mask, sample_weight=wgt)
        assert calls == ["mode_edm_loss", "mode_edm_loss_masked"]
        l1, _ = den.loss(st, inp["actions"], inp["goals"], inp["noise"], sg, action_mask=torch.ones(B, 10, device="cuda"))
        assert calls[-1] == "mode_edm_loss_masked"
    finally:
        for n, fn in real.items():
            setattr(lib, n, fn)
    a, nz = inp["actions"].contiguous(), inp["noise"].contiguous()
    direct, dFd = torch.empty(1, device="cuda"), torch.empty_like(a)
    L.check(lib.mode_edm_loss(F.detach().contiguous().data_ptr(), a.data_ptr(), nz.data_ptr(), sg.data_ptr(), 0.5, B, 70, direct.data_ptr(), dFd.data_ptr(), H.stream()))
    assert torch.equal(loss.detach().view(1), direct) and torch.equal(F, Fm)
    ref = R.masked_loss(Fm.detach().cpu().numpy(), a.cpu().numpy(), nz.cpu().numpy(), sg.cpu().numpy(), 0.5, mask.cpu().numpy(), wgt.cpu().numpy())
    assert abs(float(lm) - ref["loss"]) <= ref["b_loss"]
    plain = R.masked_loss(F.detach().cpu().numpy(), a.cpu().numpy(), nz.cpu().numpy(), sg.cpu().numpy(), 0.5)
    assert abs(float(l1) - plain["loss"]) <= plain["b_loss"] and abs(float(l1) - float(loss)) <= 1e-5 * float(loss)      # all-ones mask: the plain mean
    # backward through the masked loss: padded steps send exactly nothing into the chain
    seen = {}
    Fm.register_hook(lambda g: seen.setdefault("dF", g.clone()))
    (2.0 * lm).backward()
    g = seen["dF"].cpu().numpy().astype(np.float64)
    assert not g[:, 6:].any() and not g[3, 1:].any() and (np.abs(g - 2.0 * ref["dF"]) <= 2.0 * ref["b_dF"]).all()          # (the factor 2 is exact)
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    # generic path (eval mode): the torch expression honours the same keywords
    den.eval()
    with torch.no_grad():
        le, Fe = den.loss(st, inp["actions"], inp["goals"], inp["noise"], sg, action_mask=mask, sample_weight=wgt)
    re = R.masked_loss(Fe.cpu().numpy(), a.cpu().numpy(), nz.cpu().numpy(), sg.cpu().numpy(), 0.5, mask.cpu().numpy(), wgt.cpu().numpy())
    assert abs(float(le) - re["loss"]) <= 1e-5 * re["loss"]
