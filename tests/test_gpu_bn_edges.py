"""The BatchNorm / FiLM pass kernels of csrc/encoder_ops.hip - all twelve __global__ kernels in their 34 instantiations - element by element against the
fp64 reference and the derived bound of tests/bn_refs.py (validated on the CPU by tests/test_bn_references.py): (a) mode_bn_film_act_fwd in the
desc.scale / shift form under every term set and in the raw-eval form, (b) mode_bn_stats and mode_bn_prepare with nn.BatchNorm2d's bookkeeping over two
steps, (c) mode_bn_film_act_bwd in phases 0, 1 and 2, training and eval, and on the ReLU kink itself, (d) the refusals.  Everything is launched through
ctypes descriptors, so that scale / shift, mean / invstd, phase and inv_count are the test's to choose.  y, dx and dresidual are NaN-prefilled and lie
between canary rows, the [C] and [N, C] outputs are NaN-prefilled with canaries around them, the workspace starts as NaN, and the poison family's
activations lie inside NaN padding.  After a launch, in this order: status 0, canaries intact, no NaN left, the per-element bound.  Each test prints its
worst err / bound per kernel form (LABNOTES.md, "BatchNorm / FiLM pass against fp64")."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
from bn_refs import F32  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAN = float("nan")
CASES = R.all_cases()
PARAMS = ("scale", "shift", "mean", "invstd", "bn_w", "bn_b", "bn_mean", "bn_var", "pre_g", "pre_b", "post_g", "post_b")
FILM_OUT = {"pre": ("d_pre_gamma", "d_pre_beta"), "post": ("d_post_gamma", "d_post_beta")}


def dev(t):
    return None if t is None else t.to("cuda")


def lay(c, t, poison=False, off_bytes=0):
    """The logical [N, C, HW] CPU tensor in the case's layout on the device, `off_bytes` into a 16-byte aligned storage, inside (poison) NaN padding."""
    if t is None:
        return None
    flat = (t.permute(0, 2, 1) if c.cl else t).contiguous().reshape(-1)
    pad = 64
    buf = torch.full((2 * pad + flat.numel() + 8,), NAN if poison else 0.0, dtype=t.dtype, device="cuda")
    off = pad + off_bytes // t.element_size()
    v = buf[off: off + flat.numel()]
    v.copy_(flat)
    assert (v.data_ptr() - off_bytes) % 16 == 0
    return v


def logical(c, out):
    """A Guarded activation output as the logical [N, C, HW] CPU tensor."""
    flat = out.t.cpu().reshape(-1)
    return flat.view(c.N, c.HW, c.C).permute(0, 2, 1).contiguous() if c.cl else flat.view(c.N, c.C, c.HW)


def act(c):
    """A guarded activation-shaped output: NCHW [N C, HW], channels_last [N HW, C]."""
    return H.Guarded(*((c.N * c.HW, c.C) if c.cl else (c.N * c.C, c.HW)), c.tdtype)


def workspace(c):
    n = R.workspace_bytes(c.N, c.C, c.HW, c.dtype, int(c.cl))
    return torch.full((n // 4,), NAN, dtype=F32, device="cuda"), n


def device_inputs(c, x=None):
    inp = R.inputs(c)
    poison = c.family == "poison"
    d = dict(x=lay(c, inp.x if x is None else x, poison, 8 if c.misaligned else 0), res=lay(c, inp.res, poison), dy=lay(c, inp.dy, poison))
    for k in PARAMS:
        d[k] = dev(getattr(inp, k))
    return d


def desc(c, d, y=None, raw=None, **over):
    """ModeBnFilmDesc of a case from device operands.  raw: None = the desc.scale / shift form, else (weight given, bias given) of the raw-eval form."""
    t = c.terms
    f = dict(N=c.N, C=c.C, HW=c.HW, dtype=c.mode_dtype, x=H.p(d["x"]), relu=int("relu" in t), y=H.p(y), bn_eps=R.BN_EPS, channels_last=int(c.cl))
    if raw is None:
        f.update(scale=H.p(d["scale"]), shift=H.p(d["shift"]))
    else:
        f.update(bn_mean=H.p(d["bn_mean"]), bn_var=H.p(d["bn_var"]), bn_weight=H.p(d["bn_w"]) if raw[0] else None, bn_bias=H.p(d["bn_b"]) if raw[1] else None)
    if "pre" in t:
        f.update(pre_gamma=H.p(d["pre_g"]), pre_beta=H.p(d["pre_b"]))
    if "post" in t:
        f.update(post_gamma=H.p(d["post_g"]), post_beta=H.p(d["post_b"]))
    if "res" in t:
        f.update(residual=H.p(d["res"]))
    f.update(over)
    return L.ModeBnFilmDesc(**f)


def kname(c, what):
    """The kernel form a launch of `what` ("fwd", "stats", "bwd_sums", "bwd_dx") takes, for the report."""
    if c.cl:
        return f"{what}_nhwc<{c.dtype}" + ((", PLAIN>" if not c.film else ", FILM>") if what == "bwd_sums" else ">")
    return f"{what}<{c.dtype}, {c.vec}>"


# ------------------------------------------------------------------------------------------------------------------ (a) forward
def forward(c, d, raw=None, **over):
    y = act(c)
    rc = L.load().mode_bn_film_act_fwd(C.byref(desc(c, d, y.t, raw, **over)), H.stream())
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.shape_id for c in CASES])
def test_forward(i):
    """Every term set at every shape in the desc.scale / shift form; the raw-eval form (weight / bias given and NULL) on every third shape."""
    rep = R.Report("forward")
    for c in R.with_every_term_set(CASES[i]):
        inp, d = R.inputs(c), device_inputs(c)
        ref, bound = R.forward_ref(c, inp)
        rc, y = forward(c, d)
        got = logical(c, y)
        if rc != 0 or not y.intact() or bool(torch.isnan(got).any()):
            rep.fail(f"{c.tag}: status {rc}, canaries intact {y.intact()}, NaN left {bool(torch.isnan(got).any())}")
            continue
        rep.add(kname(c, "fwd"), c.tag, R.ratios(dict(y=got), dict(y=ref), dict(y=bound)))
        if i % 3 == 0 and c.terms in (CASES[i].terms, R.ALL):
            for raw in ((True, True), (False, False)):
                ref, bound, gaps = R.forward_raw_ref(c, inp, *raw)
                rc, y = forward(c, d, raw)
                got = logical(c, y)
                if rc != 0 or not y.intact() or bool(torch.isnan(got).any()):
                    rep.fail(f"{c.tag} raw-eval {raw}: status {rc}, canaries intact {y.intact()}, NaN left {bool(torch.isnan(got).any())}")
                    continue
                rep.add(kname(c, "fwd") + " raw-eval", f"{c.tag} weight/bias={raw}", R.ratios(dict(y=got), dict(y=ref), dict(y=bound)), gaps)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (b) statistics
class Prepared:
    """The outputs of one mode_bn_prepare / mode_bn_stats launch: [C] fp32, NaN-prefilled, guarded; the running statistics in place."""

    def __init__(self, c, keys, running=None, nbt=None):
        self.out = {k: H.Guarded(1, c.C) for k in keys}
        self.run = {}
        if running is not None:
            self.run = {k: H.Guarded(1, c.C) for k in R.RUN_KEYS}
            for k, v in zip(R.RUN_KEYS, running):
                self.run[k].t.copy_(v.view(1, -1))
        self.nbt = None if nbt is None else torch.tensor([nbt], dtype=torch.int64, device="cuda")

    def intact(self):
        return all(g.intact() for g in list(self.out.values()) + list(self.run.values()))

    def got(self):
        return {k: g.t.cpu()[0] for k, g in {**self.out, **self.run}.items()}

    def untouched(self):
        return all(bool(torch.isnan(g.t).all()) for g in self.out.values())


def prepare(c, x, w, b, momentum, pr, ws=None, ws_bytes=None):
    """mode_bn_prepare; x: the device activation or None (eval)."""
    if ws is None:
        ws, ws_bytes = workspace(c)
    rc = L.load().mode_bn_prepare(H.p(x), c.mode_dtype, c.N, c.C, c.HW, int(c.cl), H.p(w), H.p(b), R.BN_EPS, momentum, H.p(pr.run["running_mean"].t) if pr.run else None,
                                  H.p(pr.run["running_var"].t) if pr.run else None, H.p(pr.nbt), *(H.p(pr.out[k].t) for k in R.STAT_KEYS), H.p(ws) if ws_bytes else None, ws_bytes, H.stream())
    torch.cuda.synchronize()
    return rc


def stats(c, x, pr, ws=None, ws_bytes=None):
    if ws is None:
        ws, ws_bytes = workspace(c)
    rc = L.load().mode_bn_stats(H.p(x), c.mode_dtype, c.N, c.C, c.HW, int(c.cl), H.p(pr.out["mean"].t), H.p(pr.out["var"].t), H.p(ws), ws_bytes, H.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.shape_id for c in CASES])
def test_statistics_and_bookkeeping(i):
    """mode_bn_stats and mode_bn_prepare in training on soft, shifted and poisoned x against the fp64 statistics of x; two consecutive steps (momentum 0.1,
    then the cumulative average, which reads num_batches_tracked before it is stepped); running pointers NULL; eval from the running statistics."""
    rep = R.Report("statistics")
    nbt0 = 3
    for fam in ("soft", "shifted", "poison"):
        c = CASES[i]._replace(family=fam, terms=())
        inp, d = R.inputs(c), device_inputs(c)
        tag = f"{c.tag}"
        pr = Prepared(c, ("mean", "var"))
        rc = stats(c, d["x"], pr)
        ref, bound = R.stats_ref(c, inp.x, None, None, R.BN_EPS, 0.1, None, None, 0)
        if rc != 0 or not pr.intact():
            rep.fail(f"{tag} mode_bn_stats: status {rc}, canaries intact {pr.intact()}")
            continue
        rep.add(kname(c, "stats") + " + finalize", tag, R.ratios(pr.got(), ref, bound))
        # step 1: exponential average
        pr = Prepared(c, R.STAT_KEYS, (inp.bn_mean, inp.bn_var), nbt0)
        rc = prepare(c, d["x"], d["bn_w"], d["bn_b"], 0.1, pr)
        ref, bound = R.stats_ref(c, inp.x, inp.bn_w, inp.bn_b, R.BN_EPS, 0.1, inp.bn_mean, inp.bn_var, nbt0)
        if rc != 0 or not pr.intact() or int(pr.nbt) != nbt0 + 1:
            rep.fail(f"{tag} mode_bn_prepare step 1: status {rc}, canaries intact {pr.intact()}, num_batches_tracked {int(pr.nbt)}")
            continue
        one = pr.got()
        rep.add(kname(c, "stats") + " + prepare", tag + " momentum=0.1", R.ratios(one, ref, bound))
        # step 2 on another batch: cumulative average from the first step's running statistics, weight / bias NULL
        x2 = R.second_batch(c)
        d2 = lay(c, x2, fam == "poison", 8 if c.misaligned else 0)
        pr2 = Prepared(c, R.STAT_KEYS, (one["running_mean"], one["running_var"]), nbt0 + 1)
        rc = prepare(c, d2, None, None, -1.0, pr2)
        ref, bound = R.stats_ref(c, x2, None, None, R.BN_EPS, -1.0, one["running_mean"], one["running_var"], nbt0 + 1)
        if rc != 0 or not pr2.intact() or int(pr2.nbt) != nbt0 + 2:
            rep.fail(f"{tag} mode_bn_prepare step 2: status {rc}, canaries intact {pr2.intact()}, num_batches_tracked {int(pr2.nbt)}")
            continue
        rep.add(kname(c, "stats") + " + prepare + count_step", tag + " momentum=-1", R.ratios(pr2.got(), ref, bound))
    # running pointers NULL: the five outputs alone
    pr = Prepared(c, R.STAT_KEYS)
    rc = prepare(c, d["x"], d["bn_w"], d["bn_b"], 0.1, pr)
    ref, bound = R.stats_ref(c, inp.x, inp.bn_w, inp.bn_b, R.BN_EPS, 0.1, None, None, 0)
    assert rc == 0 and pr.intact()
    rep.add(kname(c, "stats") + " + prepare", tag + " running NULL", R.ratios(pr.got(), ref, bound))
    # eval: from the running statistics, bookkeeping untouched, no workspace
    pr = Prepared(c, R.STAT_KEYS, (inp.bn_mean, inp.bn_var), nbt0)
    rc = prepare(c, None, d["bn_w"], d["bn_b"], 0.1, pr, 0, 0)
    ref, bound = R.prepare_eval_ref(inp.bn_mean, inp.bn_var, inp.bn_w, inp.bn_b, R.BN_EPS)
    got = pr.got()
    assert rc == 0 and pr.intact() and int(pr.nbt) == nbt0 and torch.equal(got.pop("running_mean"), inp.bn_mean) and torch.equal(got.pop("running_var"), inp.bn_var)
    rep.add("prepare eval", tag, R.ratios(got, ref, bound))
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (c) backward
class BwdOut:
    """The outputs of one mode_bn_film_act_bwd launch, NaN-prefilled and guarded.  given: (dweight, dbias) device tensors phase 2 is to read."""

    def __init__(self, c, given=None):
        self.c = c
        self.dx = act(c)
        self.dres = act(c) if "res" in c.terms else None
        self.small = {k: H.Guarded(1, c.C) for k in ("dweight", "dbias")}
        for t in (t for t in ("pre", "post") if t in c.terms):
            self.small.update({k: H.Guarded(c.N, c.C) for k in FILM_OUT[t]})
        if given is not None:
            self.small["dweight"].t.copy_(given[0].view(1, -1)), self.small["dbias"].t.copy_(given[1].view(1, -1))

    def ptr(self, k):
        return H.p(self.small[k].t) if k in self.small else None

    def intact(self):
        return self.dx.intact() and (self.dres is None or self.dres.intact()) and all(g.intact() for g in self.small.values())

    def got(self, acts=True, small=True):
        out = {}
        if acts:
            out["dx"] = logical(self.c, self.dx)
            if self.dres is not None:
                out["dresidual"] = logical(self.c, self.dres)
        if small:
            out.update({k: (g.t.cpu()[0] if k in ("dweight", "dbias") else g.t.cpu()) for k, g in self.small.items()})
        return out

    def bits(self, **kw):
        return {k: v.contiguous().view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32) for k, v in self.got(**kw).items()}


def backward(c, d, o, training, phase=0, inv_count=0.0, ws=None, ws_bytes=None, over=None, **args):
    """One launch; over: descriptor fields replaced, args: entry arguments replaced (the refusals)."""
    if ws is None:
        ws, ws_bytes = workspace(c)
    a = dict(dy=H.p(d["dy"]), mean=H.p(d["mean"]), invstd=H.p(d["invstd"]), dx=H.p(o.dx.t), dresidual=None if o.dres is None else H.p(o.dres.t), dweight=o.ptr("dweight"),
             dbias=o.ptr("dbias"), d_pre_gamma=o.ptr("d_pre_gamma"), d_pre_beta=o.ptr("d_pre_beta"), d_post_gamma=o.ptr("d_post_gamma"), d_post_beta=o.ptr("d_post_beta"))
    a.update(args)
    rc = L.load().mode_bn_film_act_bwd(C.byref(desc(c, d, o.dx.t, **(over or {}))), a["dy"], a["mean"], a["invstd"], training, phase, inv_count, a["dx"], a["dresidual"],
                                       a["dweight"], a["dbias"], a["d_pre_gamma"], a["d_pre_beta"], a["d_post_gamma"], a["d_post_beta"], H.p(ws), ws_bytes, H.stream())
    torch.cuda.synchronize()
    return rc


def no_nan(got):
    return not any(bool(torch.isnan(v).any()) for v in got.values())


def check_backward(rep, c, d, training):
    """Phase 0 against the reference; returns the launch's outputs (None after a failure)."""
    ref, bound = R.backward_ref(c, R.inputs(c), training)
    o = BwdOut(c)
    rc = backward(c, d, o, training)
    got = o.got()
    if rc != 0 or not o.intact() or not no_nan(got) or set(got) != set(ref):
        rep.fail(f"{c.tag} training={training}: status {rc}, canaries intact {o.intact()}, NaN left {not no_nan(got)}, outputs {sorted(got)}")
        return None
    small = {k: v for k, v in got.items() if k not in ("dx", "dresidual")}
    rep.add(kname(c, "bwd_sums") + " + fold", f"{c.tag} training={training}", R.ratios(small, ref, bound))
    rep.add(kname(c, "bwd_dx"), f"{c.tag} training={training}", R.ratios({k: got[k] for k in got if k not in small}, ref, bound))
    return o


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.shape_id for c in CASES])
def test_backward(i):
    """Phase 0 under every term set, training and eval; at the shape's own term set: phase 1 then phase 2 with inv_count = 1 / (N HW) is phase 0 bit for bit,
    phase 1 leaves dx / dresidual alone and phase 2 the [C] and [N, C] gradients, and phase 2 alone with somebody else's dweight / dbias and inv_count = 1
    is the fp64 formula with those values."""
    rep = R.Report("backward")
    for c in R.with_every_term_set(CASES[i]):
        d = device_inputs(c)
        whole = check_backward(rep, c, d, 1)
        check_backward(rep, c, d, 0)
        if c.terms != CASES[i].terms or whole is None:
            continue
        inp = R.inputs(c)
        o = BwdOut(c)
        rc = backward(c, d, o, 1, phase=1)
        if rc != 0 or not o.intact() or not bool(torch.isnan(o.dx.t).all()) or (o.dres is not None and not bool(torch.isnan(o.dres.t).all())):
            rep.fail(f"{c.tag} phase 1: status {rc}, canaries intact {o.intact()}, or dx / dresidual written")
            continue
        small = o.bits(acts=False)
        inv_count = float(torch.tensor(1.0, dtype=F32) / (torch.tensor(float(c.N), dtype=F32) * torch.tensor(float(c.HW), dtype=F32)))
        rc = backward(c, d, o, 1, phase=2, inv_count=inv_count)
        same = all(torch.equal(v, small[k]) for k, v in o.bits(acts=False).items())
        if rc != 0 or not o.intact() or not same:
            rep.fail(f"{c.tag} phase 2: status {rc}, canaries intact {o.intact()}, [C] / [N, C] gradients as phase 1 left them {same}")
            continue
        a, b = o.bits(), whole.bits()
        if not all(torch.equal(a[k], b[k]) for k in b):
            rep.fail(f"{c.tag}: phase 1 + phase 2 differ from phase 0 in {[k for k in b if not torch.equal(a[k], b[k])]}")
        # phase 2 alone, with sums that are not this batch's
        gw, gb = inp.bn_w * 3, inp.bn_b * 5
        ref, bound = R.backward_ref(c, inp, 1, gw, gb, 1.0)
        o = BwdOut(c, (dev(gw), dev(gb)))
        rc = backward(c, d, o, 1, phase=2, inv_count=1.0)
        got = o.got(small=False)
        s = o.got(acts=False)
        kept = torch.equal(s.pop("dweight"), gw) and torch.equal(s.pop("dbias"), gb) and all(bool(torch.isnan(v).all()) for v in s.values())
        if rc != 0 or not o.intact() or not no_nan(got) or not kept:
            rep.fail(f"{c.tag} phase 2 alone: status {rc}, canaries intact {o.intact()}, NaN left {not no_nan(got)}, [C] / [N, C] gradients untouched {kept}")
            continue
        rep.add(kname(c, "bwd_dx") + " phase 2", c.tag, R.ratios(got, ref, bound))
    rep.close()


@pytest.mark.parametrize("c", R.kink_cases(), ids=lambda c: c.shape_id)
def test_kink_exact(c):
    """x holds +0.0 and -0.0 and shift is 0, so v3 == 0 in any arithmetic: dx, the sums and the FiLM gradients treat those elements as masked."""
    rep = R.Report("kink-exact")
    d, inp = device_inputs(c), R.inputs(c)
    assert check_backward(rep, c, d, 1) is not None
    o = check_backward(rep, c, d, 0)
    assert o is not None and bool((logical(c, o.dx)[inp.x == 0] == 0).all())
    rc, y = forward(c, d)
    ref, bound = R.forward_ref(c, inp)
    assert rc == 0 and y.intact()
    rep.add(kname(c, "fwd"), c.tag, R.ratios(dict(y=logical(c, y)), dict(y=ref), dict(y=bound)))
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (d) refusals
def _untouched(o):
    return o.intact() and bool(torch.isnan(o.dx.t).all()) and (o.dres is None or bool(torch.isnan(o.dres.t).all())) and all(bool(torch.isnan(g.t).all()) for g in o.small.values())


@pytest.mark.parametrize("dtype,C_bad", (("bf16", 12), ("f32", 6)))
def test_channels_last_refusals_leave_every_output_untouched(dtype, C_bad):
    """channels_last with C % 8 != 0 (bf16) / C % 4 != 0 (fp32), and with x 8 bytes into its storage: MODE_ERR_UNSUPPORTED from every entry."""
    ok = R.Case("nhwc", dtype, 2, 16, 40, R.ALL, "soft", False, False)
    for c in (ok._replace(C=C_bad), ok._replace(misaligned=True)):
        d = device_inputs(c)
        rc, y = forward(c, d)
        assert rc == UNSUPPORTED and y.intact() and bool(torch.isnan(y.t).all()), (c.tag, rc)
        o = BwdOut(c)
        assert backward(c, d, o, 1) == UNSUPPORTED and _untouched(o), c.tag
        pr = Prepared(c, ("mean", "var"))
        assert stats(c, d["x"], pr) == UNSUPPORTED and pr.intact() and pr.untouched(), c.tag
        inp = R.inputs(c)
        pr = Prepared(c, R.STAT_KEYS, (inp.bn_mean, inp.bn_var), 3)
        assert prepare(c, d["x"], d["bn_w"], d["bn_b"], 0.1, pr) == UNSUPPORTED and pr.intact() and pr.untouched() and int(pr.nbt) == 3, c.tag
        assert torch.equal(pr.run["running_mean"].t.cpu()[0], inp.bn_mean) and torch.equal(pr.run["running_var"].t.cpu()[0], inp.bn_var)
    d = device_inputs(ok)
    rc, y = forward(ok, d)
    assert rc == 0 and y.intact() and not bool(torch.isnan(y.t).any())


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_argument_refusals_leave_every_output_untouched(layout):
    c = R.Case(layout, "bf16", 2, 16, 40, R.ALL, "soft", False, False)
    d, inp = device_inputs(c), R.inputs(c)
    o = BwdOut(c)
    assert backward(c, d, o, 1) == 0 and o.intact() and no_nan(o.got())
    ws, n = workspace(c)
    # the workspace one byte short
    o = BwdOut(c)
    assert backward(c, d, o, 1, ws=ws, ws_bytes=n - 1) == WORKSPACE and _untouched(o)
    pr = Prepared(c, ("mean", "var"))
    assert stats(c, d["x"], pr, ws, n - 1) == WORKSPACE and pr.intact() and pr.untouched()
    pr = Prepared(c, R.STAT_KEYS, (inp.bn_mean, inp.bn_var), 3)
    assert prepare(c, d["x"], d["bn_w"], d["bn_b"], 0.1, pr, ws, n - 1) == WORKSPACE and pr.intact() and pr.untouched() and int(pr.nbt) == 3
    assert torch.equal(pr.run["running_mean"].t.cpu()[0], inp.bn_mean)
    # inconsistent descriptors and arguments
    for what, over, args in (("scale without shift", dict(shift=None), {}), ("shift without scale", dict(scale=None), {}),
                             ("pre_gamma without pre_beta", dict(pre_beta=None), {}), ("post_beta without post_gamma", dict(post_gamma=None), {}),
                             ("residual without dresidual", {}, dict(dresidual=None)), ("pre-FiLM without d_pre_beta", {}, dict(d_pre_beta=None)),
                             ("post-FiLM without its gradients", {}, dict(d_post_gamma=None, d_post_beta=None)), ("dy NULL", {}, dict(dy=None))):
        o = BwdOut(c)
        assert backward(c, d, o, 1, over=over, **args) == BAD_ARG and _untouched(o), what
        if over:
            rc, y = forward(c, d, **over)
            assert rc == BAD_ARG and y.intact() and bool(torch.isnan(y.t).all()), what
    o = BwdOut(c)
    assert backward(c, d, o, 1, phase=3) == BAD_ARG and _untouched(o)
    o = BwdOut(c)
    assert backward(c, d, o, 1, phase=-1) == BAD_ARG and _untouched(o)
    # N = 0: nothing to do, nothing written
    o = BwdOut(c)
    assert backward(c, d, o, 1, over=dict(N=0)) == 0 and _untouched(o)
    rc, y = forward(c, d, N=0)
    assert rc == 0 and y.intact() and bool(torch.isnan(y.t).all())
