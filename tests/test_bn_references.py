"""tests/bn_refs.py without a GPU: (a) the fp64 reference of the BatchNorm / FiLM pass equals fp64 torch autograd of the same chain around
nn.BatchNorm2d's functional form, training and eval, on every term set, and its raw-eval form is the scale / shift form; (b) the bound has power: an fp32
torch stand-in for a correct kernel - the chain in the kernels' operation order, its sums reversed or pairwise - stays inside it for every case and
every output of the GPU test's table, and each deliberate defect of the stand-in leaves it; (c) no element sits near the ReLU kink; (d) the case table
holds the chunk lengths and reaches every kernel instantiation of csrc/encoder_ops.hip, and the dispatch predicates are the library's."""
import types

import pytest
import torch
import torch.nn.functional as F

import bn_refs as R
from bn_refs import F32
from mode_diffusion_policy_amd import _lib as L

CASES = R.all_cases()
KINK = R.kink_cases()
SMALL = [c for c in CASES if c.N * c.C * c.HW <= 50000]
ORDERS = ("reversed", "pairwise")
eps32 = torch.tensor(R.BN_EPS, dtype=F32)


def test_constants_and_descriptor_fields_are_the_bindings():
    assert (R.MODE_BF16, R.MODE_F32) == (L.MODE_BF16, L.MODE_F32)
    assert [f[0] for f in L.ModeBnFilmDesc._fields_] == ["N", "C", "HW", "dtype", "x", "scale", "shift", "pre_gamma", "pre_beta", "residual", "relu", "post_gamma",
                                                          "post_beta", "y", "bn_weight", "bn_bias", "bn_mean", "bn_var", "bn_eps", "channels_last"]


# ------------------------------------------------------------------------------------------------------------------ (a) the reference is autograd's
def _exact(c, inp, training):
    """The case's operands with the BatchNorm folded in fp64 and not rounded: the batch statistics of x (training) or the running ones (eval)."""
    x = R.f64(inp.x)
    e = types.SimpleNamespace(**vars(inp))
    e.mean, var = (x.mean((0, 2)), x.var((0, 2), unbiased=False)) if training else (inp.bn_mean.double(), inp.bn_var.double())
    e.invstd = 1 / torch.sqrt(var + float(eps32))
    e.scale = inp.bn_w.double() * e.invstd
    e.shift = inp.bn_b.double() - e.mean * e.scale
    return e


@pytest.mark.parametrize("training", (1, 0), ids=("training", "eval"))
@pytest.mark.parametrize("terms", R.TERM_SETS, ids=lambda t: "+".join(t) or "none")
def test_reference_is_fp64_autograd_around_batch_norm(terms, training):
    c = R.Case("nchw", "f32", 3, 5, 49, terms, "shifted", False, False)
    inp = R.inputs(c)
    e = _exact(c, inp, training)
    leaf = lambda t: R.f64(t).clone().requires_grad_(True)
    x, w, b, pg, pb, qg, qb = (leaf(t) for t in (inp.x, inp.bn_w, inp.bn_b, inp.pre_g, inp.pre_b, inp.post_g, inp.post_b))
    res = leaf(inp.res) if "res" in terms else None
    rm, rv = inp.bn_mean.double().clone(), inp.bn_var.double().clone()
    v = F.batch_norm(x.unsqueeze(-1), rm, rv, w, b, bool(training), 0.1, float(eps32)).squeeze(-1)
    if "pre" in terms:
        v = pg[:, :, None] * v + pb[:, :, None]
    if "res" in terms:
        v = v + res
    if "relu" in terms:
        v = torch.relu(v)
    if "post" in terms:
        v = (1 + qg[:, :, None]) * v + qb[:, :, None]
    (v * R.f64(inp.dy)).sum().backward()
    y, _ = R.forward_ref(c, e)
    ref, bound = R.backward_ref(c, e, training)
    want = dict(dx=x.grad, dweight=w.grad, dbias=b.grad)
    want.update(dict(dresidual=res.grad) if "res" in terms else {})
    want.update(dict(d_pre_gamma=pg.grad, d_pre_beta=pb.grad) if "pre" in terms else {})
    want.update(dict(d_post_gamma=qg.grad, d_post_beta=qb.grad) if "post" in terms else {})
    assert set(ref) == set(want) == set(bound)
    assert torch.allclose(y, v.detach(), rtol=1e-12, atol=1e-12)
    for k, g in want.items():
        assert torch.allclose(ref[k], g, rtol=1e-10, atol=1e-11), (k, float((ref[k] - g).abs().max()))
        assert bool((bound[k] >= 0).all())
    if training:                                                          # and the bookkeeping is nn.BatchNorm2d's
        sref, _ = R.stats_ref(c, inp.x, inp.bn_w, inp.bn_b, R.BN_EPS, 0.1, inp.bn_mean, inp.bn_var, 3)
        f = float(torch.tensor(0.1, dtype=F32))
        assert torch.allclose(sref["mean"], e.mean) and torch.allclose(sref["scale"], e.scale) and torch.allclose(sref["shift"], e.shift)
        rm2, rv2 = inp.bn_mean.double().clone(), inp.bn_var.double().clone()
        F.batch_norm(R.f64(inp.x).unsqueeze(-1), rm2, rv2, None, None, True, f, float(eps32))
        assert torch.allclose(sref["running_mean"], rm2, rtol=1e-12) and torch.allclose(sref["running_var"], rv2, rtol=1e-12)


@pytest.mark.parametrize("momentum,nbt", ((-1.0, 0), (-1.0, 3)))
def test_cumulative_average_is_batch_norm_with_momentum_none(momentum, nbt):
    c = R.Case("nchw", "f32", 3, 5, 49, (), "shifted", False, False)
    inp = R.inputs(c)
    sref, _ = R.stats_ref(c, inp.x, inp.bn_w, inp.bn_b, R.BN_EPS, momentum, inp.bn_mean, inp.bn_var, nbt)
    rm, rv = inp.bn_mean.double().clone(), inp.bn_var.double().clone()
    F.batch_norm(R.f64(inp.x).unsqueeze(-1), rm, rv, None, None, True, float(torch.tensor(1.0, dtype=F32) / torch.tensor(nbt + 1.0, dtype=F32)), float(eps32))
    assert torch.allclose(sref["running_mean"], rm, rtol=1e-12) and torch.allclose(sref["running_var"], rv, rtol=1e-12)


@pytest.mark.parametrize("terms", R.TERM_SETS, ids=lambda t: "+".join(t) or "none")
def test_raw_eval_form_is_the_scale_shift_form(terms):
    c = R.Case("nhwc", "bf16", 2, 8, 33, terms, "tails", False, False)
    inp = R.inputs(c)
    y_raw, b_raw, gaps = R.forward_raw_ref(c, inp)
    y, _ = R.forward_ref(c, _exact(c, inp, 0))
    assert torch.allclose(y_raw, y, rtol=1e-12, atol=1e-12) and bool((b_raw > 0).all()) and 0 < max(gaps) < 4 * R.U
    y_nw, _, _ = R.forward_raw_ref(c, inp, weight=False, bias=False)
    e = _exact(c, inp, 0)
    e.scale, e.shift = e.invstd, -e.mean * e.invstd
    assert torch.allclose(y_nw, R.forward_ref(c, e)[0], rtol=1e-12, atol=1e-12)


def test_eval_prepare_reference_takes_the_running_statistics():
    inp = R.inputs(CASES[1])
    ref, bound = R.prepare_eval_ref(inp.bn_mean, inp.bn_var, inp.bn_w, inp.bn_b, R.BN_EPS)
    e = _exact(CASES[1], inp, 0)
    assert torch.equal(ref["mean"], e.mean) and torch.allclose(ref["var"], inp.bn_var.double(), rtol=1e-14)
    assert torch.allclose(ref["scale"], e.scale, rtol=1e-12) and torch.allclose(ref["shift"], e.shift, rtol=1e-12, atol=1e-14) and set(bound) == set(R.STAT_KEYS)


# ------------------------------------------------------------------------------------------------------------------ (b) the bound has power
DEFECTS = ("chunk_last_pixel", "film_prev_sample", "tile_tail", "mask_from_v2", "dres_unmasked", "post_no_one", "film_first_split", "dweight_from_x",
           "inv_m_1_over_N", "unbiased_var", "cumulative_after_step", "lane_last_trip")


def fsum(t, order):
    """The sum over the last axis in fp32, one term after the other from the back, or pairwise."""
    if t.shape[-1] == 0:
        return torch.zeros(t.shape[:-1])
    if order == "reversed":
        return t.flip(-1).cumsum(-1)[..., -1]
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat((t, torch.zeros_like(t[..., :1])), -1)
        t = t[..., ::2] + t[..., 1::2]
    return t[..., 0]


def chunk_sums(c, t, order, defect=None):
    """[N, S, C] fp32: t [N, C, HW] summed over each split chunk (NCHW: the row)."""
    parts = []
    for p0, p1 in c.chunks:
        seg = t[:, :, p0:p1]
        if defect == "chunk_last_pixel":
            seg = seg[:, :, :-1]
        if defect == "lane_last_trip":                                   # lane 0 leaves the loop one trip early
            start = (-(-seg.shape[-1] // (64 * c.vec)) - 1) * 64 * c.vec
            seg = torch.cat((seg[..., :start], seg[..., start + c.vec:]), -1)
        parts.append(fsum(seg, order))
    return torch.stack(parts, 1)


def _film(p, defect):
    return (p.roll(1, 0) if defect == "film_prev_sample" else p)[:, :, None]


def standin_forward(c, inp, defect=None, upto_v4=False):
    t = c.terms
    v1 = inp.x.float() * inp.scale[None, :, None] + inp.shift[None, :, None]
    v2 = _film(inp.pre_g, defect) * v1 + _film(inp.pre_b, defect) if "pre" in t else v1
    v3 = v2 + inp.res.float() if "res" in t else v2
    v4 = v3.clamp_min(0) if "relu" in t else v3
    if upto_v4:
        return v1, v2, v3, v4
    y = v4
    if "post" in t:
        y = ((0.0 if defect == "post_no_one" else 1.0) + _film(inp.post_g, defect)) * v4 + _film(inp.post_b, defect)
    if defect == "tile_tail":
        y = y.clone()
        y[:, c.C // R.nhwc_ct(c.dtype) * R.nhwc_ct(c.dtype):] = float("nan")   # never written
    return y.to(c.tdtype)


def standin_backward(c, inp, training, order, defect=None, dweight=None, dbias=None, inv_count=0.0, open_kink=False):
    t = c.terms
    x, dy = inp.x.float(), inp.dy.float()
    v1, v2, v3, v4 = standin_forward(c, inp, defect, upto_v4=True)
    dv4 = dy * ((0.0 if defect == "post_no_one" else 1.0) + _film(inp.post_g, defect)) if "post" in t else dy
    src = v2 if defect == "mask_from_v2" else v3
    dv2 = torch.where(src < 0 if open_kink else src <= 0, torch.zeros(()), dv4) if "relu" in t else dv4
    dv1 = dv2 * _film(inp.pre_g, defect) if "pre" in t else dv2
    xh = (x - inp.mean[None, :, None]) * inp.invstd[None, :, None]
    sums = [chunk_sums(c, s, order, defect) for s in (dy * v4, dy, dv2 * v1, dv2, dv1, dv1 * (x if defect == "dweight_from_x" else xh))]

    def film_grad(P):
        out = P[:, 0].clone()
        for k in range(1, 1 if defect == "film_first_split" else c.S):
            out = out + P[:, k]
        return out

    out = {}
    if "post" in t:
        out["d_post_gamma"], out["d_post_beta"] = film_grad(sums[0]), film_grad(sums[1])
    if "pre" in t:
        out["d_pre_gamma"], out["d_pre_beta"] = film_grad(sums[2]), film_grad(sums[3])
    out["dbias"], out["dweight"] = sums[4].double().sum((0, 1)).float(), sums[5].double().sum((0, 1)).float()
    inner = dv1
    if training:
        inv_m = torch.tensor(inv_count, dtype=F32) if inv_count > 0 else 1.0 / (torch.tensor(float(c.N), dtype=F32) * torch.tensor(float(c.HW), dtype=F32))
        if defect == "inv_m_1_over_N":
            inv_m = torch.tensor(1.0 / c.N, dtype=F32)
        db, dw = (out["dbias"], out["dweight"]) if dweight is None else (dbias, dweight)
        inner = dv1 - (db * inv_m)[None, :, None] - xh * (dw * inv_m)[None, :, None]
    out["dx"] = (inp.scale[None, :, None] * inner).to(c.tdtype)
    if "res" in t:
        out["dresidual"] = (dv4 if defect == "dres_unmasked" else dv2).to(c.tdtype)
    return out


def standin_stats(c, x, w, b, momentum, rm, rv, nbt, order, defect=None):
    xf = x.float()
    count = float(c.N * c.HW)
    m = chunk_sums(c, xf, order, defect).double().sum((0, 1)) / count
    v = (chunk_sums(c, xf * xf, order, defect).double().sum((0, 1)) / count - m * m).clamp_min(0)
    unbias = torch.tensor(count / max(count - 1.0, 1.0), dtype=F32)
    mf, vf = m.float(), v.float()
    vn = vf * unbias if defect == "unbiased_var" else vf
    inv = 1.0 / torch.sqrt(vn + eps32)
    sc = w * inv
    f = torch.tensor(momentum, dtype=F32) if momentum >= 0 else 1.0 / torch.tensor(float(nbt + (2 if defect == "cumulative_after_step" else 1)), dtype=F32)
    return dict(mean=mf, var=vn, invstd=inv, scale=sc, shift=b - mf * sc, running_mean=rm * (1 - f) + mf * f,
                running_var=rv * (1 - f) + (vf * f if defect == "unbiased_var" else vf * unbias * f))


def worst(rs):
    return max(rs, key=lambda r: r[1]) if rs else ("", 0.0, ())


def all_ratios(c, order="reversed", defect=None):
    """Every output of the case - forward, training and eval backward, phase 2 with given sums and inv_count = 1, the statistics under both momenta -
    of the stand-in against the reference: [(name, err / bound, index)]."""
    inp = R.inputs(c)
    y, by = R.forward_ref(c, inp)
    rs = [("y",) + r[1:] for r in R.ratios(dict(y=standin_forward(c, inp, defect)), dict(y=y), dict(y=by))]
    for training in (1, 0):
        ref, bound = R.backward_ref(c, inp, training)
        rs += [(f"{r[0]} training={training}",) + r[1:] for r in R.ratios(standin_backward(c, inp, training, order, defect), ref, bound)]
    gw, gb = inp.bn_w * 3, inp.bn_b * 5
    ref, bound = R.backward_ref(c, inp, 1, gw, gb, 1.0)
    got = standin_backward(c, inp, 1, order, defect, gw, gb, 1.0)
    rs += [(f"{k} phase 2",) + r[1:] for k in ("dx",) for r in R.ratios({k: got[k]}, ref, bound)]
    for momentum in (0.1, -1.0):
        ref, bound = R.stats_ref(c, inp.x, inp.bn_w, inp.bn_b, R.BN_EPS, momentum, inp.bn_mean, inp.bn_var, 3)
        rs += [(f"{r[0]} momentum={momentum}",) + r[1:] for r in R.ratios(standin_stats(c, inp.x, inp.bn_w, inp.bn_b, momentum, inp.bn_mean, inp.bn_var, 3, order, defect),
                                                                        ref, bound)]
    return rs


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("c", CASES + KINK, ids=lambda c: c.shape_id)
def test_correct_standin_is_inside_the_bound(c, order):
    name, q, idx = worst(all_ratios(c, order))
    print(f"{c.tag} {order}: worst err / bound of the stand-in {q:.3g} at {name}{list(idx)}")
    assert q <= 1.0, f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}"


@pytest.mark.parametrize("c", [c for c in SMALL if c.N * c.C * c.HW <= 3000][::3], ids=lambda c: c.shape_id)
def test_correct_standin_is_inside_the_bound_under_every_term_set(c):
    for v in R.with_every_term_set(c):
        name, q, idx = worst(all_ratios(v))
        assert q <= 1.0, f"{v.tag}: {name}{list(idx)} err / bound = {q:.3g}"


def _applies(defect, c):
    t = c.terms
    return {"chunk_last_pixel": c.cl, "film_prev_sample": c.film and c.N >= 2, "tile_tail": c.cl and c.C % R.nhwc_ct(c.dtype) != 0 and c.C > R.nhwc_ct(c.dtype),
            "mask_from_v2": "res" in t and "relu" in t, "dres_unmasked": "res" in t and "relu" in t, "post_no_one": "post" in t,
            "film_first_split": c.film and c.S > 1, "dweight_from_x": True, "inv_m_1_over_N": c.HW > 1, "unbiased_var": c.N * c.HW > 1,
            "cumulative_after_step": True, "lane_last_trip": not c.cl}[defect]


DEFECT_CASES = {d: [c for c in SMALL if _applies(d, c)] for d in DEFECTS}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_leaves_the_bound(defect):
    """In every case of the table the defect applies to, the one-element shape aside (there a wrong mask can be the right one by chance)."""
    cases = DEFECT_CASES[defect]
    assert cases, defect
    caught = []
    for c in cases:
        name, q, idx = worst(all_ratios(c, "pairwise", defect))
        caught.append(q > 1.0)
        print(f"{defect} at {c.tag}: err / bound = {q:.3g} at {name}{list(idx)}")
        assert q > 1.0 or c.N * c.C * c.HW == 1, f"a kernel with {defect} would pass {c.tag}"
    print(f"{defect}: leaves the bound in {sum(caught)} of {len(cases)} cases")
    assert any(caught), f"a kernel with {defect} would pass all of {[c.tag for c in cases]}"


# ------------------------------------------------------------------------------------------------------------------ (c) the ReLU kink
def test_no_element_is_near_the_kink():
    n = 0
    for c in CASES + KINK + [v for c in SMALL for v in R.with_every_term_set(c)]:
        if "relu" in c.terms:
            inp = R.inputs(c)
            assert not bool(R.kink_offenders(c, inp).any()), c.tag
            f = R.chain(c.terms, inp.x, inp.scale, inp.shift, inp.pre_g, inp.pre_b, inp.res, inp.post_g, inp.post_b)
            live = inp.x != 0 if c.kink else torch.ones_like(f.v3, dtype=torch.bool)
            assert bool((f.v3[live].abs() > R.KINK_MARGIN * f.b3[live]).all())
            if c.N * c.C * c.HW >= 64:
                assert 0.1 < float((f.v3 <= 0).double().mean()) < 0.9, c.tag
            n += 1
    assert n > 100


@pytest.mark.parametrize("c", KINK, ids=lambda c: c.shape_id)
def test_kink_exact_case_lies_on_the_kink_and_is_masked(c):
    inp = R.inputs(c)
    zero = inp.x == 0
    assert inp.res is None and bool((inp.shift == 0).all()) and float(zero.double().mean()) > 0.5
    assert bool(torch.signbit(inp.x[zero]).any()) and not bool(torch.signbit(inp.x[zero]).all())
    f = R.chain(c.terms, inp.x, inp.scale, inp.shift, inp.pre_g, inp.pre_b, inp.res, inp.post_g, inp.post_b)
    assert bool((f.v3[zero] == 0).all()) and bool((f.b3[zero] == 0).all())
    ref, bound = R.backward_ref(c, inp, 0)
    assert bool((ref["dx"][zero] == 0).all()) and bool((bound["dx"][zero] == 0).all())
    shut = R.ratios(standin_backward(c, inp, 0, "pairwise"), ref, bound)
    opened = R.ratios(standin_backward(c, inp, 0, "pairwise", open_kink=True), ref, bound)
    assert worst(shut)[1] <= 1.0 and all(q > 1.0 for name, q, _ in opened if name in ("dx", "dbias", "dweight"))


# ------------------------------------------------------------------------------------------------------------------ (d) the table and the predicates
def test_the_table_holds_the_chunk_lengths_and_the_folds_trips():
    nhwc = R.nhwc_cases()
    for dt in ("bf16", "f32"):
        lengths = {b - a for c in nhwc if c.dtype == dt for a, b in c.chunks}
        assert set(R.CHUNK_LENGTHS) <= lengths and {128, 129, 130, 131, 144, 145} <= lengths, sorted(lengths)
        mine = [c for c in nhwc if c.dtype == dt]
        assert {c.S for c in mine} >= {1, 2, 6, 32} and any(c.S == 1 and c.rows > R.FR for c in mine) and any(c.S > 1 and c.rows > R.FR for c in mine)
        assert any(c.C % R.nhwc_ct(dt) == 0 for c in mine) and any(c.C > 2 * R.nhwc_ct(dt) and c.C % R.nhwc_ct(dt) for c in mine)
        for many in (False, True):                                       # PLAIN and FiLM at S = 1 and S > 1
            assert {c.film for c in mine if (c.S > 1) == many} == {False, True}
    nchw = R.nchw_cases()
    for dt in ("bf16", "f32"):
        mine = [c for c in nchw if c.dtype == dt]
        assert any(c.rows > R.FR for c in mine)                          # second trip of the per-channel folds
        film_blocks = lambda c: min(-(-c.N * c.C // 1024), 256) if c.film else 0
        chan_blocks = lambda c: -(-c.C // R.FC)
        assert any(film_blocks(c) > chan_blocks(c) for c in mine) and any(chan_blocks(c) > film_blocks(c) > 0 for c in mine)
        assert any(c.film and c.N * c.C > 256 * 1024 for c in mine)      # second trip of the fold kernel's grid-stride loop
        assert any(c.misaligned and c.vec == 1 and R.bn_vec(c.dtype, c.HW) > 1 for c in mine)
    assert all(c.N * c.C * c.HW <= 10 ** 5 or (c.N, c.C, c.HW) == (33000, 8, 1) for c in CASES)
    assert {c.family for c in CASES} == set(R.FAMILIES) and {c.terms for c in CASES} == set(R.TERM_SETS)


def test_the_case_table_reaches_every_kernel_instantiation():
    reached = set().union(*(c.kernels for c in CASES))
    assert reached == set(R.ALL_KERNELS), sorted(set(R.ALL_KERNELS) - reached)
    assert len({k[0] for k in R.ALL_KERNELS}) == R.GLOBAL_KERNELS == 12 and len(R.ALL_KERNELS) == 34
    for k in R.ALL_KERNELS:
        print(k, sum(k in c.kernels for c in CASES), "cases")
    import os
    import re
    src = open(os.path.join(os.path.dirname(L.__file__), "csrc", "encoder_ops.hip")).read()
    assert set(re.findall(r"__global__ .*?void (\w+)\(", src)) == {k[0] for k in R.ALL_KERNELS}


def test_predicates():
    assert [R.bn_vec("bf16", hw) for hw in (8, 12, 4, 7, 64)] == [8, 4, 4, 1, 8] and [R.bn_vec("f32", hw) for hw in (8, 12, 4, 7)] == [4, 4, 4, 1]
    assert R.bn_vec("bf16", 64, aligned=False) == 1 and (R.nhwc_ct("bf16"), R.nhwc_ct("f32")) == (64, 32)
    assert R.nhwc_ok("bf16", 8) and not R.nhwc_ok("bf16", 12) and R.nhwc_ok("f32", 12) and not R.nhwc_ok("f32", 6) and not R.nhwc_ok("f32", 8, aligned=False)
    assert [R.nhwc_splits(*a) for a in ((1, 8, 289, 64), (2, 40, 784, 64), (12, 8, 784, 64), (1, 8, 4100, 64), (70, 16, 36, 64), (1, 8, 127, 64), (64, 256, 3136, 64))] \
        == [2, 6, 6, 32, 1, 1, 3]


def test_workspace_bytes_is_the_library_s():
    """mode_bn_workspace_bytes (host only) = N S C 24 + 256 with the mirrored S, for every case of the table in both layouts."""
    lib = L.load()
    for c in CASES + KINK:
        for cl in (0, 1):
            assert lib.mode_bn_workspace_bytes(c.N, c.C, c.HW, c.mode_dtype, cl) == R.workspace_bytes(c.N, c.C, c.HW, c.dtype, cl), c.tag
    assert lib.mode_bn_workspace_bytes(-1, 8, 8, 0, 0) == 0 and lib.mode_bn_workspace_bytes(2, 0, 8, 0, 1) == 0
