"""The implicit-GEMM convolution kernels of csrc/conv_gemm.hip - all twelve conv_gemm_kernel<W_KN, BN, FUSE, NS> - element by element against the fp64
reference and the derived bound of tests/conv_refs.py (validated on the CPU by tests/test_conv_references.py): (a) mode_gemm with a_rows in taps in
both weight layouts, (b) mode_conv_bn_act_fwd with every epilogue term and the statistics epilogue, (c) the convolution wrappers of
perceptual_encoders against F.conv2d in fp64, (d) mode_bn_prepare_partials, (e) the refusals.  Every table-level launch writes into a NaN-prefilled
output between canary rows with canary pad columns (ldy > Cout), reads operands whose leading dimensions are padded and whose index tables lie
a_rows_tap_stride > M apart, and runs under "conv_ns" 2 and 3, which must agree bit for bit.  After a launch, in this order: status 0, canaries intact, no
NaN left inside the logical output, the per-element bound.  Each test prints its worst err / bound per kernel (LABNOTES.md, "Implicit-GEMM convolution
against fp64")."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
from conv_refs import BF16  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
F32 = torch.float32


def dev(t):
    return None if t is None else t.to("cuda")


class conv_ns:
    """The "conv_ns" option for the length of a with-block, 0 (automatic) restored behind it."""

    def __init__(self, ns):
        self.ns = ns

    def __enter__(self):
        assert L.load().mode_set_option(b"conv_ns", self.ns) == 0

    def __exit__(self, *exc):
        L.load().mode_set_option(b"conv_ns", 0)


class Launched:
    def __init__(self, rc, out, stats):
        self.rc, self.out, self.stats = rc, out, stats
        self.intact = out.intact() and all(s.intact() for s in stats)
        self.y = out.out.cpu().contiguous()
        self.stat = [s.t.cpu() for s in stats]
        self.untouched = bool(torch.isnan(self.y).all()) and all(bool(torch.isnan(s).all()) for s in self.stat)
        self.nan_left = bool(torch.isnan(self.y).any()) or any(bool(torch.isnan(s).any()) for s in self.stat)

    def bits(self):
        return [self.y.view(torch.int16)] + [s.view(torch.int32) for s in self.stat]


def fused_desc(c, d_in, out, stats=(), **over):
    """ModeConvBnDesc of a fused case from device operands `d_in` (a dict); over: fields replaced afterwards (the refusals)."""
    t = c.terms
    f = dict(x=H.p(d_in["A"]), ldx=c.lda, idx=H.p(d_in["idx"]), idx_tap_stride=c.idx_stride, taps=c.taps, w=H.p(d_in["W"]), ldw=c.ldw, y=H.p(out.out), ldy=out.ld,
             M=c.M, Cin=c.tap_k, Cout=c.N, bn_eps=R.BN_EPS, relu=int("relu" in t), rows_per_sample=c.rps)
    if "bn" in t:
        f.update(bn_mean=H.p(d_in["bn_mean"]), bn_var=H.p(d_in["bn_var"]))
    if "bn_w" in t:
        f.update(bn_weight=H.p(d_in["bn_w"]))
    if "bn_b" in t:
        f.update(bn_bias=H.p(d_in["bn_b"]))
    if "pre" in t:
        f.update(pre_gamma=H.p(d_in["pre_g"]), pre_beta=H.p(d_in["pre_b"]))
    if "post" in t:
        f.update(post_gamma=H.p(d_in["post_g"]), post_beta=H.p(d_in["post_b"]))
    if "res" in t:
        f.update(residual=H.p(d_in["res"]), ldr=c.ldr)
    if stats:
        f.update(stat_sum=H.p(stats[0].t), stat_sq=H.p(stats[1].t))
    f.update(over)
    return L.ModeConvBnDesc(**f)


def device_inputs(c):
    inp = R.inputs(c)
    d = dict(A=dev(inp.A_buf), W=dev(inp.W_buf), idx=dev(inp.idx_buf), res=dev(inp.res_buf))
    for k in ("bn_mean", "bn_var", "bn_w", "bn_b", "pre_g", "pre_b", "post_g", "post_b"):
        d[k] = dev(getattr(inp, k))
    return d


def launch(c, d_in=None, M=None, **over):
    """One launch of case `c` under its conv_ns.  M: the row count passed (the refusals' M = 0); over: descriptor fields replaced (fused cases)."""
    d_in = d_in or device_inputs(c)
    M = c.M if M is None else M
    out = H.GuardedCols(c.M, c.N, c.ldc, BF16)
    stats = (H.Guarded(c.m_tiles, c.N), H.Guarded(c.m_tiles, c.N)) if c.stats else ()
    with conv_ns(c.ns):
        if c.kind == "gemm":
            rc = H.gemm_into(d_in["A"], d_in["W"], out, M, c.N, c.K, a_rows=d_in["idx"], flags=R.W_KN if c.layout == "w_kn" else 0, lda=c.lda, ldw=c.ldw,
                             a_tap_cols=c.tap_k, a_rows_tap_stride=c.idx_stride)
        else:
            desc = fused_desc(c, d_in, out, stats, **dict(dict(M=M), **over))
            rc = L.load().mode_conv_bn_act_fwd(C.byref(desc), H.stream())
        torch.cuda.synchronize()
    return Launched(rc, out, stats)


def check(rep, c, d_in=None):
    """Reference and bound before the launch; then status, canaries, NaN, bound (and the statistics against the stored y).  Returns the launch."""
    ref, bound, gaps = R.reference(c)
    r = launch(c, d_in)
    if r.rc != 0 or not r.intact or r.nan_left:
        rep.fail(f"{c.tag}: status {r.rc}, canaries intact {r.intact}, NaN left {r.nan_left}")
        return None
    rs = R.ratios(dict(C=r.y), ref, bound)
    if c.stats:
        rs += R.stat_ratios(r.y, r.stat[0], r.stat[1], c.M)
    rep.add(c.kernel, c.tag, rs, gaps)
    zr = R.inputs(c).zero_row
    if c.kind == "gemm" and zr is not None and not bool((r.y[zr].view(torch.int16) == 0).all()):
        rep.fail(f"{c.tag}: row {zr}, whose every tap is -1, is not +0")
    return r


def both_depths(rep, c):
    """The case under conv_ns 2 and 3 from the same device operands: each inside the bound, and the same bits (only the staging differs)."""
    d_in = device_inputs(c)
    a, b = check(rep, c._replace(ns=2), d_in), check(rep, c._replace(ns=3), d_in)
    if a is not None and b is not None and not all(torch.equal(x, y) for x, y in zip(a.bits(), b.bits())):
        rep.fail(f"{c.tag}: conv_ns 2 and 3 differ")


# ------------------------------------------------------------------------------------------------------------------ (a) mode_gemm with a_rows in taps
@pytest.mark.parametrize("tap_k,taps", R.TABLE_TAPS)
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_table_level_gemm(layout, tap_k, taps):
    """M = 1 .. 300 x N = 8 .. 192 at nk = 1, 2, 3 and more K-steps (the ring's prologue, wrap and tail); random tables with repeats and 15-30 % of -1,
    one tap -1 everywhere, one output row -1 in every tap (exactly 0); soft / tails / poison rotate over the shapes."""
    rep = R.Report(f"taps {layout} tap_k={tap_k} taps={taps}")
    for c in R.table_cases(layout, tap_k, taps):
        both_depths(rep, c)
    rep.close()


@pytest.mark.parametrize("i", range(len(R.WIDE) + 1), ids=[f"M={s[0]}_N={s[1]}_taps={s[3]}" for s in R.WIDE + (R.NARROW_NEIGHBOUR,)])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_table_level_gemm_wide_tiles(layout, i):
    """The BN = 128 kernels (t128 = 384 at N % 128 == 0) and the neighbour one m-tile below the threshold, which takes BN = 64 at the same N."""
    c = R.wide_cases(layout)[i]
    assert c.kernel[1] == (64 if i == len(R.WIDE) else 128)
    rep = R.Report(f"taps {layout} wide")
    both_depths(rep, c)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (b) mode_conv_bn_act_fwd
def _fused_groups():
    cs = R.fused_cases()
    small = [c for c in cs if not R.takes_wide(c.M, c.N)]
    groups = {"terms_alone_and_all": [c for c in small if (c.M, c.N, c.taps) == (300, 72, 9) and c.rps == 49 and c.terms not in R.RESNET[:3]]}
    for M, N, tk, tp, rps in R.FUSED_SHAPES:
        groups[f"resnet_M={M}_Cout={N}_rps={rps}"] = [c for c in small if (c.M, c.N, c.tap_k, c.taps, c.rps) == (M, N, tk, tp, rps) and c.terms in R.RESNET]
    groups["idx_null"] = [c for c in small if c.direct]
    for c in cs:
        if R.takes_wide(c.M, c.N):
            groups[f"wide_{'direct' if c.direct else 'table'}"] = [c]
    assert sorted(map(str, set(sum(groups.values(), [])))) == sorted(map(str, set(cs)))
    return groups


FUSED_GROUPS = _fused_groups()


@pytest.mark.parametrize("group", FUSED_GROUPS)
def test_fused_epilogue(group):
    """conv + eval-mode BatchNorm + FiLM + residual + ReLU in one launch: each term alone (bn_weight / bn_bias NULL among them), all together, the
    ResNet-block combinations at rows_per_sample 1 .. 200 (tiles that straddle samples, samples that span tiles), idx NULL, ldr > Cout, Cout 8 .. 2048."""
    rep = R.Report(f"fused {group}")
    for c in FUSED_GROUPS[group]:
        both_depths(rep, c)
    rep.close()


@pytest.mark.parametrize("c", R.stat_cases(), ids=lambda c: f"M={c.M}_Cout={c.N}" + ("_direct" if c.direct else ""))
def test_statistics_epilogue(c):
    """stat_sum / stat_sq [ceil(M / 128), Cout] of y as stored, the last tile partial, for BN = 64 (an 8-column n-tile among them) and BN = 128."""
    assert c.M % 128 != 0
    rep = R.Report("stats")
    both_depths(rep, c)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (c) the convolution wrappers
@pytest.mark.parametrize("cv", R.CONVS, ids=lambda cv: cv.tag.replace(" ", "_"))
def test_convolution_level(cv):
    """_conv_fwd_taps, _conv_dgrad_taps and _conv_bn_fwd (plain, with the whole epilogue, and with the statistics) against F.conv2d in fp64 and its
    autograd on the same bf16 operands, under the automatic ring depth and both forced ones."""
    from mode_diffusion_policy_amd import perceptual_encoders as E
    inp, ref = R.conv_inputs(cv), R.conv_reference(cv)
    cl = lambda t: t.to("cuda").contiguous(memory_format=torch.channels_last)
    x, w, dy, res = cl(inp.x), cl(inp.w), cl(inp.dy), cl(inp.res)
    st, pd = (cv.sh, cv.sw), (cv.ph, cv.pw)
    Kf, Kd = cv.taps * cv.cin, cv.taps * cv.cout
    b_y = (Kf + 2) * R.U * ref["S_y"] + R.half_ulp_bf16(ref["y"])
    b_dx = (Kd + 2) * R.U * ref["S_dx"] + R.half_ulp_bf16(ref["dx"])
    ep = {k: dev(getattr(inp, k)) for k in ("bn_mean", "bn_var", "bn_w", "bn_b", "pre_g", "pre_b", "post_g", "post_b")}
    ye, b_e, gaps, _ = R.epilogue_ref(ref["y"], ref["S_y"], Kf, R.TERMS, cv.ho * cv.wo, inp.bn_mean, inp.bn_var, inp.bn_w, inp.bn_b, R.BN_EPS, inp.pre_g,
                                      inp.pre_b, R.rows_of(inp.res), inp.post_g, inp.post_b)
    b_e = b_e + R.half_ulp_bf16(ye)
    rep = R.Report(cv.tag)
    wide = R.takes_wide(cv.rows_out, cv.cout)
    for ns in (0, 2, 3):
        with conv_ns(ns):
            y = E._conv_fwd_taps(x, w, st, pd)
            dx = E._conv_dgrad_taps(dy, w, tuple(x.shape), st, pd)
            yp = E._conv_bn_fwd(x, w, st, pd)
            yf = E._conv_bn_fwd(x, w, st, pd, bn_mean=H.p(ep["bn_mean"]), bn_var=H.p(ep["bn_var"]), bn_weight=H.p(ep["bn_w"]), bn_bias=H.p(ep["bn_b"]),
                                bn_eps=R.BN_EPS, residual=H.p(res), ldr=cv.cout, relu=1, pre_gamma=H.p(ep["pre_g"]), pre_beta=H.p(ep["pre_b"]),
                                post_gamma=H.p(ep["post_g"]), post_beta=H.p(ep["post_b"]))
            ys, s1, s2 = E._conv_bn_fwd(x, w, st, pd, stats=True)
            torch.cuda.synchronize()
        assert y.shape == (cv.n, cv.cout, cv.ho, cv.wo) and dx.shape == x.shape
        nsf = R.ring_depth(cv.rows_out, cv.cout, wide, ns)
        tag = f"{cv.tag} ns={ns}"
        rep.add(("fwd", 64, nsf), tag, R.ratios(dict(y=R.rows_of(y.cpu())), ref, dict(y=b_y)))
        rep.add(("w_kn", 64, R.ring_depth(cv.rows_in, cv.cin, False, ns)), tag, R.ratios(dict(dx=R.rows_of(dx.cpu())), ref, dict(dx=b_dx)))
        rep.add(("fuse", 64, nsf), tag + " plain", R.ratios(dict(y=R.rows_of(yp.cpu())), ref, dict(y=b_y)))
        rep.add(("fuse", 64, nsf), tag + " epilogue", R.ratios(dict(y=R.rows_of(yf.cpu())), dict(y=ye), dict(y=b_e)), gaps)
        ys_rows = R.rows_of(ys.cpu())
        rep.add(("fuse", 64, nsf), tag + " stats", R.ratios(dict(y=ys_rows), ref, dict(y=b_y)) + R.stat_ratios(ys_rows, s1.cpu(), s2.cpu(), cv.rows_out))
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (d) mode_bn_prepare_partials
@pytest.mark.parametrize("momentum", (0.1, -1.0), ids=("exponential", "cumulative"))
@pytest.mark.parametrize("rows", (1, 3, 157))
def test_bn_prepare_partials(rows, momentum):
    """Given partial sums [rows, 72]: mean, var, invstd, scale, shift, the running statistics (exponential and cumulative average) and
    num_batches_tracked against fp64 under conv_refs.bn_partials_ref's bounds."""
    Cc, per, nbt0 = 72, 5, 3
    g = torch.Generator().manual_seed(rows)
    xs = torch.randn(rows * per, Cc, generator=g, dtype=torch.float64) * 2 + 0.5
    psum, psq = xs.reshape(rows, per, Cc).sum(1).float(), xs.reshape(rows, per, Cc).square().sum(1).float()
    w, b = torch.randn(Cc, generator=g).float(), torch.randn(Cc, generator=g).float()
    rm, rv = torch.randn(Cc, generator=g).float(), (0.5 + torch.rand(Cc, generator=g)).float()
    count = float(rows * per)
    ref, bound = R.bn_partials_ref(psum, psq, count, w, b, 1e-5, momentum, rm, rv, nbt0)
    outs = {k: H.Guarded(1, Cc) for k in ("mean", "var", "invstd", "scale", "shift")}
    run = {k: H.Guarded(1, Cc) for k in ("running_mean", "running_var")}
    run["running_mean"].t.copy_(rm), run["running_var"].t.copy_(rv)
    nbt = torch.tensor([nbt0], dtype=torch.int64, device="cuda")
    d_psum, d_psq, d_w, d_b = dev(psum), dev(psq), dev(w), dev(b)
    rc = L.load().mode_bn_prepare_partials(H.p(d_psum), H.p(d_psq), rows, count, Cc, H.p(d_w), H.p(d_b), 1e-5, momentum, H.p(run["running_mean"].t),
                                           H.p(run["running_var"].t), H.p(nbt), *(H.p(outs[k].t) for k in ("mean", "var", "invstd", "scale", "shift")), H.stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(nbt) == nbt0 + 1 and all(o.intact() for o in list(outs.values()) + list(run.values()))
    rep = R.Report(f"bn_prepare_partials rows={rows}")
    got = {k: o.t.cpu()[0] for k, o in {**outs, **run}.items()}
    rep.add("bn_prepare_partials", f"rows={rows} momentum={momentum}", R.ratios(got, ref, bound))
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ (e) refusals
def test_fused_refusals_leave_the_output_untouched():
    ok = R.fused_case(130, 72, 64, 3, R.RESNET[3], 9, stats=True)
    d_in = device_inputs(ok)
    assert launch(ok, d_in).rc == 0
    p = lambda k: H.p(d_in[k])
    for what, status, over in (("Cin % 64", UNSUPPORTED, dict(Cin=96)), ("Cout % 8", UNSUPPORTED, dict(Cout=68)),
                               ("x 8 bytes off", UNSUPPORTED, dict(x=p("A") + 8)), ("w 8 bytes off", UNSUPPORTED, dict(w=p("W") + 8)),
                               ("idx NULL with taps > 1", BAD_ARG, dict(idx=None)), ("bn_mean without bn_var", BAD_ARG, dict(bn_var=None)),
                               ("bn_var without bn_mean", BAD_ARG, dict(bn_mean=None)), ("stat_sum without stat_sq", BAD_ARG, dict(stat_sq=None)),
                               ("stat_sq without stat_sum", BAD_ARG, dict(stat_sum=None)), ("ldr % 4", UNSUPPORTED, dict(ldr=ok.ldr + 2)),
                               ("FiLM with rows_per_sample = 0", BAD_ARG, dict(rows_per_sample=0)), ("ldy % 8", UNSUPPORTED, dict(ldy=ok.ldc + 4))):
        r = launch(ok, d_in, **over)
        assert r.rc == status and r.intact and r.untouched, (what, r.rc, r.intact, r.untouched)
    r = launch(ok, d_in, M=0)
    assert r.rc == 0 and r.intact and r.untouched


def test_gemm_in_taps_refusals_leave_the_output_untouched():
    c = R.gemm_case("fwd", 130, 72, 128, 2)
    d_in = device_inputs(c)
    assert launch(c, d_in).rc == 0

    def go(out=None, N=c.N, K=c.K, M=c.M, **kw):
        out = out or H.GuardedCols(c.M, c.N, c.ldc, BF16)
        rc = H.gemm_into(d_in["A"], d_in["W"], out, M, N, K, a_rows=d_in["idx"], lda=c.lda, ldw=c.ldw, a_tap_cols=c.tap_k, a_rows_tap_stride=c.idx_stride, **kw)
        torch.cuda.synchronize()
        return rc, out.intact() and bool(torch.isnan(out.out).all())

    offs = torch.tensor([0, 128, 256], dtype=torch.int32, device="cuda")
    bias = torch.zeros(c.N, device="cuda")
    for what, status, kw in (("fp32 out", UNSUPPORTED, dict(out=H.GuardedCols(c.M, c.N, c.ldc, F32))), ("BIAS epilogue", UNSUPPORTED, dict(epilogue=L.EPI_BIAS, bias=bias)),
                             ("split_k = 2", UNSUPPORTED, dict(split_k=2, split_stride=(c.M + 1) * c.ldc)),
                             ("k_group_offsets", UNSUPPORTED, dict(k_group_offsets=offs, num_k_groups=2, c_group_stride=0)), ("N < 8", UNSUPPORTED, dict(N=4)),
                             ("K % a_tap_cols", BAD_ARG, dict(K=c.K + 64)), ("M = 0", 0, dict(M=0))):
        rc, clean = go(**kw)
        assert rc == status and clean, (what, rc, clean)
