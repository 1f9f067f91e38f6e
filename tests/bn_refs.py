"""The fp64 reference of the BatchNorm / FiLM pass (include/mode_hip.h: ModeBnFilmDesc, mode_bn_stats, mode_bn_prepare, mode_bn_film_act_bwd), the
per-element bound, the input families, the launchers' dispatch predicates and the case table, shared by tests/test_gpu_bn_edges.py (which launches the
kernels of csrc/encoder_ops.hip) and tests/test_bn_references.py (which validates all of this without a GPU).  The reference is written from the header's
description of the operation, in plain torch on the CPU in fp64, on logical [N, C, HW] tensors whatever the layout of the launch.

The bound (LABNOTES.md, "BatchNorm / FiLM pass against fp64"), per element, u = 2^-23.  Inputs (bf16 or fp32 activations, fp32 parameters) are exact; a
step a * b + c with R roundings adds R u (|a b| + |c|) to the bounds its operands carry; a sum of n fp32 terms in any order errs by at most
n u sum |terms|; the outputs round by half a unit in the last place of their dtype at the reference value, and nothing else is added.
  forward  (encoder_ops.hip:99-103 and :412-416; R_BN, R_PRE, R_RES, R_POST of conv_refs: one fma each, post-FiLM 1.f + g and the fma)
    v1 = x scale + shift          b1 = R_BN u (|x scale| + |shift|)          (desc.scale / shift form: the parameters are exact)
    v2 = pg v1 + pb               b2 = |pg| b1 + R_PRE u (|pg v1| + |pb|)
    v3 = v2 + r                   b3 = b2 + R_RES u (|v2| + |r|)
    v4 = max(v3, 0)               b4 = b3
    y  = (1 + qg) v4 + qb         b5 = |1 + qg| b4 + R_POST u (|(1 + qg) v4| + |qb|)
    raw-eval form (scale == shift == NULL, :71-73 and :379-385): conv_refs.epilogue_ref itself on the rows of x - 1 / sqrt(var + eps) cannot be
    counted from the source, so scale and shift carry 4 x the MEASURED reference-alone gap (conv_refs.scale_shift_gap), which the GPU test prints
  backward (encoder_ops.hip:222-230 = :472-480 for the sums, :289-296 = :520-527 for dx); the mask is v3 <= 0 and the generator keeps |v3| > 64 b3
    dv4 = dy (1 + qg)             R_DV4 = 2 (:226, 1.f + qg and the product)           dv2 = mask(dv4): its bound, 0 where masked
    dv1 = dv2 pg                  R_DV1 = 1 (:228)
    xhat = (x - mean) invstd      R_XHAT = 2 (:230, the difference and the product)
    six sums over a row (NCHW: n = HW) or over the pixels of one split chunk (channels_last: n = the longest chunk), of dy v4, dy, dv2 v1, dv2, dv1,
    dv1 xhat: the terms' own bounds + n u sum |terms|; the FiLM gradients add the S chunks in fp32 (:253, S - 1 more additions); dweight / dbias fold
    all rows in double (:263) and round once: + u |value|
    dx = scale (dv1 - dbias inv_m - xhat dweight inv_m)   (:277 and :296) with the kernel's OWN dweight / dbias, whose bounds are propagated (inv_m,
      |xhat| inv_m); R_MB = 2 (inv_m's division on the host, :720, and the product), xhat dweight inv_m one more product, the two differences one
      rounding each, the product with scale one; training == 0: dx = scale dv1, one rounding
    dresidual = dv2
  statistics (encoder_ops.hip:122 and :352-360, :151-155, :174-193): fp32 row / chunk sums of x and x^2 - n u sum |x|, n u sum x^2 over the channel -
    folded in double; from there conv_refs.bn_partials_ref (e_sum / e_sq)."""
import collections
import functools
import types

import torch

from conv_refs import R_BN, R_POST, R_PRE, R_RES, Report, bn_partials_ref, epilogue_ref, rows_of, scale_shift_gap  # noqa: F401  (Report, gap: for the tests)
from gemm_refs import U, f64, half_ulp_bf16, ratios  # noqa: F401

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = {"f32": F32, "bf16": BF16}
MODE_BF16, MODE_F32 = 0, 1                          # ModeDType (checked against _lib by test_bn_references.py)
BN_EPS = 1e-5
FAMILIES = ("soft", "shifted", "tails", "poison")
TERMS = ("pre", "res", "relu", "post")
R_DV4, R_DV1, R_XHAT, R_MB = 2, 1, 2, 2             # fp32 roundings of one backward step (module docstring)
KINK_MARGIN = 64
FC, FR = 16, 64                                     # channels and row lanes of a per-channel fold workgroup (encoder_ops.hip:133)


# ------------------------------------------------------------------------------------------------------------------ dispatch predicates
def bn_vec(dtype, HW, aligned=True):
    """Elements per lane and access of the NCHW kernels (encoder_ops.hip bn_vec): 8 (bf16, 16 bytes), 4 (8-byte bf16 / 16-byte fp32) or 1."""
    if not aligned:
        return 1
    if dtype == "bf16" and HW % 8 == 0:
        return 8
    return 4 if HW % 4 == 0 else 1


def nhwc_ct(dtype):
    """Channels of one channels_last tile: 8 threads x 16 bytes."""
    return 64 if dtype == "bf16" else 32


def nhwc_splits(N, C, HW, CT):
    """Pixel splits of a sample: 768 workgroups wanted, chunks of at least 128 pixels, at most 32."""
    wg = N * -(-C // CT)
    return min(min(max(1, 768 // max(wg, 1)), max(1, HW // 128)), 32)


def nhwc_ok(dtype, C, aligned=True):
    return aligned and C % (8 if dtype == "bf16" else 4) == 0


def workspace_bytes(N, C, HW, dtype, cl):
    S = nhwc_splits(N, C, HW, nhwc_ct(dtype)) if cl else 1
    return N * S * C * 24 + 256


# ------------------------------------------------------------------------------------------------------------------ cases
_Case = collections.namedtuple("Case", "layout dtype N C HW terms family misaligned kink")


class Case(_Case):
    """One shape of the pass.  layout "nchw" / "nhwc" (ModeBnFilmDesc.channels_last), dtype "f32" / "bf16", terms: the optional terms present (a subset of
    TERMS; the folded BatchNorm always is), misaligned: x is viewed 8 bytes into its storage, kink: the kink-exact case (x holds +0.0 and -0.0, shift = 0)."""
    __slots__ = ()

    cl = property(lambda s: s.layout == "nhwc")
    S = property(lambda s: nhwc_splits(s.N, s.C, s.HW, nhwc_ct(s.dtype)) if s.cl else 1)
    chunks = property(lambda s: [(s.HW * k // s.S, s.HW * (k + 1) // s.S) for k in range(s.S)])
    n_sum = property(lambda s: max(b - a for a, b in s.chunks))          # terms of one fp32 partial sum: the row (NCHW), the longest split chunk
    vec = property(lambda s: bn_vec(s.dtype, s.HW, not s.misaligned))
    rows = property(lambda s: s.N * s.S)                                 # partial rows a per-channel fold walks
    film = property(lambda s: "pre" in s.terms or "post" in s.terms)
    tdtype = property(lambda s: DTYPES[s.dtype])
    mode_dtype = property(lambda s: MODE_BF16 if s.dtype == "bf16" else MODE_F32)

    @property
    def kernels(self):
        """The instantiations of encoder_ops.hip the GPU tests launch for this case (forward, statistics, both backward passes, the folds)."""
        if self.cl:
            own = {("bn_film_act_fwd_nhwc_kernel", self.dtype), ("bn_nhwc_stats_kernel", self.dtype), ("bn_film_act_bwd_dx_nhwc_kernel", self.dtype),
                   ("bn_film_act_bwd_sums_nhwc_kernel", self.dtype, "PLAIN" if not self.film else "FILM")}
        else:
            own = {(k, self.dtype, self.vec) for k in ("bn_film_act_fwd_kernel", "bn_row_sums_kernel", "bn_film_act_bwd_sums_kernel", "bn_film_act_bwd_dx_kernel")}
        return own | {("bn_finalize_kernel",), ("bn_prepare_kernel",), ("bn_count_step_kernel",), ("bn_film_bwd_fold_kernel",)}

    @property
    def tag(self):
        return (f"{self.layout} {self.dtype} N={self.N} C={self.C} HW={self.HW} {self.family} terms={'+'.join(self.terms) or 'none'}"
                + (" misaligned" if self.misaligned else "") + (" kink-exact" if self.kink else ""))

    @property
    def shape_id(self):
        return f"{self.layout}_{self.dtype}_{self.N}x{self.C}x{self.HW}" + ("_misaligned" if self.misaligned else "") + ("_kink" if self.kink else "")


ALL_KERNELS = tuple([(k, dt, v) for k in ("bn_film_act_fwd_kernel", "bn_row_sums_kernel", "bn_film_act_bwd_sums_kernel", "bn_film_act_bwd_dx_kernel")
                     for dt, v in (("f32", 4), ("f32", 1), ("bf16", 8), ("bf16", 4), ("bf16", 1))]
                    + [(k, dt) for k in ("bn_film_act_fwd_nhwc_kernel", "bn_nhwc_stats_kernel", "bn_film_act_bwd_dx_nhwc_kernel") for dt in ("f32", "bf16")]
                    + [("bn_film_act_bwd_sums_nhwc_kernel", dt, f) for dt in ("f32", "bf16") for f in ("PLAIN", "FILM")]
                    + [("bn_finalize_kernel",), ("bn_prepare_kernel",), ("bn_count_step_kernel",), ("bn_film_bwd_fold_kernel",)])
GLOBAL_KERNELS = 12                                 # __global__ definitions in encoder_ops.hip

ALL = TERMS
TERM_SETS = ((), ("pre",), ("res",), ("relu",), ("post",), ("res", "relu"), ("pre", "res", "relu"), ALL)     # each alone, none, the ResNet-block forms, all
NCHW_SHAPES = ((1, 1, 1), (3, 5, 49), (3, 2, 65), (2, 7, 36), (2, 3, 64), (2, 3, 260), (2, 6, 520), (70, 5, 9), (2, 130, 9), (300, 8, 4), (33000, 8, 1))
NCHW_FORCED = {(2, 130, 9): ALL, (300, 8, 4): ("pre", "res", "relu"), (33000, 8, 1): ALL}                    # the shapes the fold kernel's FiLM loop is for
NHWC_SHAPES = ((3, 8, 9), (2, 64, 32), (2, 72, 33), (2, 136, 65), (2, 16, 97), (70, 16, 36), (1, 8, 289), (2, 40, 784), (12, 8, 784), (1, 8, 4100),
               (2, 8, 64), (3, 16, 96))             # (N, C of bf16, HW); the last two: chunk lengths 64 and 96, which no other shape has
CHUNK_LENGTHS = (32, 33, 64, 65, 96, 97)            # around the two-in-flight statistics loop and the backward prefetch
MISALIGNED_SHAPE = (2, 3, 64)
KINK_SHAPE = (3, 8, 49)


def nchw_cases():
    out = []
    for j, dt in enumerate(("f32", "bf16")):
        for i, s in enumerate(NCHW_SHAPES):
            fam = "soft" if s == (1, 1, 1) else FAMILIES[(i + 2 * j) % 4]
            out.append(Case("nchw", dt, *s, NCHW_FORCED.get(s, TERM_SETS[(i + 5 * j) % 8]), fam, False, False))
        out.append(Case("nchw", dt, *MISALIGNED_SHAPE, ALL, "poison", True, False))
    return out


def nhwc_cases():
    out = []
    for j, dt in enumerate(("bf16", "f32")):
        for i, (N, C, HW) in enumerate(NHWC_SHAPES):
            out.append(Case("nhwc", dt, N, C // (1 + j), HW, TERM_SETS[(i + 3 * j) % 8], FAMILIES[(i + 1 + j) % 4], False, False))
    return out


def kink_cases():
    return [Case(lay, dt, *KINK_SHAPE, ("relu", "post"), "soft", False, True) for lay in ("nchw", "nhwc") for dt in ("f32", "bf16")]


def all_cases():
    return nchw_cases() + nhwc_cases()


def with_every_term_set(c):
    return [c._replace(terms=t) for t in TERM_SETS]


# ------------------------------------------------------------------------------------------------------------------ the reference: forward
def _nc(t):
    return None if t is None else f64(t)[:, :, None]


def _c(t):
    return f64(t)[None, :, None]


def chain(terms, x, scale, shift, pre_g=None, pre_b=None, res=None, post_g=None, post_b=None):
    """The forward of the desc.scale / shift form on x [N, C, HW], every intermediate value v and its bound b (module docstring)."""
    x, sc, sh = f64(x), _c(scale), _c(shift)
    f = types.SimpleNamespace()
    f.v1, f.b1 = x * sc + sh, R_BN * U * ((x * sc).abs() + sh.abs())
    v, b = f.v1, f.b1
    if "pre" in terms:
        g, be = _nc(pre_g), _nc(pre_b)
        v, b = g * v + be, g.abs() * b + R_PRE * U * ((g * v).abs() + be.abs())
    f.v2, f.b2 = v, b
    if "res" in terms:
        r = f64(res)
        v, b = v + r, b + R_RES * U * (v.abs() + r.abs())
    f.v3, f.b3 = v, b
    if "relu" in terms:
        v = v.clamp_min(0)
    f.v4, f.b4 = v, b
    if "post" in terms:
        g, be = _nc(post_g), _nc(post_b)
        v, b = (1 + g) * v + be, (1 + g).abs() * b + R_POST * U * (((1 + g) * v).abs() + be.abs())
    f.y, f.by = v, b
    return f


def half_ulp(ref, dtype):
    """Half the spacing of `dtype` at the reference value."""
    if dtype == BF16:
        return half_ulp_bf16(ref)
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 25))


def forward_ref(c, inp):
    """(y, bound) [N, C, HW] of mode_bn_film_act_fwd with desc.scale / shift."""
    f = chain(c.terms, inp.x, inp.scale, inp.shift, inp.pre_g, inp.pre_b, inp.res, inp.post_g, inp.post_b)
    return f.y, f.by + half_ulp(f.y, c.tdtype)


def forward_raw_ref(c, inp, weight=True, bias=True):
    """(y, bound, (gap_scale, gap_shift)) of the raw-eval form: conv_refs.epilogue_ref on the rows of x, one sample every HW rows."""
    rows = rows_of(f64(inp.x).unsqueeze(-1))
    terms = ("bn",) + (("bn_w",) if weight else ()) + (("bn_b",) if bias else ()) + c.terms
    res = None if inp.res is None else rows_of(inp.res.unsqueeze(-1))
    y, b, gaps, _ = epilogue_ref(rows, torch.zeros_like(rows), 0, terms, c.HW, inp.bn_mean, inp.bn_var, inp.bn_w, inp.bn_b, BN_EPS, inp.pre_g, inp.pre_b, res,
                                 inp.post_g, inp.post_b)
    back = lambda t: t.view(c.N, c.HW, c.C).permute(0, 2, 1).contiguous()
    return back(y), back(b) + half_ulp(back(y), c.tdtype), gaps


# ------------------------------------------------------------------------------------------------------------------ the reference: backward
def backward_ref(c, inp, training, dweight=None, dbias=None, inv_count=0.0):
    """(ref dict, bound dict) of mode_bn_film_act_bwd.  dweight / dbias [C]: the values phase 2 is given (None: this batch's own sums, as phases 0 and 1
    form them - then dx carries their bounds); inv_count as the entry takes it (<= 0: 1 / (N HW)).  Keys: dx, dresidual [N, C, HW], dweight, dbias [C],
    d_pre_gamma, d_pre_beta, d_post_gamma, d_post_beta [N, C] - those the terms call for."""
    t = c.terms
    f = chain(t, inp.x, inp.scale, inp.shift, inp.pre_g, inp.pre_b, inp.res, inp.post_g, inp.post_b)
    x, dy, sc, mu, inv = f64(inp.x), f64(inp.dy), _c(inp.scale), _c(inp.mean), _c(inp.invstd)
    zero = torch.zeros_like(x)
    dv4, b_dv4 = dy, zero
    if "post" in t:
        dv4 = dy * (1 + _nc(inp.post_g))
        b_dv4 = R_DV4 * U * dv4.abs()
    dv2, b_dv2 = dv4, b_dv4
    if "relu" in t:
        keep = f.v3 > 0
        dv2, b_dv2 = torch.where(keep, dv4, zero), torch.where(keep, b_dv4, zero)
    dv1, b_dv1 = dv2, b_dv2
    if "pre" in t:
        pg = _nc(inp.pre_g)
        dv1 = dv2 * pg
        b_dv1 = pg.abs() * b_dv2 + R_DV1 * U * dv1.abs()
    xh = (x - mu) * inv
    b_xh = R_XHAT * U * xh.abs()
    n, S = c.n_sum, c.S

    def per_row(term, err):                                              # [N, C]: S chunk sums of at most n terms, added in fp32
        return term.sum(2), err.sum(2) + (n + S - 1) * U * term.abs().sum(2)

    def per_channel(term, err):                                          # [C]: the same chunk sums folded in double, one rounding
        v = term.sum((0, 2))
        return v, err.sum((0, 2)) + n * U * term.abs().sum((0, 2)) + U * v.abs()

    ref, bound = {}, {}
    if "post" in t:
        ref["d_post_gamma"], bound["d_post_gamma"] = per_row(dy * f.v4, dy.abs() * f.b4)
        ref["d_post_beta"], bound["d_post_beta"] = per_row(dy, zero)
    if "pre" in t:
        ref["d_pre_gamma"], bound["d_pre_gamma"] = per_row(dv2 * f.v1, dv2.abs() * f.b1 + b_dv2 * (f.v1.abs() + f.b1))
        ref["d_pre_beta"], bound["d_pre_beta"] = per_row(dv2, b_dv2)
    ref["dbias"], bound["dbias"] = per_channel(dv1, b_dv1)
    ref["dweight"], bound["dweight"] = per_channel(dv1 * xh, dv1.abs() * b_xh + b_dv1 * (xh.abs() + b_xh))
    inner, b_inner = dv1, b_dv1
    if training:
        inv_m = float(torch.tensor(inv_count, dtype=F32)) if inv_count > 0 else 1.0 / (c.N * c.HW)
        given = dweight is not None
        dw, db = (f64(dweight), f64(dbias)) if given else (ref["dweight"], ref["dbias"])
        b_dw, b_db = (torch.zeros_like(dw), torch.zeros_like(db)) if given else (bound["dweight"], bound["dbias"])
        mb, mw = _c(db * inv_m), _c(dw * inv_m)
        b_mb, b_mw = _c(b_db * inv_m) + R_MB * U * mb.abs(), _c(b_dw * inv_m) + R_MB * U * mw.abs()
        t3 = xh * mw
        b_t3 = (xh.abs() + b_xh) * b_mw + b_xh * mw.abs() + U * t3.abs()
        inner = dv1 - mb - t3
        b_inner = b_dv1 + b_mb + b_t3 + 2 * U * (dv1.abs() + mb.abs() + t3.abs())
    ref["dx"] = sc * inner
    bound["dx"] = sc.abs() * b_inner + U * ref["dx"].abs() + half_ulp(ref["dx"], c.tdtype)
    if "res" in t:
        ref["dresidual"], bound["dresidual"] = dv2, b_dv2 + half_ulp(dv2, c.tdtype)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------ the reference: statistics
STAT_KEYS = ("mean", "var", "invstd", "scale", "shift")
RUN_KEYS = ("running_mean", "running_var")


def stats_ref(c, x, w, b, eps, momentum, running_mean, running_var, nbt):
    """(ref dict, bound dict) of mode_bn_prepare in training (mean and var: also mode_bn_stats): the fp64 statistics of x [N, C, HW] and nn.BatchNorm2d's
    bookkeeping, under conv_refs.bn_partials_ref's bounds with the fp32 row / chunk sums' own error in front.  running_* None: those keys are left out."""
    xd = f64(x)
    psum, psq = xd.sum(2), xd.square().sum(2)
    e_sum, e_sq = c.n_sum * U * xd.abs().sum((0, 2)), c.n_sum * U * psq.sum(0)
    z = torch.zeros(c.C)
    have = running_mean is not None
    ref, bound = bn_partials_ref(psum, psq, float(c.N * c.HW), w, b, eps, momentum, running_mean if have else z, running_var if have else z, nbt, e_sum, e_sq)
    if not have:
        for k in RUN_KEYS:
            del ref[k], bound[k]
    return ref, bound


def prepare_eval_ref(running_mean, running_var, w, b, eps):
    """mode_bn_prepare with x == NULL: the five outputs from the running statistics (one partial row of count 1 whose mean and variance they are)."""
    rm, rv = f64(running_mean), f64(running_var)
    ref, bound = bn_partials_ref(rm[None], (rv + rm * rm)[None], 1.0, w, b, eps, 0.0, rm, rv, 0)
    return {k: ref[k] for k in STAT_KEYS}, {k: bound[k] for k in STAT_KEYS}


# ------------------------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """CPU tensors of one case, all logical [N, C, HW] / [N, C] / [C] (the GPU test lays the activations out and pads them).  x, res (None without the
    term), dy in the case's dtype; bn_w, bn_b fp32 and mean, invstd, scale, shift fp32: the batch statistics of the x first drawn, folded in fp64 and
    rounded (the reference takes them as given); bn_mean, bn_var: running statistics for the raw-eval form; pre_g, pre_b, post_g, post_b [N, C] fp32."""


def _seed(c):
    return (7919 * c.N + 104729 * c.C + 31 * c.HW + 17 * FAMILIES.index(c.family) + (977 if c.cl else 0) + (13 if c.dtype == "bf16" else 0)
            + (3 if c.misaligned else 0) + (5 if c.kink else 0) + sum(7 ** i for i, t in enumerate(TERMS) if t in c.terms)) % (2 ** 31)


def kink_offenders(c, inp):
    """Elements whose |v3| is within KINK_MARGIN forward bounds of the ReLU kink (the kink-exact case: its zeros, which sit on it on purpose, aside)."""
    f = chain(c.terms, inp.x, inp.scale, inp.shift, inp.pre_g, inp.pre_b, inp.res, inp.post_g, inp.post_b)
    bad = f.v3.abs() <= KINK_MARGIN * f.b3
    return bad & (inp.x != 0) if c.kink else bad


@functools.lru_cache(maxsize=32)
def inputs(c):
    g = torch.Generator().manual_seed(_seed(c))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    N, C, HW, dt = c.N, c.C, c.HW, c.tdtype
    inp = Inputs()
    x, res, dy = rn(N, C, HW), rn(N, C, HW), rn(N, C, HW)
    if c.family == "shifted":
        x = x + (8 * ru(C) - 4)[None, :, None]                          # per-channel mean up to 4 standard deviations
    if c.family == "tails":                                             # magnitudes over eleven binades
        x, res, dy = (t * 2.0 ** torch.randint(-6, 5, (N, C, HW), generator=g).double() for t in (x, res, dy))
    inp.x, inp.dy = x.to(dt), dy.to(dt)
    inp.res = res.to(dt) if "res" in c.terms else None
    inp.bn_w, inp.bn_b = (0.8 + 0.7 * rn(C)).float(), (0.3 * rn(C)).float()
    xd = f64(inp.x)
    mean, var = xd.mean((0, 2)), xd.var((0, 2), unbiased=False)
    invstd = 1 / torch.sqrt(var + float(torch.tensor(BN_EPS, dtype=F32)))
    scale = inp.bn_w.double() * invstd
    inp.mean, inp.invstd, inp.scale, inp.shift = mean.float(), invstd.float(), scale.float(), (inp.bn_b.double() - mean * scale).float()
    inp.bn_mean, inp.bn_var = (0.3 * rn(C)).float(), (0.5 + ru(C)).float()
    if c.family == "tails":
        inp.bn_var[::5] = 1e-3
    inp.pre_g, inp.pre_b = (1 + 0.3 * rn(N, C)).float(), (0.3 * rn(N, C)).float()
    inp.post_g, inp.post_b = (0.3 * rn(N, C)).float(), (0.3 * rn(N, C)).float()
    if c.kink:
        inp.shift = torch.zeros(C)
        which = torch.randint(0, 3, (N, C, HW), generator=g)
        inp.x = torch.where(which == 0, torch.zeros((), dtype=dt), torch.where(which == 1, -torch.zeros((), dtype=dt), inp.x))
        assert bool((inp.x == 0).any()) and bool(torch.signbit(inp.x[inp.x == 0]).any()) and not bool(torch.signbit(inp.x[inp.x == 0]).all())
    if "relu" in c.terms:                                               # no element within KINK_MARGIN bounds of the kink: nudge x (and the residual)
        for it in range(64):
            bad = kink_offenders(c, inp)
            if not bool(bad.any()):
                break
            step = (0.25 + ru(int(bad.sum()))) * torch.where(ru(int(bad.sum())) < 0.5, -1.0, 1.0)
            if it % 2 and inp.res is not None:
                inp.res[bad] = (inp.res[bad].double() + step).to(dt)
            else:
                inp.x[bad] = (inp.x[bad].double() + step).to(dt)
        assert not bool(kink_offenders(c, inp).any()), c.tag
    return inp


def second_batch(c):
    """Another x of the same case (the second step of the running statistics)."""
    g = torch.Generator().manual_seed(_seed(c) + 1)
    return (0.7 * torch.randn(c.N, c.C, c.HW, generator=g, dtype=torch.float64) - 0.2).to(c.tdtype)
