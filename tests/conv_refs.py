"""The fp64 reference of the implicit-GEMM convolution (include/mode_hip.h: ModeGemmDesc.a_tap_cols / a_rows_tap_stride, ModeConvBnDesc), the
per-element bound, the input families, the launchers' dispatch predicates and the case table, shared by tests/test_gpu_conv_edges.py (which launches
the kernels of csrc/conv_gemm.hip) and tests/test_conv_references.py (which validates all of this without a GPU).  The reference is written from the
header's description of the operation: plain torch on the CPU, operands widened to fp64 here, at two levels - the index TABLE
(C[m, n] = sum_t sum_c A[idx[t * stride + m], c] W_t[c, n], a negative index = a zero row) and the CONVOLUTION (F.conv2d in fp64 and its autograd).

The bound (LABNOTES.md, "Implicit-GEMM convolution against fp64"), per element, u = 2^-23, K = taps * tap_k, S = sum_t sum_c |a| |w|:
  accumulator                 (K + 2) u S: products of bf16 operands are exact in fp32, any order of K fp32 additions errs by at most K u S
  fused epilogue              y = post(relu(pre(acc * scale + shift) + residual)), walked term by term with the fp64 value v and the bound b of each step:
    BatchNorm   v1 = acc scale + shift        b1 = |scale| b_acc + (|acc| + b_acc) e_scale + e_shift + R_BN u (|acc scale| + |shift|)
                e_scale = 4 gap_scale |scale|, e_shift = 4 gap_shift (|bias| + |mean scale|): the fp32 evaluation of 1 / sqrt(var + eps) * w and
                b - mean * scale cannot be counted from the source (sqrtf, the division), so it is MEASURED as the reference-alone gap - the same two
                expressions in fp32 torch on the CPU against fp64, relative to those magnitudes, the maximum over the channels of the case
    pre-FiLM    v2 = g v1 + beta              b2 = |g| b1 + R_PRE u (|g v1| + |beta|)
    residual    v3 = v2 + r                   b3 = b2 + R_RES u (|v2| + |r|)
    ReLU        v4 = max(v3, 0)               b4 = b3 (1-Lipschitz: the bound is on the value, no element is exempt)
    post-FiLM   v5 = (1 + g) v4 + beta        b5 = |1 + g| b4 + R_POST u (|(1 + g) v4| + |beta|)     (1 + g rounds, then the fma)
  bf16 output                 + half a bf16 unit in the last place at the reference value (gemm_refs.half_ulp_bf16), and nothing more
  stat_sum / stat_sq          "of y as stored": against the fp64 column sums / sums of squares of the kernel's OWN stored y over the valid rows of each
                              128-row tile, (rows + 1) u sum |y| and (rows + 1) u sum y^2 (bf16 values and their squares are exact in fp32; any order of
                              `rows` additions); y itself is held to the fp64 reference separately."""
import collections
import functools

import torch
import torch.nn.functional as F

from gemm_refs import U, f64, half_ulp_bf16, ratios  # noqa: F401  (ratios: re-exported for the tests)

BF16 = torch.bfloat16
W_KN = 2                                            # MODE_GEMM_W_KN (checked against _lib by test_conv_references.py)
NUM_CUS = 256                                       # pp_num_cus() on an MI355X
FAMILIES = ("soft", "tails", "poison")
TERMS = ("bn", "bn_w", "bn_b", "pre", "res", "relu", "post")
R_BN, R_PRE, R_RES, R_POST = 1, 1, 1, 2             # fp32 roundings of one epilogue step (conv_gemm.hip:255-268: one fma each; post: 1.f + g, then the fma)
BN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------ dispatch predicates
def takes_wide(M, N):
    """BN = 128 (gemm_bf16_conv_launch and mode_conv_bn_act_fwd: N % 128 == 0 and at least 384 tiles of 128 x 128)."""
    return N % 128 == 0 and -(-M // 128) * -(-N // 128) >= 384


def ring_depth(M, N, wide, forced=0):
    """NS (conv_launch): the "conv_ns" option when it is 2 or 3, else three slots below two workgroups per CU."""
    if forced:
        return 3 if forced == 3 else 2
    bn = 128 if wide else 64
    return 3 if -(-M // 128) * -(-N // bn) < 2 * NUM_CUS else 2


ALL_KERNELS = tuple((lay, bn, ns) for lay in ("fwd", "w_kn", "fuse") for bn in (64, 128) for ns in (2, 3))


# ------------------------------------------------------------------------------------------------------------------ cases
_Case = collections.namedtuple("Case", "kind layout M N tap_k taps family terms rps stats direct ns")


class Case(_Case):
    """One launch.  kind "gemm": mode_gemm with a_rows in taps, layout "fwd" / "w_kn"; kind "fused": mode_conv_bn_act_fwd (N = Cout, tap_k = Cin), terms:
    the epilogue terms present (a subset of TERMS; "bn_w" / "bn_b" need "bn"), rps: rows_per_sample, stats: stat_sum / stat_sq requested, direct: idx NULL
    (taps = 1, row m reads row m); ns: the forced "conv_ns" (0 = auto).  Leading dimensions are always padded: lda = tap_k + 8, ldw = row + 8, ldc = N + 8,
    ldr = N + 12, a_rows_tap_stride = M + 3; A has rows no index names."""
    __slots__ = ()

    K = property(lambda s: s.taps * s.tap_k)
    lda = property(lambda s: s.tap_k + 8)
    ldc = property(lambda s: s.N + 8)
    ldr = property(lambda s: s.N + 12)
    idx_stride = property(lambda s: s.M + 3)
    wrow = property(lambda s: s.taps * (s.N if s.layout == "w_kn" else s.tap_k))
    ldw = property(lambda s: s.wrow + 8)
    samples = property(lambda s: -(-s.M // s.rps) if s.rps > 0 else 1)
    m_tiles = property(lambda s: -(-s.M // 128))

    @property
    def kernel(self):
        wide = takes_wide(self.M, self.N)
        return ("fuse" if self.kind == "fused" else self.layout, 128 if wide else 64, ring_depth(self.M, self.N, wide, self.ns))

    @property
    def tag(self):
        t = f"{self.kind} {self.layout} M={self.M} N={self.N} tap_k={self.tap_k} taps={self.taps} {self.family} ns={self.ns}"
        if self.kind == "fused":
            t += f" terms={'+'.join(self.terms) or 'none'} rps={self.rps}" + (" stats" if self.stats else "") + (" direct" if self.direct else "")
        return t

    @property
    def data_key(self):
        return self._replace(ns=0)


def gemm_case(layout, M, N, tap_k, taps, family="soft", ns=0):
    return Case("gemm", layout, M, N, tap_k, taps, family, (), 1, False, False, ns)


def fused_case(M, N, tap_k, taps, terms=(), rps=1, family="soft", stats=False, direct=False, ns=0):
    terms = tuple(t for t in TERMS if t in terms)
    assert not (direct and taps != 1) and not ({"bn_w", "bn_b"} & set(terms) and "bn" not in terms)
    return Case("fused", "fwd", M, N, tap_k, taps, family, terms, rps, stats, direct, ns)


# ------------------------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """CPU tensors of one case.  A_buf [T, lda] / W_buf [rows, ldw] / res_buf [M, ldr] (the wide buffers) and their logical views A [T, tap_k], W
    (fwd: [N, K]; w_kn: [tap_k, taps * N], element (t, c, n) at [c, t * N + n]), res [M, N]; idx_buf int32 [taps * idx_stride] and its view idx [taps, M];
    dead: the rows of A that no index names; zero_tap / zero_row: the tap / output row whose every index is -1 (None when the shape has none);
    bn_mean / bn_var / bn_w / bn_b [N] fp32; pre_g / pre_b / post_g / post_b [samples, N] fp32."""


def _seed(c):
    return (7919 * c.M + 104729 * c.N + 31 * c.tap_k + 1009 * c.taps + 17 * FAMILIES.index(c.family) + 13 * c.rps + 5 * len(c.terms)
            + (977 if c.layout == "w_kn" else 0) + (3 if c.direct else 0) + sum(7 ** i for i, t in enumerate(TERMS) if t in c.terms)) % (2 ** 31)


@functools.lru_cache(maxsize=16)
def _inputs(c):
    g = torch.Generator().manual_seed(_seed(c))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    M, N, K, tk, taps = c.M, c.N, c.K, c.tap_k, c.taps
    poison = c.family == "poison"
    nan = float("nan")
    inp = Inputs()
    # ---- A: live rows (named by the table, with repeats) and dead rows (never named; NaN in the poison family)
    n_live = M if c.direct else max(1, (2 * M) // 3)
    n_dead = 3 + n_live // 16
    T = n_live + n_dead
    if c.direct:
        dead = torch.arange(n_live, T)                                  # row m reads row m: the dead rows lie behind them
    else:
        dead = torch.randperm(T, generator=g)[:n_dead].sort().values
    live = torch.tensor(sorted(set(range(T)) - set(dead.tolist())))
    A_buf = rn(T, c.lda)
    wrows = tk if c.layout == "w_kn" else N
    W_buf = rn(wrows, c.ldw) * K ** -0.5
    if c.family == "tails":                                             # a few large-magnitude entries: accumulators far out on both sides
        A_buf = torch.where(ru(T, c.lda) < 0.01, 24.0 * A_buf, A_buf)
        W_buf = torch.where(ru(wrows, c.ldw) < 0.005, 12.0 * W_buf, W_buf)
    if poison:
        A_buf[dead] = nan
        A_buf[:, tk:] = nan
        W_buf[:, c.wrow:] = nan
    inp.A_buf, inp.W_buf = A_buf.to(BF16), W_buf.to(BF16)
    inp.A, inp.W = inp.A_buf[:, :tk], inp.W_buf[:, :c.wrow]
    inp.dead = dead
    # ---- the index table: 15-30 % of -1, one tap that is -1 everywhere, one output row whose every tap is -1; the slack of the tap stride names a dead row
    inp.zero_tap = inp.zero_row = None
    if c.direct:
        inp.idx_buf = inp.idx = None
    else:
        idx = live[torch.randint(0, n_live, (taps, M), generator=g)]
        idx = torch.where(ru(taps, M) < 0.15 + 0.15 * float(ru(1)), torch.full_like(idx, -1), idx)
        if taps >= 2:
            inp.zero_tap = (taps - 1) // 2                                 # never the last tap: the ring's tail K-steps carry data
            idx[inp.zero_tap] = -1
        if M >= 2:
            inp.zero_row = M // 2
            idx[:, inp.zero_row] = -1
        buf = torch.full((taps, c.idx_stride), int(dead[0]), dtype=torch.int64)
        buf[:, :M] = idx
        inp.idx_buf = buf.reshape(-1).int()
        inp.idx = inp.idx_buf.view(taps, c.idx_stride)[:, :M]
    # ---- the fused epilogue's operands
    S = c.samples
    inp.bn_mean, inp.bn_var = (0.3 * rn(N)).float(), (0.5 + ru(N)).float()
    inp.bn_w, inp.bn_b = (0.8 + 0.7 * rn(N)).float(), (0.3 * rn(N)).float()
    if c.family == "tails":
        inp.bn_var[::5] = 1e-3                                           # scale ~ 30
        inp.bn_mean[1::7] = 4.0
    inp.pre_g, inp.pre_b = (1 + 0.3 * rn(S, N)).float(), (0.3 * rn(S, N)).float()
    inp.post_g, inp.post_b = (0.3 * rn(S, N)).float(), (0.3 * rn(S, N)).float()
    res = rn(M, c.ldr) * (8.0 if c.family == "tails" else 1.0)
    if poison:
        res[:, N:] = nan
    inp.res_buf = res.to(BF16)
    inp.res = inp.res_buf[:, :N]
    return inp


def inputs(c):
    return _inputs(c.data_key)


# ------------------------------------------------------------------------------------------------------------------ the reference, table level
def table_product(A, idx, W, M, N, tap_k, taps, w_kn):
    """(acc, S) [M, N] in fp64.  A [T, tap_k]; idx int [taps, M] (row t = the table at t * a_rows_tap_stride), None: one tap, row m reads row m;
    W: forward layout [N, taps * tap_k] (W_t[c, n] = W[n, t * tap_k + c]); with MODE_GEMM_W_KN the [tap_k, >= taps * N] view of the weight memory
    (W_t[c, n] = W[c * ldw + t * N + n])."""
    A, W = f64(A), f64(W)
    acc, S = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
    for t in range(taps):
        if idx is None:
            At = A[:M]
        else:
            it = torch.as_tensor(idx[t]).long()
            At = torch.where((it >= 0)[:, None], A[it.clamp_min(0)], torch.zeros((), dtype=torch.float64))
        Wt = W[:, t * N:(t + 1) * N] if w_kn else W[:, t * tap_k:(t + 1) * tap_k].t()
        acc += At @ Wt
        S += At.abs() @ Wt.abs()
    return acc, S


def scale_shift(mean, var, w, b, eps, dtype=torch.float64):
    """scale = bn_weight / sqrt(bn_var + bn_eps), shift = bn_bias - bn_mean * scale (weight / bias None: 1 / 0), evaluated in `dtype`."""
    mean, var = mean.to(dtype), var.to(dtype)
    scale = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32).to(dtype))
    if w is not None:
        scale = scale * w.to(dtype)
    ms = mean * scale
    shift = -ms if b is None else b.to(dtype) - ms
    return scale, shift


def scale_shift_gap(mean, var, w, b, eps):
    """The reference-alone gap of the folded BatchNorm: fp32 torch on the CPU against fp64.  Returns (gap_scale relative to |scale|, gap_shift relative to
    |bias| + |mean scale|, scale64, shift64, shift magnitude)."""
    s64, h64 = scale_shift(mean, var, w, b, eps)
    s32, h32 = scale_shift(mean, var, w, b, eps, torch.float32)
    mag = (mean.double() * s64).abs() + (0 if b is None else b.double().abs())
    d = (h32.double() - h64).abs()
    gs = float(((s32.double() - s64).abs() / s64.abs()).max())
    gh = float(torch.where(d == 0, torch.zeros_like(d), d / mag).max())
    return gs, gh, s64, h64, mag


def epilogue_ref(acc, S, K, terms, rps=1, bn_mean=None, bn_var=None, bn_w=None, bn_b=None, eps=BN_EPS, pre_g=None, pre_b=None, res=None,
                 post_g=None, post_b=None):
    """y = post(relu(pre(acc * scale + shift) + residual)) in fp64 from the fp64 accumulator, walked step by step together with its bound (module
    docstring).  terms: the epilogue terms present.  Returns (y, bound before the output rounding, (gap_scale, gap_shift), fraction clipped by ReLU)."""
    M = acc.shape[0]
    sample = torch.arange(M) // max(rps, 1)
    v, b = acc, (K + 2) * U * S
    gaps, clipped = (0.0, 0.0), 0.0
    if "bn" in terms:
        gs, gh, sc, sh, mag = scale_shift_gap(bn_mean, bn_var, bn_w if "bn_w" in terms else None, bn_b if "bn_b" in terms else None, eps)
        gaps = (gs, gh)
        e_sc, e_sh = 4 * gs * sc.abs(), 4 * gh * mag
        b = sc.abs() * b + (v.abs() + b) * e_sc + e_sh + R_BN * U * ((v * sc).abs() + sh.abs())
        v = v * sc + sh
    if "pre" in terms:
        g, be = f64(pre_g)[sample], f64(pre_b)[sample]
        b = g.abs() * b + R_PRE * U * ((g * v).abs() + be.abs())
        v = g * v + be
    if "res" in terms:
        r = f64(res)
        b = b + R_RES * U * (v.abs() + r.abs())
        v = v + r
    if "relu" in terms:
        clipped = float((v < 0).double().mean())
        v = v.clamp_min(0)
    if "post" in terms:
        g, be = f64(post_g)[sample], f64(post_b)[sample]
        b = (1 + g).abs() * b + R_POST * U * (((1 + g) * v).abs() + be.abs())
        v = (1 + g) * v + be
    return v, b, gaps, clipped


@functools.lru_cache(maxsize=8)
def _reference(c):
    inp = _inputs(c)
    acc, S = table_product(inp.A, inp.idx, inp.W, c.M, c.N, c.tap_k, c.taps, c.layout == "w_kn")
    y, b, gaps, clipped = epilogue_ref(acc, S, c.K, c.terms, c.rps, inp.bn_mean, inp.bn_var, inp.bn_w, inp.bn_b, BN_EPS, inp.pre_g, inp.pre_b, inp.res,
                                       inp.post_g, inp.post_b)
    return dict(C=y, clipped=clipped), dict(C=b + half_ulp_bf16(y)), gaps


def reference(c):
    """(reference dict, bound dict, (gap_scale, gap_shift)) of a case, shared by both ring depths."""
    return _reference(c.data_key)


def stat_ratios(y_stored, stat_sum, stat_sq, M):
    """stat_sum / stat_sq [m_tiles, N] against the fp64 column sums / sums of squares of the stored y [M, N] over the valid rows of each 128-row tile,
    under (rows + 1) u sum |y| and (rows + 1) u sum y^2.  Returns gemm_refs.ratios' list."""
    y = f64(y_stored)
    tiles = -(-M // 128)
    ref = dict(stat_sum=torch.stack([y[t * 128:(t + 1) * 128].sum(0) for t in range(tiles)]),
               stat_sq=torch.stack([y[t * 128:(t + 1) * 128].square().sum(0) for t in range(tiles)]))
    rows = torch.tensor([min(128, M - t * 128) for t in range(tiles)], dtype=torch.float64)[:, None]
    bound = dict(stat_sum=(rows + 1) * U * torch.stack([y[t * 128:(t + 1) * 128].abs().sum(0) for t in range(tiles)]),
                 stat_sq=(rows + 1) * U * ref["stat_sq"])
    return ratios(dict(stat_sum=stat_sum, stat_sq=stat_sq), ref, bound)


# ------------------------------------------------------------------------------------------------------------------ the reference, convolution level
_Conv = collections.namedtuple("Conv", "n cin cout H W kh kw sh sw ph pw")


class Conv(_Conv):
    __slots__ = ()
    ho = property(lambda s: (s.H + 2 * s.ph - s.kh) // s.sh + 1)
    wo = property(lambda s: (s.W + 2 * s.pw - s.kw) // s.sw + 1)
    rows_out = property(lambda s: s.n * s.ho * s.wo)
    rows_in = property(lambda s: s.n * s.H * s.W)
    taps = property(lambda s: s.kh * s.kw)
    tag = property(lambda s: f"conv n={s.n} {s.cin}->{s.cout} {s.H}x{s.W} k=({s.kh},{s.kw}) s=({s.sh},{s.sw}) p=({s.ph},{s.pw})")


CONVS = (
    Conv(2, 64, 128, 14, 14, 3, 3, 1, 1, 1, 1),      # 3 x 3 / 1 / 1, 392 rows: four tiles, the last partial
    Conv(2, 128, 64, 9, 7, 3, 3, 2, 2, 1, 1),        # 3 x 3 / 2 / 1 on an odd image
    Conv(3, 64, 192, 9, 9, 1, 1, 2, 2, 0, 0),        # 1 x 1 / 2
    Conv(1, 64, 64, 8, 8, 5, 5, 1, 1, 2, 2),         # 5 x 5 / 1 / 2
    Conv(2, 128, 128, 9, 6, 3, 1, 2, 1, 1, 0),       # a (3, 1) kernel, stride (2, 1), padding (1, 0)
    Conv(1, 64, 64, 4, 5, 3, 3, 1, 1, 3, 3),         # padding wider than the kernel's reach: border outputs see no input at all
    Conv(2, 64, 128, 2, 2, 3, 3, 1, 1, 1, 1),        # an image smaller than the kernel
    Conv(1, 128, 64, 7, 10, 3, 3, 1, 1, 1, 1),       # n = 1, 70 rows: one partial tile
)


@functools.lru_cache(maxsize=None)
def conv_inputs(cv):
    """x [n, cin, H, W], w [cout, cin, kh, kw], dy [n, cout, ho, wo] as bf16 CPU tensors (contiguous NCHW; the GPU test makes them channels_last),
    plus the fused epilogue's operands for rows_per_sample = ho * wo."""
    g = torch.Generator().manual_seed(sum((i + 3) * 131 ** (i % 3) * v for i, v in enumerate(cv)) % (2 ** 31))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inp = Inputs()
    inp.x = rn(cv.n, cv.cin, cv.H, cv.W).to(BF16)
    inp.w = (rn(cv.cout, cv.cin, cv.kh, cv.kw) * (cv.taps * cv.cin) ** -0.5).to(BF16)
    inp.dy = rn(cv.n, cv.cout, cv.ho, cv.wo).to(BF16)
    N = cv.cout
    inp.bn_mean, inp.bn_var = (0.3 * rn(N)).float(), (0.5 + torch.rand(N, generator=g, dtype=torch.float64)).float()
    inp.bn_w, inp.bn_b = (0.8 + 0.7 * rn(N)).float(), (0.3 * rn(N)).float()
    inp.pre_g, inp.pre_b = (1 + 0.3 * rn(cv.n, N)).float(), (0.3 * rn(cv.n, N)).float()
    inp.post_g, inp.post_b = (0.3 * rn(cv.n, N)).float(), (0.3 * rn(cv.n, N)).float()
    inp.res = rn(cv.n, N, cv.ho, cv.wo).to(BF16)
    return inp


def rows_of(t):
    """[n, C, h, w] -> the channels_last row matrix [n * h * w, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@functools.lru_cache(maxsize=None)
def conv_reference(cv):
    """F.conv2d in fp64 on the bf16-rounded operands and its autograd.  Returns dict: "y" / "S_y" [rows_out, cout] (forward and sum |x| |w|), "dx" / "S_dx"
    [rows_in, cin] (data gradient for dy and sum |dy| |w|), as channels_last row matrices."""
    inp = conv_inputs(cv)
    out = {}
    for name, ab in (("", lambda t: t), ("S_", torch.abs)):
        x = ab(f64(inp.x)).requires_grad_(True)
        y = F.conv2d(x, ab(f64(inp.w)), None, (cv.sh, cv.sw), (cv.ph, cv.pw))
        dx, = torch.autograd.grad(y, x, ab(f64(inp.dy)))
        out[name + "y"], out[name + "dx"] = rows_of(y.detach()), rows_of(dx)
    return out


def tap_tables_by_loop(cv):
    """(forward [taps, rows_out], transposed [taps, rows_in]) index tables written as plain loops over every (sample, output pixel, tap): the forward entry
    is the input row that tap pairs with the output pixel, the transposed entry the output row whose tap read the input pixel; -1 where there is none."""
    fwd = torch.full((cv.taps, cv.rows_out), -1, dtype=torch.int64)
    tr = torch.full((cv.taps, cv.rows_in), -1, dtype=torch.int64)
    for n in range(cv.n):
        for oh in range(cv.ho):
            for ow in range(cv.wo):
                o = (n * cv.ho + oh) * cv.wo + ow
                for a in range(cv.kh):
                    for b in range(cv.kw):
                        ih, iw = oh * cv.sh + a - cv.ph, ow * cv.sw + b - cv.pw
                        if 0 <= ih < cv.H and 0 <= iw < cv.W:
                            i = (n * cv.H + ih) * cv.W + iw
                            fwd[a * cv.kw + b, o] = i
                            assert tr[a * cv.kw + b, i] == -1
                            tr[a * cv.kw + b, i] = o
    return fwd, tr


def conv_as_tables(cv):
    """The table-level operands of a convolution: (A_fwd [rows_in, cin], W_fwd [cout, taps * cin], A_dgrad [rows_out, cout], W_kn [cout, taps * cin]) -
    the channels_last weight memory [cout][taps][cin] read both ways."""
    inp = conv_inputs(cv)
    wmem = inp.w.permute(0, 2, 3, 1).reshape(cv.cout, cv.taps * cv.cin)
    return rows_of(inp.x), wmem, rows_of(inp.dy), wmem


# ------------------------------------------------------------------------------------------------------------------ mode_bn_prepare_partials
def bn_partials_ref(psum, psq, count, w, b, eps, momentum, running_mean, running_var, nbt, e_sum=0.0, e_sq=0.0):
    """The fold of partial sums [rows, C] and nn.BatchNorm2d's bookkeeping in fp64 (include/mode_hip.h: mode_bn_prepare / mode_bn_prepare_partials).
    Returns (ref dict, bound dict).  Bounds, u = 2^-23 (a rounding to fp32 errs by at most u / 2 of the value; `n u` stands for up to 2 n roundings):
      mean, var      the kernel folds in double: one rounding to fp32 each -> u |mean|, u |var| + 2^-40 (sum sq / count) for the cancellation in double
      invstd         from the fp32 var (u |var| through d invstd / d var = invstd / (2 (var + eps))), + the sum, the square root, the division
      scale          + one product; shift: the fp32 mean times scale's error, + the product and the difference
      running stats  (1 - f) rounds, two products (three for the unbiased variance), one sum, on top of the fp32 mean / var.
    e_sum / e_sq [C]: what the column totals of the partials the kernel folds may be off by (0: the partials are given, as here; bn_refs.stats_ref: the
    fp32 row sums of mode_bn_prepare's own pass); they enter mean as e_sum / count and var as e_sq / count + (2 |mean| + e_sum / count) e_sum / count."""
    ps, pq = f64(psum), f64(psq)
    m = ps.sum(0) / count
    ex2 = pq.sum(0) / count
    v = (ex2 - m * m).clamp_min(0)
    epsd = float(torch.tensor(eps, dtype=torch.float32))
    inv = 1 / torch.sqrt(v + epsd)
    wd = torch.ones_like(m) if w is None else f64(w)
    bd = torch.zeros_like(m) if b is None else f64(b)
    sc = wd * inv
    sh = bd - m * sc
    f = float(torch.tensor(momentum, dtype=torch.float32)) if momentum >= 0 else float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(nbt + 1), dtype=torch.float32))
    unbias = count / max(count - 1.0, 1.0)
    rm, rv = f64(running_mean), f64(running_var)
    ref = dict(mean=m, var=v, invstd=inv, scale=sc, shift=sh, running_mean=rm * (1 - f) + m * f, running_var=rv * (1 - f) + v * unbias * f)
    e_m = e_sum / count
    b_m, b_v = U * m.abs() + e_m, U * v + 2.0 ** -40 * (ex2 + m * m) + e_sq / count + (2 * m.abs() + e_m) * e_m
    b_inv = inv * (0.5 * b_v / (v + epsd)) + 2 * U * inv
    b_sc = wd.abs() * b_inv + U * sc.abs()
    b_sh = b_m * sc.abs() + m.abs() * b_sc + 2 * U * (bd.abs() + (m * sc).abs())
    bound = dict(mean=b_m, var=b_v, invstd=b_inv, scale=b_sc, shift=b_sh,
                 running_mean=f * b_m + 3 * U * ((rm * (1 - f)).abs() + (m * f).abs()),
                 running_var=f * unbias * b_v + 4 * U * ((rv * (1 - f)).abs() + (v * unbias * f).abs()))
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------ the case table
TABLE_M, TABLE_N = (1, 127, 128, 129, 300), (8, 56, 64, 72, 136, 192)
TABLE_TAPS = ((64, 1), (64, 2), (64, 3), (64, 9), (128, 1), (128, 2), (128, 3), (128, 9))      # (tap_k, taps): nk = 1, 2, 3 and >= 4 K-steps of 64
WIDE = ((2950, 2048, 64, 1), (2950, 2048, 64, 3), (6100, 1024, 64, 2))                        # t128 = 384: BN = 128
NARROW_NEIGHBOUR = (2944, 2048, 64, 1)                                                        # t128 = 368: BN = 64 at the same N
LAYOUTS = ("fwd", "w_kn")


def table_cases(layout, tap_k, taps):
    """Every M x N of the table at one (tap_k, taps); the families rotate over the shapes."""
    shapes = [(M, N) for M in TABLE_M for N in TABLE_N]
    return [gemm_case(layout, M, N, tap_k, taps, FAMILIES[(i + taps + tap_k // 64) % 3]) for i, (M, N) in enumerate(shapes)]


def wide_cases(layout):
    return [gemm_case(layout, *s, family=f) for s, f in zip(WIDE + (NARROW_NEIGHBOUR,), ("soft", "poison", "tails", "soft"))]


RESNET = (("bn", "bn_w", "bn_b", "relu"), ("bn", "bn_w", "bn_b", "res", "relu"), ("bn", "bn_w", "bn_b", "pre", "res", "relu"),
          ("bn", "bn_w", "bn_b", "pre", "res", "relu", "post"))
ALONE = ((), ("bn",), ("bn", "bn_w"), ("bn", "bn_b"), ("pre",), ("res",), ("relu",), ("post",))
FUSED_SHAPES = ((300, 72, 64, 9, 49), (129, 8, 64, 2, 9), (257, 64, 128, 3, 128), (450, 192, 64, 1, 200), (130, 72, 64, 3, 1))    # (M, Cout, Cin, taps, rps)
FUSED_WIDE = (2950, 2048, 64, 1, 200)


def fused_cases():
    """Each epilogue term alone and all of them at M = 300, Cout = 72 (rows_per_sample = 49: a tile straddles three samples); the ResNet-block
    combinations over the shapes (rows_per_sample 1, 9, 49, 128, 200: at 200 a sample spans tiles); idx NULL; the wide kernel."""
    out = [fused_case(300, 72, 64, 9, t, 49, FAMILIES[i % 3]) for i, t in enumerate(ALONE + (TERMS,))]
    for i, (M, N, tk, tp, rps) in enumerate(FUSED_SHAPES):
        out += [fused_case(M, N, tk, tp, t, rps, ("tails", "poison", "soft")[(i + j) % 3]) for j, t in enumerate(RESNET)]
    out += [fused_case(450, 192, 64, 1, t, 200, "poison", direct=True) for t in ((), RESNET[3])]
    out += [fused_case(*FUSED_WIDE[:4], RESNET[3], FUSED_WIDE[4], "tails"), fused_case(*FUSED_WIDE[:4], RESNET[1], FUSED_WIDE[4], "poison", direct=True)]
    return list(dict.fromkeys(out))


def stat_cases():
    """The training forward: no epilogue terms, stat_sum / stat_sq, a partial last tile; BN = 64 (Cout 72: an 8-column n-tile; Cout 192) and BN = 128."""
    return [fused_case(300, 72, 64, 3, stats=True, family="tails"), fused_case(129, 192, 128, 2, stats=True, family="poison"),
            fused_case(2950, 2048, 64, 1, stats=True, family="soft"), fused_case(70, 64, 64, 1, stats=True, family="soft", direct=True)]


def all_cases():
    """Every launch of the table-level GPU tests: each case under conv_ns 2 and 3."""
    base = [c for lay in LAYOUTS for tk, tp in TABLE_TAPS for c in table_cases(lay, tk, tp)] + [c for lay in LAYOUTS for c in wide_cases(lay)]
    base += fused_cases() + stat_cases()
    return [c._replace(ns=ns) for c in base for ns in (2, 3)]


# ------------------------------------------------------------------------------------------------------------------ report
class Report:
    """Worst err / bound per (kernel, output) of one test, printed at its end; a ratio above 1 fails the test."""

    def __init__(self, what):
        self.what, self.worst, self.failed, self.gaps = what, collections.OrderedDict(), [], collections.OrderedDict()

    def add(self, kernel, tag, rs, gaps=None):
        name_of = "<%s, %d, NS=%d>" % kernel if isinstance(kernel, tuple) else kernel
        if gaps and max(gaps) > 0:
            old = self.gaps.get(name_of, (0.0, 0.0))
            self.gaps[name_of] = (max(old[0], gaps[0]), max(old[1], gaps[1]))
        for name, q, idx in rs:
            key = (name_of, name)
            if key not in self.worst or q > self.worst[key][0]:
                self.worst[key] = (q, f"{tag} {name}{list(idx)}")
            if not q <= 1.0:
                self.failed.append(f"{tag}: {name}{list(idx)} err / bound = {q:.3g}")

    def fail(self, msg):
        self.failed.append(msg)

    def close(self):
        for (kernel, name), (q, where) in self.worst.items():
            print(f"{self.what} | {kernel} {name}: worst err / bound {q:.3g} ({where})")
        for kernel, (gs, gh) in self.gaps.items():
            print(f"{self.what} | {kernel}: reference-alone gap scale {gs:.3g}, shift {gh:.3g}")
        assert not self.failed, "\n".join(self.failed[:40]) + f"\n({len(self.failed)} failures)"
