"""Plain fp64 restatements (CPU torch) of the attention kernels (attn.hip, attn_core.h, attn_long.hip, qkv_attn.hip), their input families, the
per-problem metric and the case matrix, shared by tests/test_gpu_attention_edges.py (which launches the kernels) and
tests/test_attention_references.py (which validates all of this without a GPU).  Inputs are the tensors the kernel reads (fp32, or bf16 already
rounded): every function widens them itself.  The backward reference is torch autograd of the forward expression with the gains expanded to a
[B, H, hd] leaf, so that the per-(sample, head) gain partials have a reference of their own.

Wrong references (`wrong=`), for the sensitivity checks: "mask+1" / "mask-1" (causal mask off by one: one future key visible / the diagonal hidden),
"swap_gains" (q_gain and k_gain exchanged: everything depends on qg * kg alone, so it stands for the two gain-partial buffers exchanged),
"padded_hd" (softmax scale and rms over 32 * ceil(hd / 32) dims), "no_clamp" (x / rms, zero rows left zero), "eps_added" (x / (rms + eps)),
keep_wrong_index() (dropout index h * B + b) and swap_partials() (two (sample, head) rows of the gain partials exchanged)."""
import math

import torch

from oracle import mode_oracle as O

EPS = 1e-6
BF16, F32 = torch.bfloat16, torch.float32

# ------------------------------------------------------------------------------------------------------------------ case matrix
BH_CYCLE = ((1, 1), (3, 3), (5, 2), (7, 1))                      # B*H % 4 = 1, 1, 2, 3: every fill of the bf16 forward's last 4-wave workgroup
FAMILIES = ("soft", "peaked", "clamped")
FWD_SHORT_T = (1, 2, 3, 4, 5, 8, 12, 15, 16)
FWD_SHORT_HD = {BF16: (16, 48, 80, 96, 112, 128), F32: (4, 20, 48, 128, 200)}
FWD_LONG_T = (17, 31, 32, 33, 47, 49, 63, 64)
FWD_LONG_HD = {BF16: (16, 48, 96, 128), F32: (20, 64, 128)}
BWD_SHORT_T = (1, 2, 3, 4, 5, 8, 15, 16)
BWD_SHORT_HD = {BF16: (8, 24, 40, 64, 120, 128), F32: (4, 12, 20, 64, 100, 128)}
BWD_LONG_T = (17, 32, 33, 63, 64)
BWD_LONG_HD = {BF16: (8, 24, 128), F32: (4, 20, 128)}
BWD_P = (0.0, 0.3)
FUSED_T, FUSED_B, FUSED_PAD = (1, 2, 3, 4, 7, 16), (1, 3, 4, 5, 9), (0, 8, 64)
START = {("fwd", F32): 1e-5, ("bwd", F32): 2e-5, ("fwd", BF16): 1.2e-2, ("bwd", BF16): 2e-2}   # the project's whole-tensor numbers, asked of every block


def fwd_cases(dtype, T):
    """(B, H, hd, family) of every forward case at this dtype and token count."""
    if T <= 16:
        return [(*BH_CYCLE[(i + j + T) % 4], hd, fam) for i, hd in enumerate(FWD_SHORT_HD[dtype]) for j, fam in enumerate(FAMILIES)]
    return [(3, 3, hd, fam) for hd in FWD_LONG_HD[dtype] for fam in FAMILIES]


def bwd_cases(dtype, T):
    """(B, H, hd, family, p) of every backward case at this dtype and token count."""
    if T <= 16:
        return [(*BH_CYCLE[(i + j + k + T) % 4], hd, fam, p) for i, hd in enumerate(BWD_SHORT_HD[dtype]) for j, fam in enumerate(FAMILIES)
                for k, p in enumerate(BWD_P)]
    return [(3, 2, hd, fam, p) for hd in BWD_LONG_HD[dtype] for fam in FAMILIES for p in BWD_P]


# ------------------------------------------------------------------------------------------------------------------ helpers
def f64(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


def bf16r(t):
    return t.to(BF16).to(t.dtype)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def heads(t, B, T, H, hd):
    """[B*T, H*hd] -> [B, H, T, hd]"""
    return t.reshape(B, T, H, hd).transpose(1, 2)


def merge(t):
    """[B, H, T, hd] -> [B*T, H*hd]"""
    B, H, T, hd = t.shape
    return t.transpose(1, 2).reshape(B * T, H * hd)


def split_qkv(qkv, B, T, H, hd):
    return tuple(heads(t, B, T, H, hd) for t in qkv.split(H * hd, dim=-1))


def causal_mask(T, wrong=None):
    if wrong == "mask+1":
        return torch.ones(T, T, dtype=torch.bool).tril(1)
    if wrong == "mask-1":
        m = torch.ones(T, T, dtype=torch.bool).tril(-1)
        m[0, 0] = True                                           # token 0 keeps itself: a row without a key has no softmax
        return m
    return torch.ones(T, T, dtype=torch.bool).tril()


def qk_rms(x, eps, n=None, wrong=None):
    """clamp(||x|| * n^-1/2, eps) as sqrt(clamp(||x||^2, eps^2 n) / n): the same number, and a finite (zero) gradient through an all-zero row."""
    n = n or x.shape[-1]
    ss = x.pow(2).sum(-1, keepdim=True)
    if wrong == "no_clamp":
        return torch.where(ss > 0, (ss / n).sqrt(), torch.ones_like(ss))
    if wrong == "eps_added":
        return (ss.clamp_min(1e-300) / n).sqrt() + eps
    return (ss.clamp_min(eps * eps * n) / n).sqrt()


def gain4(g, B, H, hd):
    """[hd] or [B, H, hd] (the expanded leaf) -> broadcastable against [B, H, T, hd]"""
    return g.reshape(1, 1, 1, hd) if g.dim() == 1 else g.reshape(B, H, 1, hd)


def attn_parts(qkv, qg, kg, B, T, H, hd, eps=EPS, keep=None, wrong=None, bf16_points=False):
    """(q_hat, k_hat, v, P after dropout) of the forward, each [B, H, T, *]; dtype of qkv (callers pass fp64, or fp32 for the fp32 gap)."""
    q, k, v = split_qkv(qkv, B, T, H, hd)
    if wrong == "swap_gains":
        qg, kg = kg, qg
    n = 32 * -(-hd // 32) if wrong == "padded_hd" else hd
    nw = wrong if wrong in ("no_clamp", "eps_added") else None
    qh = q / qk_rms(q, eps, n, nw) * gain4(qg, B, H, hd)
    kh = k / qk_rms(k, eps, n, nw) * gain4(kg, B, H, hd)
    if bf16_points:
        qh, kh = bf16r(qh), bf16r(kh)
    att = (qh @ kh.transpose(-2, -1)) / math.sqrt(n)
    att = att.masked_fill(~causal_mask(T, wrong), float("-inf")).softmax(-1)
    if keep is not None:
        att = att * keep.to(att.dtype)
    if bf16_points:
        att = bf16r(att)
    return qh, kh, v, att


def attn_ref(qkv, qg, kg, B, T, H, hd, eps=EPS, keep=None, wrong=None, dtype=torch.float64):
    """qk-RMSNorm x / clamp(||x|| hd^-1/2, eps) * g, causal softmax(q k^T / sqrt(hd)) (* keep [B, H, T, T]) @ v, heads merged: [B*T, H*hd]."""
    c = lambda t: torch.as_tensor(t).cpu().to(dtype)
    _, _, v, att = attn_parts(c(qkv), c(qg), c(kg), B, T, H, hd, eps, keep, wrong)
    return merge(att @ v)


def attn_model_bf16(qkv, qg, kg, B, T, H, hd, eps=EPS, keep=None):
    """The bf16 rounding-point model of the forward: q_hat, k_hat and the probabilities rounded to bf16 before their MFMAs, the output to bf16.  It
    sets tolerances; it is never an oracle."""
    _, _, v, att = attn_parts(f64(qkv), f64(qg), f64(kg), B, T, H, hd, eps, keep, bf16_points=True)
    return bf16r(merge(att @ v))


def attn_floor_fwd(qkv, qg, kg, B, T, H, hd, eps=EPS, keep=None):
    """The forward's absolute-value companion P @ |v|, merged like y."""
    _, _, v, att = attn_parts(f64(qkv), f64(qg), f64(kg), B, T, H, hd, eps, keep)
    return merge(att @ v.abs())


def logits_max(qkv, qg, kg, B, T, H, hd, eps=EPS):
    q, k, _ = split_qkv(f64(qkv), B, T, H, hd)
    qh = q / qk_rms(q, eps) * gain4(f64(qg), B, H, hd); kh = k / qk_rms(k, eps) * gain4(f64(kg), B, H, hd)
    att = (qh @ kh.transpose(-2, -1)) / math.sqrt(hd)
    return float(att.masked_fill(~causal_mask(T), float("-inf")).max())


def attn_bwd_ref(qkv, qg, kg, dy, B, T, H, hd, eps=EPS, keep=None, wrong=None, dtype=torch.float64, round_out=False):
    """Autograd of <attn_ref, dy>.  Returns dict(y, dqkv [B*T, 3D], dgq / dgk [B*H, hd]: the per-(sample, head) gain partials).  round_out: the bf16
    rounding-point model of the backward (inputs and dy are bf16 already; dV stored in bf16, dq | dk rounded on the way out; the partials stay fp32)."""
    c = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)
    x = c(qkv).requires_grad_(True)
    a = c(qg).expand(B, H, hd).clone().requires_grad_(True); b = c(kg).expand(B, H, hd).clone().requires_grad_(True)
    _, _, v, att = attn_parts(x, a, b, B, T, H, hd, eps, keep, wrong)
    y = merge(att @ v)
    y.backward(c(dy))
    dqkv = x.grad
    if round_out:
        dqkv = bf16r(dqkv)
    return dict(y=y.detach(), dqkv=dqkv, dgq=a.grad.reshape(B * H, hd), dgk=b.grad.reshape(B * H, hd))


def attn_bwd_floor(qkv, qg, kg, dy, B, T, H, hd, eps=EPS, keep=None):
    """The backward's absolute-value companion: the kernel's expressions in fp64 with every operand and every product replaced by its magnitude -
    P (|dP| + |sum|) instead of P (dP - sum), |g| |dxh| r + |x| <|g| |dxh|, |x|> r^3 / hd instead of the difference.  Same dict as attn_bwd_ref."""
    qkv, qg, kg, dy = f64(qkv), f64(qg), f64(kg), f64(dy)
    q, k, _ = split_qkv(qkv, B, T, H, hd)
    qh, kh, v, pd = attn_parts(qkv, qg, kg, B, T, H, hd, eps, keep)
    p = attn_parts(qkv, qg, kg, B, T, H, hd, eps)[3]
    m = torch.ones_like(p) if keep is None else keep.double()
    do = heads(dy, B, T, H, hd).abs()
    dv = pd.transpose(-2, -1) @ do
    dp = (do @ v.abs().transpose(-2, -1)) * m * causal_mask(T)
    ds = p * (dp + (p * dp).sum(-1, keepdim=True)) / math.sqrt(hd)
    dqh, dkh = ds @ kh.abs(), ds.transpose(-2, -1) @ qh.abs()
    out = {}
    for name, x, dxh, g in (("q", q, dqh, qg), ("k", k, dkh, kg)):
        n = qk_rms(x, eps)
        r, clamped = 1.0 / n, x.pow(2).sum(-1, keepdim=True) <= eps * eps * hd
        gd = g.abs() * dxh
        proj = x.abs() * (gd * x.abs()).sum(-1, keepdim=True) * r ** 3 / hd
        out["d" + name] = gd * r + torch.where(clamped, torch.zeros_like(proj), proj)
        out["dg" + name] = (dxh * x.abs() * r).sum(2).reshape(B * H, hd)
    return dict(y=merge(pd @ v.abs()), dqkv=torch.cat([merge(out["dq"]), merge(out["dk"]), merge(dv)], -1), dgq=out["dgq"], dgk=out["dgk"])


def keep_wrong_index(seed, B, H, T, p):
    """The dropout multiplier with the problem index built as h * B + b instead of b * H + h."""
    return O.attn_keep_scale(seed, H, B, T, p).transpose(0, 1).contiguous()


def swap_partials(part, i=0, j=1):
    out = part.clone()
    out[[i, j]] = part[[j, i]]
    return out


# ------------------------------------------------------------------------------------------------------------------ input families
class Inputs:
    """qkv [B*T, 3D] and dy [B*T, D] in `dtype`, qg / kg [hd] fp32 (qg != kg), clamped = {"q": {(b, h, t), ..}, "k": {..}}."""


def make_inputs(family, B, T, H, hd, dtype, seed=0):
    D = H * hd
    s = 1000 * seed + 131 * T + 17 * hd + 7 * B + H
    inp = Inputs()
    inp.B, inp.T, inp.H, inp.hd, inp.dtype, inp.family = B, T, H, hd, dtype, family
    qkv = rnd(B * T, 3 * D, seed=s).to(dtype).double().view(B, T, 3, H, hd)          # rounded first: the structure below is exact in bf16
    center = 3.0 if family == "peaked" else 1.0
    inp.qg = (center + 0.1 * rnd(hd, seed=s + 1)).float(); inp.kg = (center + 0.1 * rnd(hd, seed=s + 2)).float()
    inp.clamped = {"q": set(), "k": set()}
    if family == "peaked":
        # the last query of each sample meets a key equal to it, one equal to half of it (the same k_hat: two equal maxima) and its negative
        ql = qkv[:, T - 1, 0]
        qkv[:, 0, 1] = ql
        if T >= 2:
            qkv[:, T // 2 if T >= 3 else 1, 1] = 0.5 * ql
        if T >= 3:
            qkv[:, T - 1, 1] = -ql
    elif family == "clamped":
        for i, (which, kind, t) in enumerate((("q", "zero", 0), ("k", "zero", T - 1), ("q", "tiny", T - 1), ("k", "tiny", 0))):
            b, h = divmod(i % (B * H), H)
            if (b, h, t) in inp.clamped[which]:
                continue                                         # T = 1 with one problem: the zero row keeps the place
            row = qkv[b, t, 0 if which == "q" else 1, h]
            if kind == "zero":
                row.zero_()
            else:
                row.mul_(1e-8 / row.pow(2).mean().sqrt())
            inp.clamped[which].add((b, h, t))
    elif family != "soft":
        raise ValueError(family)
    inp.qkv = qkv.reshape(B * T, 3 * D).to(dtype)
    inp.dy = rnd(B * T, D, seed=s + 3).to(dtype)
    if family == "peaked" and hd == 128:
        assert logits_max(inp.qkv, inp.qg, inp.kg, B, T, H, hd) > 88.8                # exp() of it overflows fp32
    if family == "clamped":
        for which, c in ((0, "q"), (1, "k")):
            for b, h, t in inp.clamped[c]:
                assert float(inp.qkv.double().view(B, T, 3, H, hd)[b, t, which, h].pow(2).mean().sqrt()) < EPS
    return inp


# ------------------------------------------------------------------------------------------------------------------ metric
def blocks(t, B, T, H, hd):
    """[B*T, n*H*hd] -> [n, B, H, T, hd]"""
    n = t.shape[1] // (H * hd)
    return t.reshape(B, T, n, H, hd).permute(2, 0, 3, 1, 4)


def block_errors(got, ref, floor, B, T, H, hd, names, clamped=None):
    """The per-problem metric.  got / ref / floor [B*T, len(names)*H*hd].  Per part and (sample, head): ||got - ref|| over the [T, hd] block against
    ||ref_block|| + floor_block (floor None: no floor term); clamped rows are taken out of their block and compared row by row in the same way.
    Returns a list of (err, ref norm, floor norm, label)."""
    g, r = blocks(f64(got), B, T, H, hd), blocks(f64(ref), B, T, H, hd)
    fl = None if floor is None else blocks(f64(floor), B, T, H, hd)
    out = []
    for pi, name in enumerate(names):
        special = (clamped or {}).get({"dq": "q", "dk": "k"}.get(name), ())
        rest = torch.ones(B, H, T, dtype=torch.bool)
        for b, h, t in special:
            rest[b, h, t] = False
            out.append((float((g[pi, b, h, t] - r[pi, b, h, t]).norm()), float(r[pi, b, h, t].norm()),
                        0.0 if fl is None else float(fl[pi, b, h, t].norm()), f"{name}[b={b},h={h},row {t}]"))
        w = rest[..., None].double()
        e, n = ((g[pi] - r[pi]) * w).flatten(2).norm(dim=2), (r[pi] * w).flatten(2).norm(dim=2)
        f = torch.zeros_like(n) if fl is None else (fl[pi] * w).flatten(2).norm(dim=2)
        out += [(float(e[b, h]), float(n[b, h]), float(f[b, h]), f"{name}[b={b},h={h}]") for b in range(B) for h in range(H)]
    return out


def row_errors(got, ref, floor, name):
    """The same metric per row of the gain partials [B*H, hd]."""
    g, r = f64(got), f64(ref)
    f = torch.zeros_like(r) if floor is None else f64(floor)
    return [(float((g[i] - r[i]).norm()), float(r[i].norm()), float(f[i].norm()), f"{name}[{i}]") for i in range(r.shape[0])]


def worst(errs):
    """max over blocks of err / (||ref|| + floor): the case passes at rtol when this is <= rtol.  A block that is exactly right counts 0."""
    w, where = 0.0, ""
    for e, n, f, label in errs:
        v = 0.0 if e == 0.0 else (e / (n + f) if n + f > 0 else float("inf"))
        if not v <= w:
            w, where = v, label
    return w, where


def floor_dominates(errs):
    """How many blocks have a floor term above the relative term."""
    return sum(1 for _, n, f, _ in errs if f > n)


def use_floor(family):
    """Only `peaked` takes the floor term: it is there for the saturated softmax, whose dq / dk blocks cancel to ~1e-11 (exactly 0 at T = 1).  `soft`
    and `clamped` blocks are held to rtol * ||ref_block|| alone (the clamped rows by the row split): the all-magnitude companion is 3 to 70 times
    ||ref_block|| on ordinary data (|sum a| <= sum |a|, always), so adding it there would only loosen the project's bound.  LABNOTES.md, "Attention
    kernels at their edges"."""
    return family == "peaked"


# ------------------------------------------------------------------------------------------------------------------ references and bounds of a case
def fwd_case(inp, keep=None):
    """fp64 reference, floor, the reference-alone gap (fp32 torch for fp32, the rounding-point model for bf16) and the bound of one forward case:
    rtol = max(starting value, 4 x gap)."""
    a = (inp.qkv, inp.qg, inp.kg, inp.B, inp.T, inp.H, inp.hd)
    ref = attn_ref(*a, keep=keep)
    floor = attn_floor_fwd(*a, keep=keep) if use_floor(inp.family) else None
    model = attn_model_bf16(*a, keep=keep) if inp.dtype == BF16 else attn_ref(*a, keep=keep, dtype=F32)
    gap, where = worst(block_errors(model, ref, floor, inp.B, inp.T, inp.H, inp.hd, ("y",)))
    start = START["fwd", inp.dtype]
    return dict(ref=ref, floor=floor, gap=gap, gap_at=where, start=start, rtol=max(start, 4 * gap))


def fwd_errors(y, case, inp):
    return block_errors(y, case["ref"], case["floor"], inp.B, inp.T, inp.H, inp.hd, ("y",))


def bwd_case(inp, keep=None):
    a = (inp.qkv, inp.qg, inp.kg, inp.dy, inp.B, inp.T, inp.H, inp.hd)
    ref = attn_bwd_ref(*a, keep=keep)
    floor = attn_bwd_floor(*a, keep=keep) if use_floor(inp.family) else None
    model = attn_bwd_ref(*a, keep=keep, round_out=True) if inp.dtype == BF16 else attn_bwd_ref(*a, keep=keep, dtype=F32)
    gap, where = worst(bwd_errors(model["dqkv"], model["dgq"], model["dgk"], dict(ref=ref, floor=floor), inp))
    start = START["bwd", inp.dtype]
    return dict(ref=ref, floor=floor, gap=gap, gap_at=where, start=start, rtol=max(start, 4 * gap))


def bwd_errors(dqkv, dgq, dgk, case, inp, ref=None):
    ref, fl = ref or case["ref"], case["floor"]
    return (block_errors(dqkv, ref["dqkv"], fl and fl["dqkv"], inp.B, inp.T, inp.H, inp.hd, ("dq", "dk", "dv"), inp.clamped)
            + row_errors(dgq, ref["dgq"], fl and fl["dgq"], "dgq") + row_errors(dgk, ref["dgk"], fl and fl["dgk"], "dgk"))


# ------------------------------------------------------------------------------------------------------------------ sensitivity
SEED = 1234
WRONGS = ("mask+1", "mask-1", "swap_gains", "padded_hd", "no_clamp", "eps_added", "keep_idx", "swap_partials")
# (path, dtype, B, T, H, hd, family, p): one representative shape per family, path, token range and dtype
SENSITIVITY = [(path, dtype, B, T, H, hd[dtype], family, p)
               for path, B, H, p, shapes in (("fwd", 3, 3, 0.3, ((12, {BF16: 48, F32: 48}), (17, {BF16: 48, F32: 20}))),
                                            ("bwd", 3, 2, 0.3, ((8, {BF16: 24, F32: 20}), (17, {BF16: 24, F32: 20}))))
               for T, hd in shapes for dtype in (BF16, F32) for family in FAMILIES]


def applicable_wrongs(path, dtype, T, hd, family, p, B, H):
    """The wrong references a case can tell apart.  Each restriction is a property of the reference, shown by tests/test_attention_references.py:
    - padded_hd scales every logit by sqrt(32 ceil(hd / 32) / hd) <= 1.16: far outside fp32's bound, a few times bf16's at best (one time where the
      softmax is saturated), so bf16 takes it for `soft` only, with the margin PADDED_BF16_MARGIN instead of 10;
    - eps_added changes one tiny row's q_hat by 1 %: the forward moves by about its fp32 bound, the row's own gradient by 20 times it (fp32 backward);
    - swap_gains: the forward and dq | dk | dv depend on qg * kg alone, and so do the partials (dgq = kg * S, dgk = qg * S with one S): exchanging the
      gains changes nothing anywhere.  What can go wrong is the two partial BUFFERS exchanged; that moves them by |qg - kg| / |g| ~ 0.1 (fp32 only);
    - swap_partials: not under the floor term (`peaked`), which is ~50 times a partial row's norm."""
    w = ["mask+1", "mask-1"] if T >= 2 else []
    if hd % 32 and (dtype == F32 or family == "soft"):
        w.append("padded_hd")
    if family == "clamped":
        w.append("no_clamp")
        if dtype == F32 and path == "bwd":
            w.append("eps_added")
    if p > 0 and B >= 2 and H >= 2:
        w.append("keep_idx")
    if path == "bwd" and T >= 2:
        w += (["swap_gains"] if dtype == F32 else []) + (["swap_partials"] if B * H >= 2 and not use_floor(family) else [])
    return w


PADDED_BF16_MARGIN = 4


def wrong_errors(path, wrong, inp, case, keep, got):
    """The metric of `got` (y, or dict(dqkv, dgq, dgk)) against the deliberately wrong reference, with the case's own floor."""
    kw = dict(keep=keep_wrong_index(SEED, inp.B, inp.H, inp.T, 0.3) if wrong == "keep_idx" else keep,
              wrong=None if wrong in ("keep_idx", "swap_partials", "swap_gains") else wrong)
    if path == "fwd":
        bad = attn_ref(inp.qkv, inp.qg, inp.kg, inp.B, inp.T, inp.H, inp.hd, **kw)
        return block_errors(got, bad, case["floor"], inp.B, inp.T, inp.H, inp.hd, ("y",))
    bad = attn_bwd_ref(inp.qkv, inp.qg, inp.kg, inp.dy, inp.B, inp.T, inp.H, inp.hd, **kw)
    if wrong == "swap_partials":
        bad["dgq"], bad["dgk"] = swap_partials(bad["dgq"]), swap_partials(bad["dgk"])
    if wrong == "swap_gains":
        bad["dgq"], bad["dgk"] = bad["dgk"], bad["dgq"]
    return bwd_errors(got["dqkv"], got["dgq"], got["dgk"], case, inp, ref=bad)
