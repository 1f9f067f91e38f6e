"""The attention kernels at their edges against the fp64 references of tests/attn_refs.py (validated on the CPU by
tests/test_attention_references.py): the stand-alone forward for T <= 16 (attn_bf16_kernel<1..4>, attn_f32_kernel) and 16 < T <= 64 (attn_long.hip),
the fused QKV + attention launch, and the backward in both token ranges and both forms of its matrix products.

Three input families - today's soft softmax, a saturated one (gains ~3, a key aligned with the last query: a logit of ~100 at head_dim 128) and rows
inside the qk-norm's eps clamp - at token counts from 1, at every head dim class of the contract, with NaN-prefilled outputs between canary rows.  The
metric is per (sample, head) block, clamped rows row by row; a case's bound is max(the project's number, 4 x the reference-alone gap measured for that
case before the launch).  Dropout masks come from oracle.mode_oracle.attn_keep_scale, never from the kernel.  One shape per family, path and dtype is
also held against each deliberately wrong reference, which the kernel must miss."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
from attn_refs import BF16, F32  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402

UNSUPPORTED = -2


def dev(t):
    return t.to("cuda")


class Report:
    """Worst err / (||ref|| + floor) per (family, quantity) of one test, next to the bound of the case it came from; printed at the end of the test."""

    def __init__(self, what):
        self.what, self.worst, self.failed, self.rule = what, collections.OrderedDict(), [], 0

    def add(self, errs, case, family, tag):
        self.rule += case["rtol"] > case["start"]
        by_qty = collections.defaultdict(list)
        for e in errs:
            by_qty[e[3].split("[")[0]].append(e)
        for qty, es in by_qty.items():
            w, where = R.worst(es)
            old = self.worst.get((family, qty))
            if old is None or w / case["rtol"] > old[0] / old[1]:
                self.worst[family, qty] = (w, case["rtol"], f"{tag} {where}")
            if not w <= case["rtol"]:
                self.failed.append(f"{tag} {family} {where}: {w:.3e} > {case['rtol']:.3e} (reference-alone gap {case['gap']:.2e})")

    def fail(self, msg):
        self.failed.append(msg)

    def close(self):
        for (family, qty), (w, rtol, where) in self.worst.items():
            print(f"{self.what} {family} {qty}: worst {w:.2e} of bound {rtol:.2e} ({where})")
        print(f"{self.what}: {self.rule} cases took the 4x rule")
        assert not self.failed, "\n".join(self.failed)


def launch_fwd(inp, p=0.0, sample=None):
    """The forward into a Guarded output; sample: that sample alone, as a batch of one."""
    B, D = (inp.B, inp.H * inp.hd)
    qkv = inp.qkv if sample is None else inp.qkv.view(B, inp.T, 3 * D)[sample].reshape(inp.T, 3 * D)
    nb = B if sample is None else 1
    y = H.Guarded(nb * inp.T, D, inp.dtype)
    rc = H.attn(dev(qkv.contiguous()), dev(inp.qg), dev(inp.kg), nb, inp.T, inp.H, inp.hd, seed=R.SEED, p_drop=p, out=y)
    torch.cuda.synchronize()
    return rc, y


def launch_bwd(inp, p=0.0, sample=None):
    B, D = (inp.B, inp.H * inp.hd)
    qkv, dy = inp.qkv, inp.dy
    if sample is not None:
        qkv, dy = qkv.view(B, inp.T, 3 * D)[sample].reshape(inp.T, 3 * D), dy.view(B, inp.T, D)[sample].reshape(inp.T, D)
    nb = B if sample is None else 1
    out = H.attn_bwd(dev(qkv.contiguous()), dev(inp.qg), dev(inp.kg), dev(dy.contiguous()), nb, inp.T, inp.H, inp.hd, seed=R.SEED, p_drop=p)
    torch.cuda.synchronize()
    return out


def keep_of(inp, p):
    return O.attn_keep_scale(R.SEED, inp.B, inp.H, inp.T, p) if p else None


def check_fwd(rep, inp, p=0.0):
    """One forward case; returns (y on the CPU, its case) for the sensitivity checks."""
    tag = f"B={inp.B} H={inp.H} T={inp.T} hd={inp.hd} p={p}"
    case = R.fwd_case(inp, keep_of(inp, p))                                 # reference, gap and bound: before the launch
    rc, y = launch_fwd(inp, p)
    if rc != 0 or not y.intact() or bool(torch.isnan(y.t).any()):
        rep.fail(f"{tag} {inp.family}: status {rc}, canaries intact {y.intact()}, NaN left {bool(torch.isnan(y.t).any())}")
        return None, case
    got = y.t.cpu()
    rep.add(R.fwd_errors(got, case, inp), case, inp.family, tag)
    D = inp.H * inp.hd
    if p == 0.0:
        # token 0 has one key: exp(0) = 1, sum = 1, and 1 * v is exact in both dtypes - its output is its own v, bit for bit
        if not torch.equal(got.view(inp.B, inp.T, D)[:, 0], inp.qkv.view(inp.B, inp.T, 3 * D)[:, 0, 2 * D:]):
            rep.fail(f"{tag} {inp.family}: token 0 is not its own v")
        if inp.B > 1:                                                       # a problem's bits do not depend on the batch around it
            rc1, y1 = launch_fwd(inp, sample=inp.B - 1)
            if rc1 != 0 or not y1.intact() or not torch.equal(y1.t.cpu(), got[-inp.T:]):
                rep.fail(f"{tag} {inp.family}: the last sample alone differs from the same sample in the batch")
    return got, case


def check_bwd(rep, inp, p=0.0, form=""):
    tag = f"B={inp.B} H={inp.H} T={inp.T} hd={inp.hd} p={p}{form}"
    keep = keep_of(inp, p)
    case = R.bwd_case(inp, keep)
    rc, dqkv, pq, pk = launch_bwd(inp, p)
    outs = (dqkv, pq, pk)
    if rc != 0 or not all(o.intact() for o in outs) or any(bool(torch.isnan(o.t).any()) for o in outs):
        rep.fail(f"{tag} {inp.family}: status {rc}, canaries intact {[o.intact() for o in outs]}, NaN left {[bool(torch.isnan(o.t).any()) for o in outs]}")
        return None, case
    got = dict(dqkv=dqkv.t.cpu(), dgq=pq.t.cpu(), dgk=pk.t.cpu())
    rep.add(R.bwd_errors(got["dqkv"], got["dgq"], got["dgk"], case, inp), case, inp.family, tag)
    if not form and (inp.dtype == F32 or inp.hd % 16 == 0):                 # (the bf16 forward takes head_dim % 16 == 0 only)
        # the forward with the same seed agrees with the reference that used the same mask
        fcase = R.fwd_case(inp, keep)
        rcf, y = launch_fwd(inp, p)
        if rcf != 0 or not y.intact():
            rep.fail(f"{tag} {inp.family}: forward status {rcf}")
        else:
            rep.add(R.fwd_errors(y.t.cpu(), fcase, inp), fcase, inp.family, tag)
    if not form and p == 0.0 and inp.B > 1:                                 # a problem's bits do not depend on the batch around it
        rc1, d1, q1, k1 = launch_bwd(inp, sample=inp.B - 1)
        same = rc1 == 0 and all(o.intact() for o in (d1, q1, k1)) and torch.equal(d1.t.cpu(), got["dqkv"][-inp.T:]) \
            and torch.equal(q1.t.cpu(), got["dgq"][-inp.H:]) and torch.equal(k1.t.cpu(), got["dgk"][-inp.H:])
        if not same:
            rep.fail(f"{tag} {inp.family}: the last sample alone differs from the same sample in the batch")
    return got, case


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("T", R.FWD_SHORT_T + R.FWD_LONG_T)
def test_forward(T, dtype):
    """Every head dim and family at this token count (attn_refs.fwd_cases), then dropout at p = 0.3 and 0.9 on one head dim per family."""
    rep = Report(f"forward {dtype} T={T}")
    cases = R.fwd_cases(dtype, T)
    for B, Hh, hd, family in cases:
        check_fwd(rep, R.make_inputs(family, B, T, Hh, hd, dtype))
    for i, p in enumerate((0.3, 0.9)):
        for j, family in enumerate(R.FAMILIES):
            B, Hh, hd, _ = cases[(3 * (T + i + j)) % len(cases)]
            check_fwd(rep, R.make_inputs(family, max(B, 2), T, max(Hh, 2), hd, dtype), p)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("T", R.BWD_SHORT_T + R.BWD_LONG_T)
def test_backward(T, dtype):
    """Every head dim, family and dropout rate at this token count (attn_refs.bwd_cases); for T <= 16 and head_dim % 16 == 0 both forms of the five
    matrix products ("attn_bwd_mfma" 1 and 0)."""
    rep = Report(f"backward {dtype} T={T}")
    lib = L.load()
    for B, Hh, hd, family, p in R.bwd_cases(dtype, T):
        inp = R.make_inputs(family, B, T, Hh, hd, dtype)
        check_bwd(rep, inp, p)
        if T <= 16 and hd % 16 == 0:
            assert lib.mode_set_option(b"attn_bwd_mfma", 0) == 0
            try:
                check_bwd(rep, inp, p, form=" VALU")
            finally:
                lib.mode_set_option(b"attn_bwd_mfma", 1)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ fused QKV + attention
@pytest.mark.parametrize("T", R.FUSED_T)
def test_fused_qkv_attention(T):
    """mode_qkv_attn_fwd with peaked gains, one all-zero h row under a zero bias (its q, k and v are zero: the clamp) and padded leading dimensions:
    bit-equal to mode_gemm(EPI_BIAS) + mode_attn_block_fwd on the same strided h and weight in all four geometries, the pad columns of y untouched,
    and inside the forward bound of the fp64 reference on the q | k | v the GEMM produced.

    The GEMM of the bit comparison is the k-ordered tiled kernel ("gemm_skinny_rows" 0).  Up to 32 rows mode_gemm otherwise takes the weight streamer
    of gemm_bf16_skinny.hip, which cuts K into one slice per wave: its fp32 sums differ from the k-ordered chain in the last bit, and about one bf16
    q | k | v element in 1e5 rounds the other way (8 of the 60 shapes here at T <= 7).  Against that default dispatch the fused result is held to the
    fp64 bound only, and the count of differing elements is printed."""
    rep = Report(f"fused T={T}")
    lib = L.load()
    Hh, hd = 2, 128
    D = Hh * hd
    differing = compared = 0
    for B in R.FUSED_B:
        for r in range(3):
            ph, pw, py = (R.FUSED_PAD[(r + k) % 3] for k in range(3))
            tag = f"B={B} T={T} ldh=D+{ph} ldw=D+{pw} ldy=D+{py}"
            s = 100 * T + 10 * B + r
            hbuf = R.rnd(B * T, D + ph, seed=s).to(BF16)
            hbuf[(B * T) // 2] = 0
            wbuf = (R.rnd(3 * D, D + pw, seed=s + 1) * D ** -0.5).to(BF16)
            qg, kg = (3 + 0.1 * R.rnd(hd, seed=s + 2)).float(), (3 + 0.1 * R.rnd(hd, seed=s + 3)).float()
            hd_, wd_ = dev(hbuf), dev(wbuf)
            h, w, bias, qgd, kgd = hd_[:, :D], wd_[:, :D], torch.zeros(3 * D, device="cuda"), dev(qg), dev(kg)
            assert lib.mode_set_option(b"gemm_skinny_rows", 0) == 0
            try:
                qkv = H.gemm(h, w, epilogue=L.EPI_BIAS, bias=bias)
            finally:
                lib.mode_set_option(b"gemm_skinny_rows", 32)
            y2 = H.attn(qkv, qgd, kgd, B, T, Hh, hd)
            if B * T <= 32:
                y3 = H.attn(H.gemm(h, w, epilogue=L.EPI_BIAS, bias=bias), qgd, kgd, B, T, Hh, hd)
                differing += int((y3 != y2).sum()); compared += y2.numel()
            try:
                for waves, w3 in ((8, 1), (8, 0), (4, 1), (4, 0)):
                    assert lib.mode_set_option(b"qkv_attn_waves", waves) == 0 and lib.mode_set_option(b"qkv_attn_w3", w3) == 0
                    out = H.Guarded(B * T, D + py, BF16)
                    rc, _ = H.qkv_attn(h, w, bias, qgd, kgd, B, T, Hh, D=D, out=out)
                    torch.cuda.synchronize()
                    ok = rc == 0 and out.intact() and bool(torch.isnan(out.t[:, D:]).all()) and torch.equal(out.t[:, :D], y2)
                    if not ok:
                        rep.fail(f"{tag} waves={waves} w3={w3}: status {rc}, canaries intact {out.intact()}, or not the two kernels' bits")
            finally:
                lib.mode_set_option(b"qkv_attn_waves", 8); lib.mode_set_option(b"qkv_attn_w3", 1)
            inp = R.Inputs()
            inp.B, inp.T, inp.H, inp.hd, inp.dtype, inp.family, inp.clamped = B, T, Hh, hd, BF16, "peaked", {}
            inp.qkv, inp.qg, inp.kg = qkv.cpu(), qg, kg
            z = (B * T) // 2
            assert not bool(inp.qkv[z].any())                                # the zero row's q, k and v are zero
            case = R.fwd_case(inp)
            rep.add(R.fwd_errors(y2.cpu(), case, inp), case, "peaked", tag)
            if B * T <= 32:
                rep.add(R.fwd_errors(y3.cpu(), case, inp), case, "peaked", tag + " streamer")
    print(f"fused T={T}: {differing} of {compared} elements differ between the K-sliced streamer's q | k | v and the k-ordered chain's")
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("path,dtype,B,T,Hh,hd,family,p", R.SENSITIVITY)
def test_kernel_misses_each_wrong_reference(path, dtype, B, T, Hh, hd, family, p):
    """The kernel is inside the bound of the reference and outside it for every wrong reference that applies to the case."""
    rep = Report(f"sensitivity {path} {dtype} T={T} hd={hd}")
    inp = R.make_inputs(family, B, T, Hh, hd, dtype)
    got, case = check_fwd(rep, inp, p) if path == "fwd" else check_bwd(rep, inp, p)
    rep.close()
    for wrong in R.applicable_wrongs(path, dtype, T, hd, family, p, B, Hh):
        miss, where = R.worst(R.wrong_errors(path, wrong, inp, case, keep_of(inp, p), got))
        print(f"  {wrong}: missed by {miss:.2e} against the bound {case['rtol']:.2e} at {where}")
        assert miss > case["rtol"], f"a reference with {wrong} would pass"


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    """Shapes outside the contract are refused by the launchers before any launch: status -2, every output still NaN between intact canaries."""
    def fwd(dtype, T, hd, B=2, Hh=2):
        inp = R.make_inputs("soft", B, T, Hh, hd, dtype)
        rc, y = launch_fwd(inp)
        assert rc == UNSUPPORTED and y.intact() and bool(torch.isnan(y.t).all()), (dtype, T, hd, rc)

    def bwd(dtype, T, hd, B=2, Hh=2):
        inp = R.make_inputs("soft", B, T, Hh, hd, dtype)
        rc, *outs = launch_bwd(inp)
        assert rc == UNSUPPORTED and all(o.intact() and bool(torch.isnan(o.t).all()) for o in outs), (dtype, T, hd, rc)

    fwd(F32, 16, 344, B=1, Hh=1)            # 3 * 16 * 344 * 4 + 16 * 16 * 4 bytes of LDS: over 64 KiB
    for T in (8, 20):
        fwd(BF16, T, 24); fwd(BF16, T, 136)
        bwd(F32, T, 132); bwd(BF16, T, 12)
    for dtype in (BF16, F32):
        fwd(dtype, 65, 64); bwd(dtype, 65, 64)
