"""GPU: mode_lora_merge / mode_lora_grad (csrc/lora.hip) through ctypes, per element against the fp64 references and the DERIVED bounds of
tests/lora_refs.py: every shape, rank and group count there, bf16 and in-place fp32 merges, canaries around every output, accumulation,
bit-identity of two runs, linearity in dW, the deliberately wrong references outside the bound, and refused descriptors that launch nothing."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_refs as R  # noqa: E402
from hip_helpers import CANARY, Guarded, stream  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402

MERGE_CASES = [(G, rows, cols, r) for (rows, cols) in R.MERGE_SHAPES for r in R.RANKS for G in R.GROUPS]
GRAD_CASES = [(G, rows, cols, r) for (rows, cols) in R.GRAD_SHAPES for r in R.RANKS for G in R.GROUPS]
PAD = 64                                                                           # canary elements before and after a strided buffer


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


class Strided:
    """G matrices [rows, cols], rows * cols + STRIDE_PAD elements apart, inside a canary-filled buffer: the gaps between the matrices and PAD
    elements on either side must keep the canary."""

    def __init__(self, G, rows, cols, dtype, src=None):
        self.stride = rows * cols + R.STRIDE_PAD
        self.buf = torch.full((2 * PAD + G * self.stride,), CANARY, dtype=dtype, device="cuda")
        self.mats = self.buf[PAD: PAD + G * self.stride].view(G, self.stride)[:, : rows * cols]
        if src is None:
            self.mats.fill_(float("nan"))
        else:
            self.mats.copy_(src.reshape(G, -1))
        self.shape = (G, rows, cols)
        assert self.mats.data_ptr() % 16 == 0 and (cols % 8 != 0 or self.stride % 8 == 0)

    def value(self):
        return self.mats.float().cpu().view(self.shape)

    def intact(self):
        body = self.buf[PAD: PAD + self.shape[0] * self.stride].view(self.shape[0], self.stride)
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[-PAD:] == CANARY).all()) and bool((body[:, self.mats.shape[1]:] == CANARY).all())


def dev(d, *keys):
    return [d[k].cuda().contiguous() for k in keys]


def desc(G, rows, cols, r, stride, scale, **ptrs):
    return L.ModeLoraDesc(G=G, rows=rows, cols=cols, r=r, w_stride=stride, scale=scale.data_ptr(), **{k: (v if isinstance(v, int) else v.data_ptr()) for k, v in ptrs.items()})


def scale_dev(s=R.SCALE):
    return torch.tensor([s], dtype=torch.float32, device="cuda")


def run_grad(G, rows, cols, r, dW, A, B, s, dA, dB, accumulate=False, status=False):
    """mode_lora_grad on a Strided dW into Guarded dA [G r, cols] / dB [G rows, r]."""
    lib = L.load()
    d = desc(G, rows, cols, r, dW.stride, s, dW=dW.mats, A=A, B=B, dA=dA.t, dB=dB.t)
    d.accumulate = int(accumulate)
    need = lib.mode_lora_grad_workspace_bytes(C.byref(d))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    rc = lib.mode_lora_grad(C.byref(d), ws.data_ptr(), ws.numel(), stream())
    if status:
        return rc
    L.check(rc, "lora_grad")


@pytest.mark.parametrize("G,rows,cols,r", MERGE_CASES)
def test_merge_per_element_bf16_and_fp32_in_place(G, rows, cols, r):
    lib = L.load()
    d = R.inputs(G, rows, cols, r)
    A, B = dev(d, "A", "B")
    s = scale_dev()
    s32 = float(s.cpu()[0])                                                        # the reference uses the fp32 value the kernel reads
    ref, S = R.merge_ref(d["W"], d["A"], d["B"], s32)
    wrong = R.wrong_merges(d["W"], d["A"], d["B"], s32)
    for out_bf16 in (True, False):
        W = Strided(G, rows, cols, torch.float32, d["W"])
        out = Strided(G, rows, cols, torch.bfloat16) if out_bf16 else W           # fp32: in place over W
        w_before = bits(W.buf)
        dd = desc(G, rows, cols, r, W.stride, s, W=W.mats, A=A, B=B, out=out.mats)
        dd.out_dtype = L.MODE_BF16 if out_bf16 else L.MODE_F32
        L.check(lib.mode_lora_merge(C.byref(dd), stream()), "lora_merge")
        torch.cuda.synchronize()
        assert out.intact() and W.intact()
        if out_bf16:
            assert torch.equal(bits(W.buf), w_before)                              # the base is read, never written
        bound = R.merge_bound(ref, S, out_bf16)
        got = out.value()
        ratio = R.worst(got, ref, bound)
        print(f"merge G={G} {rows}x{cols} r={r} {'bf16' if out_bf16 else 'fp32 in place'}: worst error / bound {ratio:.3f}")
        assert torch.isfinite(got).all() and ratio <= 1.0, ratio
        for name, w in wrong.items():
            assert R.worst(got, w, bound) > 1.0, name                              # the kernel is told apart from each wrong reference


@pytest.mark.parametrize("G,rows,cols,r", GRAD_CASES)
def test_projection_per_element_accumulate_bit_identity_linearity(G, rows, cols, r):
    d = R.inputs(G, rows, cols, r)
    A, B = dev(d, "A", "B")
    s = scale_dev()
    s32 = float(s.cpu()[0])
    (rA, rB), (bA, bB) = R.grad_ref(d["dW"], d["A"], d["B"], s32)
    dW = Strided(G, rows, cols, torch.float32, d["dW"])
    dw_before = bits(dW.buf)
    runs = []
    for _ in range(2):
        dA, dB = Guarded(G * r, cols), Guarded(G * rows, r)
        run_grad(G, rows, cols, r, dW, A, B, s, dA, dB)
        torch.cuda.synchronize()
        assert dA.intact() and dB.intact() and torch.equal(bits(dW.buf), dw_before)
        runs.append((dA.t.cpu().view(G, r, cols), dB.t.cpu().view(G, rows, r)))
    (gA, gB), (gA2, gB2) = runs
    assert torch.equal(bits(gA), bits(gA2)) and torch.equal(bits(gB), bits(gB2))   # run to run: the same bits
    qa, qb = R.worst(gA, rA, bA), R.worst(gB, rB, bB)
    print(f"grad G={G} {rows}x{cols} r={r}: worst error / bound dA {qa:.3f} dB {qb:.3f}")
    assert torch.isfinite(gA).all() and torch.isfinite(gB).all() and qa <= 1.0 and qb <= 1.0, (qa, qb)
    for name, (wA, wB) in R.wrong_grads(d["dW"], d["A"], d["B"], s32).items():
        assert R.worst(gA, wA, bA) > 1.0 and R.worst(gB, wB, bB) > 1.0, name
    # accumulate: added to what the outputs hold
    (aA, aB), (baA, baB) = R.grad_ref(d["dW"], d["A"], d["B"], s32, d["dA0"], d["dB0"])
    dA, dB = Guarded(G * r, cols), Guarded(G * rows, r)
    dA.t.copy_(d["dA0"].view(G * r, cols)); dB.t.copy_(d["dB0"].view(G * rows, r))
    run_grad(G, rows, cols, r, dW, A, B, s, dA, dB, accumulate=True)
    torch.cuda.synchronize()
    assert dA.intact() and dB.intact()
    qa, qb = R.worst(dA.t.cpu().view(G, r, cols), aA, baA), R.worst(dB.t.cpu().view(G, rows, r), aB, baB)
    print(f"     accumulate: dA {qa:.3f} dB {qb:.3f}")
    assert qa <= 1.0 and qb <= 1.0, (qa, qb)
    # linearity: dW = h1 + h2 exactly (an element-wise split), so the exact projections add; the kernel's results must agree within the bound
    halves = []
    for h in (d["dW"] * d["mask"], d["dW"] * (1 - d["mask"])):
        hd = Strided(G, rows, cols, torch.float32, h)
        dA, dB = Guarded(G * r, cols), Guarded(G * rows, r)
        run_grad(G, rows, cols, r, hd, A, B, s, dA, dB)
        torch.cuda.synchronize()
        halves.append((dA.t.cpu().double().view(G, r, cols), dB.t.cpu().double().view(G, rows, r)))
    qa, qb = R.worst(gA, halves[0][0] + halves[1][0], bA), R.worst(gB, halves[0][1] + halves[1][1], bB)
    print(f"     sum of two halves: dA {qa:.3f} dB {qb:.3f}")
    assert qa <= 1.0 and qb <= 1.0, (qa, qb)


def test_scale_is_read_from_the_device_at_run_time():
    """The same descriptor after the scalar changed on the device follows the new value (what lets a captured merge outlive a change of alpha)."""
    lib = L.load()
    G, rows, cols, r = 1, 7, 64, 3
    d = R.inputs(G, rows, cols, r)
    A, B = dev(d, "A", "B")
    s = scale_dev(0.5)
    W, out = Strided(G, rows, cols, torch.float32, d["W"]), Strided(G, rows, cols, torch.bfloat16)
    dd = desc(G, rows, cols, r, W.stride, s, W=W.mats, A=A, B=B, out=out.mats)
    dd.out_dtype = L.MODE_BF16
    for val in (0.5, -2.25):
        s.fill_(val)
        L.check(lib.mode_lora_merge(C.byref(dd), stream()), "lora_merge")
        torch.cuda.synchronize()
        ref, S = R.merge_ref(d["W"], d["A"], d["B"], val)
        assert R.worst(out.value(), ref, R.merge_bound(ref, S, True)) <= 1.0 and out.intact()


@pytest.mark.parametrize("r,cols", [(0, 64), (65, 64), (16, 68)])
def test_bad_descriptors_return_an_error_and_touch_nothing(r, cols):
    lib = L.load()
    G, rows, ra = 1, 7, max(1, min(r, 64))
    s = scale_dev()
    W = Strided(G, rows, cols, torch.float32, torch.zeros(G, rows, cols))
    A, B = torch.zeros(G, ra, cols, device="cuda"), torch.zeros(G, rows, ra, device="cuda")
    for dt in (torch.bfloat16, torch.float32):
        out = Strided(G, rows, cols, dt, torch.full((G, rows, cols), CANARY))
        dd = desc(G, rows, cols, r, W.stride, s, W=W.mats, A=A, B=B, out=out.mats)
        dd.out_dtype = L.MODE_BF16 if dt == torch.bfloat16 else L.MODE_F32
        assert lib.mode_lora_merge(C.byref(dd), stream()) == -2
        torch.cuda.synchronize()
        assert bool((out.buf == CANARY).all())
    dA, dB = Guarded(G * ra, cols, fill=CANARY), Guarded(G * rows, ra, fill=CANARY)
    assert run_grad(G, rows, cols, r, W, A, B, s, dA, dB, status=True) == -2
    torch.cuda.synchronize()
    assert bool((dA.buf == CANARY).all()) and bool((dB.buf == CANARY).all())
    # a workspace that is too small is refused as well
    good = desc(G, rows, 64, 4, 7 * 64 + 64, s, dW=Strided(G, rows, 64, torch.float32, torch.zeros(G, rows, 64)).mats, A=torch.zeros(G, 4, 64, device="cuda"),
                B=torch.zeros(G, rows, 4, device="cuda"), dA=dA.t, dB=dB.t)
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    assert lib.mode_lora_grad(C.byref(good), ws.data_ptr(), 64, stream()) == -3
    torch.cuda.synchronize()
    assert bool((dA.buf == CANARY).all()) and bool((dB.buf == CANARY).all())
