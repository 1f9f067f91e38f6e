"""mode_frames_preprocess (csrc/frame_prep.hip) and camera.CameraTransform on the MI355X against the fp64 reference of tests/camera_refs.py,
element by element with nothing excluded: every output must be (L / 255 - mean) / std for a level L the unrounded reference admits
(|L - R| <= 0.5 + 2e-3), within 2e-6 (fp32) or one bf16 ulp + 2e-6 (bf16).  Shapes are the smallest that reach each path of the kernel: up- and
downscales, the identity, odd and 16-byte-aligned destination rows, more than one band, the band heights the LDS budget forces (8, 4, 2, 1),
row lists with repeats / out-of-range entries / none, a row pitch, shifts at the corners, both cameras or one."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402

import camera_refs as R  # noqa: E402
from hip_helpers import CANARY  # noqa: E402

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
MEAN2, STD2 = (0.1, 0.5, 0.9), (0.5, 1.0, 0.2)
DTYPES = [torch.float32, torch.bfloat16]


class GuardedOut:
    """A NaN-prefilled contiguous output of ``shape`` with canary regions before and after it (the pattern of hip_helpers.Guarded; ``skew`` elements
    move it off the 16-byte boundary)."""

    def __init__(self, shape, dtype, skew=0):
        n = 1
        for v in shape:
            n *= v
        self.pad = 64 + skew
        self.buf = torch.full((self.pad + n + 64,), CANARY, dtype=dtype, device="cuda")
        self.t = self.buf[self.pad: self.pad + n].view(shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[: self.pad] == CANARY).all()) and bool((self.buf[self.pad + self.t.numel():] == CANARY).all())


def frames(n, T, H, W, seed, pitch_extra=0, offset=0):
    """uint8 (n, T, H, W, 3) random frames as a view of a flat buffer: rows ``pitch_extra`` bytes further apart than they are long, the first one
    ``offset`` bytes into the allocation; frame (0, 0) all 0 and frame (n - 1, T - 1) all 255 (the clamp's ends)."""
    g = torch.Generator().manual_seed(seed)
    row = T * H * W * 3
    base = torch.randint(0, 256, (offset + n * (row + pitch_extra),), generator=g, dtype=torch.uint8).cuda()
    f = base[offset:].view(n, row + pitch_extra)[:, :row].view(n, T, H, W, 3)
    f[0, 0] = 0
    f[n - 1, T - 1] = 255
    return f


def launch(cams, rows, num_envs, m_b):
    """cams: up to two of None | dict(src, dst (GuardedOut), size, mean, std, shifts=None, pad=0).  Returns the status."""
    r = None if rows is None else torch.tensor(rows, dtype=torch.int32, device="cuda")
    d = L.ModeFramePrepDesc(rows=None if r is None else r.data_ptr(), m_b=m_b, num_envs=num_envs)
    keep = []
    for k, c in enumerate(cams):
        if c is None:
            continue
        f, dst = c["src"], c["dst"].t
        sh = c.get("shifts")
        if sh is not None:
            sh = torch.tensor(sh, dtype=torch.int32, device="cuda")
            keep.append(sh)
        cam = L.ModeFramePrepCam(src=f.data_ptr(), src_stride=f.stride(0), dst=dst.data_ptr(), shifts=None if sh is None else sh.data_ptr(),
                                 T=f.shape[1], H=f.shape[2], W=f.shape[3], OH=c["size"][0], OW=c["size"][1],
                                 dst_dtype=L.MODE_BF16 if dst.dtype == torch.bfloat16 else L.MODE_F32, pad=c.get("pad", 0))
        for i in range(3):
            cam.mean[i], cam.inv_std[i] = c["mean"][i], 1.0 / c["std"][i]
        d.cam[k] = cam
    rc = L.load().mode_frames_preprocess(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def expect(c, rows, num_envs, label):
    """Output row j of camera ``c`` against the reference of source row rows[j]; rows outside [0, num_envs) keep their NaN canary."""
    f, out = c["src"], c["dst"]
    T = f.shape[1]
    assert out.intact(), label
    got = out.t.view(len(rows), T, 3, *c["size"])
    for j, r in enumerate(rows):
        if not 0 <= r < num_envs:
            assert bool(torch.isnan(got[j]).all()), (label, j)
            continue
        sh = None if c.get("shifts") is None else c["shifts"][j * T:(j + 1) * T]
        Rv, _ = R.transform(f[r], c["size"], c["mean"], c["std"], sh, c.get("pad", 0))
        worst, ties = R.check_output(got[j], Rv, c["mean"], c["std"])
        print(f"{label} row {j} <- {r}: worst excess over tolerance {worst:.3e}, {ties} elements near a tie")
        assert worst <= 0, (label, j, r, worst)


def cam(f, size, dtype, m_b, mean=MEAN, std=STD, skew=0, **kw):
    return dict(src=f, dst=GuardedOut((m_b * f.shape[1], 3) + tuple(size), dtype, skew), size=tuple(size), mean=mean, std=std, **kw)


# (H, W) -> (OH, OW), T
GEOMETRIES = [((25, 25), (28, 28), 1),        # the 200 -> 224 ratio; four bands of 8 rows, the last one short
              ((9, 7), (16, 12), 1),          # upscale, two-tap edges
              ((37, 29), (16, 12), 1),        # antialiased downscale, 5 taps per axis
              ((21, 84), (28, 28), 1),        # up on one axis, down on the other
              ((16, 13), (16, 13), 1),        # identity: exact levels; odd OW, rows not 16-byte aligned
              ((20, 20), (24, 32), 2),        # OW a multiple of 8 (16-byte stores in both dtypes), two frames per row
              ((64, 120), (8, 16), 1),        # ratio 8 and 7.5: the widest filters (17 taps)
              ((12, 480), (12, 600), 1),      # bands of 4 rows (8 do not fit 64 KiB of LDS)
              ((12, 640), (12, 800), 1),      # bands of 2 rows
              ((5, 1400), (5, 1400), 1)]      # bands of 1 row


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("src,dst,T", GEOMETRIES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d, _ in GEOMETRIES])
def test_geometries_rows_null(src, dst, T, dtype):
    n = 2
    f = frames(n, T, *src, seed=src[0] * 1000 + src[1], offset=3)               # (a source that starts off the 16-byte boundary)
    c = cam(f, dst, dtype, n)
    assert launch([c], None, n, n) == 0
    expect(c, list(range(n)), n, f"{src}->{dst} {dtype}")
    if src == dst:                                                              # the identity's levels are the source's, exactly
        want = ((f.permute(0, 1, 4, 2, 3).double().cpu() / 255 - torch.tensor(MEAN, dtype=torch.float64).view(3, 1, 1))
                / torch.tensor(STD, dtype=torch.float64).view(3, 1, 1))
        tol = 2e-6 + (want.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
        assert bool(((c["dst"].t.view(n, T, 3, *dst).double().cpu() - want).abs() <= tol).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_unaligned_destination_takes_element_stores(dtype):
    f = frames(2, 1, 20, 20, seed=77)
    c = cam(f, (24, 32), dtype, 2, skew=1)                                      # OW a multiple of 8, but the tensor starts one element off
    assert c["dst"].t.data_ptr() % 16 != 0
    assert launch([c], None, 2, 2) == 0
    expect(c, [0, 1], 2, f"skewed {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_ratio_above_8_is_refused_and_nothing_is_written(dtype):
    f = frames(2, 1, 136, 16, seed=5)
    c = cam(f, (16, 16), dtype, 2)
    assert launch([c], None, 2, 2) == -2
    assert c["dst"].intact() and bool(torch.isnan(c["dst"].t).all())
    ok = cam(frames(2, 1, 9, 7, seed=6), (16, 12), dtype, 2)                    # one refused camera refuses the launch: the other stays untouched
    assert launch([ok, c], None, 2, 2) == -2
    assert ok["dst"].intact() and bool(torch.isnan(ok["dst"].t).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_cameras_one_launch_and_one_camera_null(dtype):
    n = 3
    a = cam(frames(n, 1, 25, 25, seed=11), (28, 28), dtype, n)
    b = cam(frames(n, 1, 37, 29, seed=12, offset=5), (16, 12), dtype, n, mean=MEAN2, std=STD2)
    assert launch([a, b], None, n, n) == 0
    expect(a, list(range(n)), n, "static")
    expect(b, list(range(n)), n, "gripper")
    both = b["dst"].t.clone()
    for slot in (0, 1):                                                         # alone, in either slot: the same bits
        solo = cam(b["src"], (16, 12), dtype, n, mean=MEAN2, std=STD2)
        assert launch([solo, None] if slot == 0 else [None, solo], None, n, n) == 0
        assert solo["dst"].intact() and torch.equal(solo["dst"].t.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                                     both.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [[2, 0, 0], [1, -1, 7]], ids=["repeat-padded", "out-of-range"])
def test_rows_gather_with_a_row_pitch(rows, dtype):
    num_envs = 3
    a = cam(frames(num_envs, 2, 25, 25, seed=21, pitch_extra=37, offset=1), (28, 28), dtype, len(rows))
    b = cam(frames(num_envs, 2, 9, 7, seed=22, pitch_extra=5), (16, 12), dtype, len(rows), mean=MEAN2, std=STD2)
    assert a["src"].stride(0) == 2 * 25 * 25 * 3 + 37
    listed = {r for r in rows if 0 <= r < num_envs}
    assert launch([a, b], rows, num_envs, len(rows)) == 0
    expect(a, rows, num_envs, f"rows {rows} static")
    expect(b, rows, num_envs, f"rows {rows} gripper")
    # nothing is read from the rows that are not listed: other contents there, the same output bits
    a2 = cam(a["src"].clone(), (28, 28), dtype, len(rows))
    for r in range(num_envs):
        if r not in listed:
            a2["src"][r] = 255 - a2["src"][r]
    assert launch([a2], rows, num_envs, len(rows)) == 0
    keep = [j for j, r in enumerate(rows) if r in listed]
    v = lambda c: c["dst"].t.view(len(rows), -1)[keep].view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(v(a), v(a2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_shifts(dtype):
    pad, n, T = 3, 3, 2
    f = frames(n, T, 25, 25, seed=31)
    shifts = [[0, 0], [6, 6], [0, 6], [3, 3], [6, 0], [2, 5]]                    # one (sx, sy) per output frame
    c = cam(f, (28, 28), dtype, n, shifts=shifts, pad=pad)
    g = cam(frames(n, T, 37, 29, seed=32), (16, 12), dtype, n, shifts=shifts[::-1], pad=pad, mean=MEAN2, std=STD2)
    assert launch([c, g], None, n, n) == 0
    expect(c, list(range(n)), n, "shifted static")
    expect(g, list(range(n)), n, "shifted gripper")
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    plain = cam(f, (28, 28), dtype, n)                                          # no shifts at all
    centre = cam(f, (28, 28), dtype, n, shifts=[[3, 3]] * (n * T), pad=pad)     # shift = pad: the unshifted output, bit for bit
    assert launch([plain], None, n, n) == 0 and launch([centre], None, n, n) == 0
    assert torch.equal(plain["dst"].t.view(bits), centre["dst"].t.view(bits))
    assert torch.equal(plain["dst"].t.view(n * T, -1)[3].view(bits), c["dst"].t.view(n * T, -1)[3].view(bits))
    # out-of-range shifts are clamped into [0, 2 pad] on the device and never index memory
    wild = cam(f, (28, 28), dtype, n, shifts=[[-5, 99], [2 ** 31 - 1, -2 ** 31], [7, -1], [3, 3], [100000, 3], [0, 6]], pad=pad)
    clamped = cam(f, (28, 28), dtype, n, shifts=[[0, 6], [6, 0], [6, 0], [3, 3], [6, 3], [0, 6]], pad=pad)
    assert launch([wild], None, n, n) == 0 and launch([clamped], None, n, n) == 0
    assert wild["dst"].intact() and torch.equal(wild["dst"].t.view(bits), clamped["dst"].t.view(bits))
    expect(wild, list(range(n)), n, "clamped shifts")
    # pad > 0 without a shift table is the unshifted transform
    nopad = cam(f, (28, 28), dtype, n, pad=pad)
    assert launch([nopad], None, n, n) == 0 and torch.equal(nopad["dst"].t.view(bits), plain["dst"].t.view(bits))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_python_interface(dtype):
    ts, tg = M.CameraTransform((28, 28), shift_pad=2), M.CameraTransform((16, 12), MEAN2, STD2)
    s, g = frames(3, 2, 25, 25, seed=41, pitch_extra=9), frames(3, 2, 37, 29, seed=42)
    sh = ts.draw_shifts(6, "cuda", torch.Generator(device="cuda").manual_seed(1))
    assert sh.dtype == torch.int32 and sh.shape == (6, 2) and 0 <= int(sh.min()) and int(sh.max()) <= 4
    a, b = M.preprocess_cameras(s, g, ts, tg, shifts=(sh, None), dtype=dtype)
    torch.cuda.synchronize()
    assert a.shape == (3, 2, 3, 28, 28) and b.shape == (3, 2, 3, 16, 12) and a.dtype == b.dtype == dtype
    Ra, _ = R.transform(s.reshape(6, 25, 25, 3), (28, 28), MEAN, STD, sh.cpu().tolist(), 2)
    Rb, _ = R.transform(g.reshape(6, 37, 29, 3), (16, 12), MEAN2, STD2)
    assert R.check_output(a.reshape(6, 3, 28, 28), Ra, MEAN, STD)[0] <= 0 and R.check_output(b.reshape(6, 3, 16, 12), Rb, MEAN2, STD2)[0] <= 0
    # one camera, (B, H, W, 3) frames, a given output: the same bits
    out = torch.empty(6, 3, 16, 12, dtype=dtype, device="cuda")
    assert tg(g.reshape(6, 37, 29, 3), out=out) is out
    assert torch.equal(out.view(3, 2, 3, 16, 12), b)
    assert M.preprocess_cameras(None, g, ts, tg, dtype=dtype)[0] is None
    with pytest.raises(ValueError, match="shifts"):
        ts(s, shifts=sh[:4])
    with pytest.raises(ValueError, match="out must be"):
        tg(g, out=torch.empty(3, 2, 3, 16, 13, dtype=dtype, device="cuda"))
    with pytest.raises(ValueError, match="more than 8"):
        M.CameraTransform(16)(frames(1, 1, 136, 16, seed=1))
