"""The host half of the AdamW step (csrc/adamw_coef.h: decay, step_size, inv_bc2_sqrt - shared by mode_adamw_step / _clipped / _lp and the weight-gradient
GEMM's fused epilogue) on the CPU: the header compiled into a stand-alone host program (tests/adamw_coef_main.cpp), plain and with
-fsanitize=address,undefined, and its printed bit patterns compared with the same expressions in numpy - float64 operations followed by one cast to
float32, the decay factor in float32 - for both optimizers' default hyper-parameters x steps 1, 2, 10, 1000, 100000.  Equal bits are required."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mode_diffusion_policy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "adamw_coef_main.cpp")
HYPER = [(1e-4, 0.9, 0.95, 0.05), (1e-3, 0.9, 0.999, 1e-2)]                             # lr, beta1, beta2, weight_decay
STEPS = [1, 2, 10, 1000, 100000]


def _cxx():
    for c in ("g++", "clang++", "c++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    pytest.skip("no host C++ compiler")


def _expected():
    f32, f64 = np.float32, np.float64
    lines = []
    for lr, b1, b2, wd in HYPER:
        lr, b1, b2, wd = f32(lr), f32(b1), f32(b2), f32(wd)                             # the C ABI passes floats
        for step in STEPS:
            bc1, bc2 = f64(1.0) - f64(b1) ** f64(step), f64(1.0) - f64(b2) ** f64(step)
            coef = (f32(1.0) - lr * wd, f32(f64(lr) / bc1), f32(f64(1.0) / np.sqrt(bc2)))
            assert all(c.dtype == np.float32 for c in coef)
            lines.append(f"{step} " + " ".join(f"{int(c.view(np.uint32)):08x}" for c in coef))
    return lines


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", f"-I{CSRC}", *extra, SRC, "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split("\n")[:-1] == _expected()


def test_coefficients_equal_the_float64_expressions_bit_for_bit(tmp_path):
    assert len(_expected()) == 10
    _build_and_run(tmp_path, "coef", [])


def test_coefficients_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone host program, never code loaded into Python."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run([_cxx(), *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True)
    if ok.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    _build_and_run(tmp_path, "coef_san", flags)


def test_every_adamw_launch_site_takes_its_coefficients_from_the_one_function():
    """The streaming launcher (train_ops.hip) and the fused epilogue's launcher (gemm_bf16_tr.hip) call adamw_coef; neither derives a bias correction."""
    for name in ("train_ops.hip", "gemm_bf16_tr.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert src.count("adamw_coef(") == 1 and "bc1" not in src and "bc2" not in src.replace("inv_bc2_sqrt", ""), name
