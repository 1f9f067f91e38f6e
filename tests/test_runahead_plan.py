"""The weight run-ahead's touch plan (csrc/runahead.h) on the CPU: the header's mapping function compiled into a stand-alone host program
(tests/runahead_plan_main.cpp) and run - range sizes 0, 4, 127, 128, 129, 8191, 8193, 2 MiB, 6 MiB x 1 / 7 / 256 issuing workgroups x 1 / 4 / 16 slots:
every offset inside the range, no line twice, full coverage whenever slots x 64 x workgroups >= lines (a prefix otherwise).  The same program built
with -fsanitize=address,undefined reads every planned dword from a heap buffer of exactly the range's size.  Plus the binding side: the descriptor's
touch fields default to "no touch", the option exists, the ABI number did not move."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from mode_diffusion_policy_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mode_diffusion_policy_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "runahead_plan_main.cpp")


def _cxx():
    for c in ("g++", "clang++", "c++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    pytest.skip("no host C++ compiler")


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", f"-I{CSRC}", *extra, SRC, "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runahead plan OK: 81 cases" in r.stdout


def test_touch_plan_every_size_workgroup_and_slot_count(tmp_path):
    _build_and_run(tmp_path, "plan", [])


def test_touch_plan_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone host program, never code loaded into Python: every planned dword is read from a malloc of exactly the range's size."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run([_cxx(), *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True)
    if ok.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    _build_and_run(tmp_path, "plan_san", flags)


def test_header_is_plain_host_cxx_and_device_code_is_guarded():
    """runahead.h compiles without HIP (the program above) because its device half sits behind __HIPCC__; the mapping is declared for both sides."""
    src = open(os.path.join(CSRC, "runahead.h")).read()
    assert "#if defined(__HIPCC__)" in src and "__host__ __device__" in src
    assert re.search(r"MODE_RA_HD long ra_offset\(long bytes, int nwg, int slots, int wg, int slot, int lane\)", src)
    dev = src[src.rindex("#if defined(__HIPCC__)"):]
    assert "global_load_lds" in dev and "ra_slot_first_line" in dev       # the device half issues the load from the same line arithmetic


def test_descriptor_fields_default_to_no_touch_and_option_exists():
    d = L.ModeGemmDesc(dtype=L.MODE_BF16, M=1, N=4, K=64)
    assert d.touch0 is None and d.touch0_bytes == 0 and d.touch1 is None and d.touch1_bytes == 0
    names = [f[0] for f in L.ModeGemmDesc._fields_]
    assert names[-4:] == ["touch0", "touch0_bytes", "touch1", "touch1_bytes"]          # appended: every older field keeps its offset
    hdr = open(os.path.join(ROOT, "include", "mode_hip.h")).read()
    body = re.search(r"typedef struct ModeGemmDesc \{(.*?)\} ModeGemmDesc;", hdr, re.S).group(1)
    assert re.search(r"const void\* touch0; int64_t touch0_bytes;\s*const void\* touch1; int64_t touch1_bytes;\s*$", body)
    assert '"weight_runahead"' in hdr
    lib = L.load()
    assert lib.mode_hip_sizeof(b"ModeGemmDesc") == C.sizeof(L.ModeGemmDesc)
    assert lib.mode_hip_version() == L.ABI_VERSION == 13                            # an addition, not a new ABI
    for v in (0, 1):
        assert lib.mode_set_option(b"weight_runahead", v) == 0
