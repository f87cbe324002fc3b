"""sqrt32_rn_normal of rome.jl_amd/csrc/rome_device_math.hpp -- the radius root of box_muller without the guards of the general
expansion -- against the compiler's correctly rounded __builtin_sqrtf, bit for bit: every float of the documented range
[2^-96, FLT_MAX] and the radius argument of every one of the 2^32 radius words.  tests/hip/sqrt32_check.hip, compiled on the fly with
hipcc and run as one child process (4e9 + 4e9 roots: well under a second of device time)."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sqrt32_rn_normal_returns_the_bits_of_the_correctly_rounded_root(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "sqrt32_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-o", exe,
                           os.path.join(ROOT, "tests", "hip", "sqrt32_check.hip")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "sqrt32_check done" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    got = {ln.split()[1]: [int(v) for v in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith("sqrt32 ")}
    compared, bad = got["range"]
    assert compared == 0x7F7FFFFF - 0x0F800000 + 1, "every float from 2^-96 to FLT_MAX"
    assert bad == 0, "%d of %d floats differ from __builtin_sqrtf" % (bad, compared)
    taken, bad, below = got["radius"]
    # h <= 0 (no root taken) only at the top of the range: the polynomial's error is <= 2.7e-7 (box_muller's header), so -ln u1 must be
    # below that, u1 = x / 2^32 > 1 - 2.7e-7, i.e. x within 2^32 * 2.7e-7 = 1160 of 2^32; x = float(wa) + 1 moves wa by at most 128 + 256
    # (two roundings at a spacing of 256): at most 1544 words
    assert 2 ** 32 - 1544 <= taken <= 2 ** 32, taken
    assert below == 0, "%d radius arguments are positive and below 2^-96" % below
    assert bad == 0, "%d of %d radius arguments: the root differs from __builtin_sqrtf" % (bad, taken)
