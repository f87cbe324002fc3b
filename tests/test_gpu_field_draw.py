"""box_muller_field of rome.jl_amd/csrc/rome_device_math.hpp -- the Box-Muller pair of the Pose2 draw, specialised to its 21-bit fields --
against the general box_muller on the words the draw is defined by, bit for bit, for every one of the 2^21 fields as radius field and as
angle field; and its radius root sqrt32_field against the shipped sqrt32_rn_normal at the radius argument of every field.
tests/hip/field_draw_check.hip, compiled on the fly with hipcc and run as one child process (one launch of 2^21 threads)."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = 1 << 21


def test_box_muller_field_returns_the_bits_of_box_muller_on_every_field(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "field_draw_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-o", exe,
                           os.path.join(ROOT, "tests", "hip", "field_draw_check.hip")])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=150)
    assert out.returncode == 0 and "field_draw_check done" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    got = {ln.split()[1]: [int(v) for v in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith("field ")}
    for what in ("radius", "angle", "pairc", "root"):
        fields, bad = got[what]
        assert fields == NF, "every 21-bit field"
        assert bad == 0, "%s: %d of %d fields differ in some bit" % (what, bad, fields)
    assert got["bare"][0] > 0, "the root comparison can fail: the uncorrected h * rsq(h) is not the rounded root everywhere"
