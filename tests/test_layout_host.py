"""Host-only check of csrc/rome_layout.h (the transposition every host-pointer entry point of the C API goes through)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_roundtrip_under_sanitizers(tmp_path):
    """tests/c/layout_check.cpp, a stand-alone host program (no HIP), built with ASan + UBSan and run as a child process:
    to_soa / from_soa round-trip exactly for C in {0, 1, 3}, N in {1, 2, 33}, d in {1, 2, 3, 6}; SoA input is a plain copy."""
    exe = str(tmp_path / "layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "c", "layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "layout_check ok" in out.stdout, out.stdout + out.stderr
