"""og_zlayout (the host's grid.z layout) and og_zdecode (the kernels' inverse of it) are inverses, on the host, under sanitizers.

Eight conv kernels decode blockIdx.z with og_zdecode, whose quotient is a float multiply by 1 / gz instead of an integer division.
tools/zdecode_check.hip is a stand-alone program (its own main, only og_kernels.hpp included) that checks, exhaustively,
  * the quotient against bz / gz for every gz in 1..65535 and every bz < 65535 (every grid.z the hardware takes),
  * for every layout of the launchers' parameter grid with gz <= 65535: og_zlayout equals the launch layer's rule restated in plain
    integer code, every (frame, column tile x K part) is hit exactly once, and b >= frames only in the last frame group.
It is built for the host with -fsanitize=address,undefined and run as its own process: never through Python's loader, never on a GPU.
"""
import os
import subprocess

import pytest

import isa_listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not isa_listing.available(), reason="hipcc not available")
def test_zdecode_inverts_zlayout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "zdecode_check")
    build = subprocess.run([isa_listing.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "zdecode_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    last = run.stdout.strip().split("\n")[-1]
    assert last.startswith("zdecode_check: 4294836225 quotients, ") and last.endswith(", 0 failures"), last
