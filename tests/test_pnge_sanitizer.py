"""The encoder's case list through the host twin under AddressSanitizer and UndefinedBehaviorSanitizer: tools/pnge_host_check.cpp, a
stand-alone program around the host-only build of og_pnge.inc, compiled and run here -- never loaded into Python.  Every buffer is a
heap block of exactly its declared size.  The sanitizer runtimes are linked statically into the program, as tests/test_png_sanitizer.py
does for the decoder's corpus.  No GPU."""
import os
import re
import subprocess
import sys

import pytest

import pnge_cases as EC
from test_mjpd_sanitizer import ROOT, _toolchain


def test_the_case_list_is_clean_under_asan_and_ubsan(tmp_path):
    cxx, flags, why = _toolchain(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with static sanitizer runtimes: " + "; ".join(why))
    exe = tmp_path / "pnge_host_check"
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "pnge_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]                               # (the probe built: this is an error in the sources)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pnge_cases_corpus.py"), str(tmp_path / "cases.bin")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    m = re.match(r"(\d+) cases, (\d+) raw bytes, (\d+) file bytes, (\d+) files at their bound", r.stdout)
    cases = EC.cases()
    assert m and int(m.group(1)) == len(cases), r.stdout
    assert int(m.group(2)) == sum(f.shape[0] * (1 + f.shape[1] * f.shape[2]) for _, f, _ in cases)
    assert int(m.group(3)) < int(m.group(2)) and int(m.group(4)) >= 6        # the noise frames are stored whole: exactly the bound
