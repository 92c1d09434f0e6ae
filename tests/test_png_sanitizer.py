"""The hostile corpus and the valid set through the host twin under AddressSanitizer and UndefinedBehaviorSanitizer:
tools/png_host_fuzz.cpp, a stand-alone program around the host-only build of og_png.inc, compiled and run here -- never loaded into
Python.  The sanitizer runtimes are linked statically into the program, as tests/test_mjpd_sanitizer.py does for its corpus.  No GPU."""
import os
import re
import subprocess
import sys

import pytest

import png_cases as PC
from test_mjpd_sanitizer import ROOT, _toolchain


def test_the_corpus_is_clean_under_asan_and_ubsan(tmp_path):
    cxx, flags, why = _toolchain(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with static sanitizer runtimes: " + "; ".join(why))
    exe = tmp_path / "png_host_fuzz"
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "png_host_fuzz.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]                               # (the probe built: this is an error in the sources)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "png_fuzz_corpus.py"), str(tmp_path / "corpus.bin")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    m = re.match(r"(\d+) cases, (\d+) palettes, (\d+) pixel bytes; per status:(.*)", r.stdout)
    n_valid = len(PC.valid_cases())
    assert m and int(m.group(1)) == len(PC.hostile_corpus()) + n_valid and int(m.group(2)) >= 2, r.stdout
    seen = {int(k): int(v) for k, v in (p.split(":") for p in m.group(4).split())}
    assert sum(seen.values()) == int(m.group(1)) and seen[0] >= n_valid and all(seen[s] > 0 for s in range(1, 8))
