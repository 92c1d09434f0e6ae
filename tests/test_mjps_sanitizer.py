"""The split twin under AddressSanitizer and UndefinedBehaviorSanitizer: tools/mjps_host_fuzz.cpp, a stand-alone program around the
host-only build of og_mjpd.inc and og_mjps.inc, compiled and run here as tests/test_mjpd_sanitizer.py runs its own -- never loaded into
Python, the runtimes linked statically.  Every file of the hostile corpora and every hand-made scan goes through the split twin at
(sub, lanes) = (4, 2) and (4, 256) in a heap block of exactly its size and has to give the sequential twin's status and bytes.  No GPU."""
import os
import re
import subprocess
import sys

import pytest

import mjps_cases as SC
from test_mjpd_sanitizer import ROOT, _toolchain


def test_the_corpus_is_clean_under_asan_and_ubsan(tmp_path):
    cxx, flags, why = _toolchain(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with static sanitizer runtimes: " + "; ".join(why))
    exe = tmp_path / "mjps_host_fuzz"
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "mjps_host_fuzz.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]                               # (the probe built: this is an error in the sources)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mjps_fuzz_corpus.py"), str(tmp_path / "corpus.bin")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    m = re.match(r"(\d+) cases; lanes (\d+) windows (\d+) most rounds (\d+) decodes (\d+); per status:(.*)", r.stdout)
    assert m and int(m.group(1)) == len(SC.hostile()) + 20 + 12, r.stdout
    seen = {int(k): int(v) for k, v in (p.split(":") for p in m.group(6).split())}
    assert sum(seen.values()) == int(m.group(1)) and seen[0] >= 12 and all(seen[s] > 0 for s in (1, 2, 3, 4, 5, 6)) and seen[7] == 0
    assert int(m.group(3)) > int(m.group(1)) and 2 <= int(m.group(4)) <= 256 and int(m.group(5)) >= int(m.group(2))
