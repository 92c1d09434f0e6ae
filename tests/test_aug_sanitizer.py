"""The augmentation's case list through the host twin under AddressSanitizer and UndefinedBehaviorSanitizer: tools/aug_host_check.cpp,
a stand-alone program around the host-only build of og_aug.inc, compiled and run here -- never loaded into Python.  Every buffer is a
heap block of exactly its declared size.  The sanitizer runtimes are linked statically into the program, as
tests/test_pnge_sanitizer.py does for the encoder.  The program's build of the twin (a host compiler's) must give the bits of the
library's (hipcc's host pass): the arithmetic is written without contraction.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aug_cases as AC
from openglottal_amd import augment as A
from test_mjpd_sanitizer import ROOT, _toolchain


def test_the_case_list_is_clean_under_asan_and_ubsan(tmp_path):
    cxx, flags, why = _toolchain(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with static sanitizer runtimes: " + "; ".join(why))
    exe = tmp_path / "aug_host_check"
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "aug_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]                               # (the probe built: this is an error in the sources)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aug_cases_corpus.py"), str(tmp_path / "cases.bin")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    m = re.match(r"(\d+) cases, (\d+) pixels, image bits sum (\d+)", r.stdout)
    cases = AC.corpus()
    assert m and int(m.group(1)) == len(cases) == sum(len(AC.case_list(S)) for S in AC.SIZES), r.stdout
    assert int(m.group(2)) == sum(S * S for S, *_ in cases)
    want = 0
    for S, rec, im, mk in cases:
        oi, _ = A.augment_host(im[None], mk[None], [0], [rec])
        want += int(oi.view(np.uint32).astype(np.uint64).sum())
    assert int(m.group(3)) == want                                            # the two builds of the twin agree bit for bit
