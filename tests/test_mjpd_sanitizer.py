"""The hostile corpus through the host twin under AddressSanitizer and UndefinedBehaviorSanitizer: tools/mjpd_host_fuzz.cpp, a
stand-alone program around the host-only build of og_mjpd.inc, compiled and run here -- never loaded into Python.  The sanitizer
runtimes are linked statically into the program, so nothing about the environment it inherits matters to them, and the environment
is passed on as it is.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# per compiler family, what links the runtimes statically (clang does by default)
STATIC = {"g++": ["-static-libasan", "-static-libubsan"], "clang++": ["-static-libsan"]}


def _toolchain(tmp):
    """`(compiler, flags)` of the first host compiler that builds AND runs an empty program with the sanitizers linked statically;
    otherwise the reasons, one per candidate.  Nothing of the project is compiled here: a skip can only mean a missing runtime."""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    why = []
    for name in dict.fromkeys([os.environ.get("CXX") or "c++", "g++", "clang++"]):
        cxx = shutil.which(name)
        if not cxx:
            why.append(f"{name}: not found")
            continue
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.lower()
        flags = FLAGS + STATIC["clang++" if "clang" in version else "g++"]
        exe = os.path.join(tmp, "probe")
        r = subprocess.run([cxx, *flags, probe, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            r = subprocess.run([exe], capture_output=True, text=True)
        if r.returncode == 0:
            return cxx, flags, why
        why.append(f"{name}: {(r.stderr.strip().splitlines() or ['failed'])[-1][:200]}")
    return None, None, why


def test_the_corpus_is_clean_under_asan_and_ubsan(tmp_path):
    cxx, flags, why = _toolchain(str(tmp_path))
    if cxx is None:
        pytest.skip("no host compiler with static sanitizer runtimes: " + "; ".join(why))
    exe = tmp_path / "mjpd_host_fuzz"
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "mjpd_host_fuzz.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]                               # (the probe built: this is an error in the sources)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mjpd_fuzz_corpus.py"), str(tmp_path / "corpus.bin")], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    m = re.match(r"(\d+) cases, (\d+) table sets, form 17x9 sampling 3 Ri 1; per status:(.*)", r.stdout)
    assert m and int(m.group(1)) == 2559 + 36, r.stdout
    seen = {int(k): int(v) for k, v in (p.split(":") for p in m.group(3).split())}
    assert sum(seen.values()) == int(m.group(1)) and seen[0] >= 36 and all(seen[s] > 0 for s in (1, 2, 3, 5, 6)) and seen[7] == 0
