"""The gfx950 assembly listing of the shipped device code, compiled once and shared by the tests/test_isa_*.py modules.

Helper module (like tests/buffer_guard.py).  ``listing()`` returns the path of
``hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only openglottal_amd/csrc/og_api.hip`` (about 100 s of compile
time, which every ISA test used to pay on its own).  The file lives in a directory of the system's temp dir named after the
SHA-256 of every file under openglottal_amd/csrc/ and of ``hipcc --version``: a changed source or compiler is another
directory, so a listing is never stale.  It is written under a private name and renamed into place, so a half-written listing
is never read.  ``lines()`` is the same listing as a list of lines, read once per process.  Read-only for its users: a test that
wants a mutant edits a copy of the text in memory.
"""
import functools
import hashlib
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openglottal_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only")


def available():
    return os.path.exists(HIPCC)


def source_hash():
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC)):
        p = os.path.join(CSRC, name)
        if os.path.isfile(p):
            h.update(name.encode() + b"\0")
            with open(p, "rb") as f:
                h.update(f.read())
            h.update(b"\0")
    h.update(" ".join(FLAGS).encode())
    h.update(subprocess.run([HIPCC, "--version"], check=True, capture_output=True).stdout)
    return h.hexdigest()[:24]


@functools.lru_cache(maxsize=None)
def listing():
    name = f"openglottal_isa_{os.getuid()}_{source_hash()}"
    d = os.path.join(tempfile.gettempdir(), name)
    try:
        os.makedirs(d, mode=0o700, exist_ok=True)
        if os.stat(d).st_uid != os.getuid() or not os.access(d, os.W_OK):
            raise PermissionError(d)
    except OSError:
        d = tempfile.mkdtemp(prefix=name + "_")
    asm = os.path.join(d, "og_api.s")
    if not os.path.exists(asm):
        fd, tmp = tempfile.mkstemp(dir=d, prefix="og_api.", suffix=".part")
        os.close(fd)
        subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, "og_api.hip"), "-o", tmp],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(tmp, asm)
    return asm


@functools.lru_cache(maxsize=None)
def lines():
    with open(listing()) as f:
        return tuple(f.read().split("\n"))
