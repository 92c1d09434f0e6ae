"""Guard zones around caller-owned buffers: where does an entry point write, and which bytes does its result depend on?

Helper module (like tests/f16_emulation.py) of tests/test_buffer_guard.py (numpy only) and tests/test_gpu_buffer_extents.py.

Every caller-owned OUTPUT lives in one larger allocation ``[guard | payload | guard]``: the payload starts at a multiple of 256
bytes, each guard is ``max(64 KiB, payload bytes)``, everything is pre-filled with 0xA5.  Every caller-owned INPUT lives in
``[slack | payload | slack]`` the same way.  ``run_guarded`` calls the entry three times:

* once on plain buffers of exactly the declared sizes (outputs pre-filled with 0x5A), as the Python wrappers allocate them;
* twice on guarded buffers, the slack around every input filled with 0x00 and then with 0xFF.

and reports a ``BufferFault`` unless
(a) both guards of every output are still 0xA5,
(b) every payload equals the plain run's bit for bit -- a byte the entry leaves unwritten is 0xA5 in one and 0x5A in the other,
    so this also proves that every declared byte was written,
(c) the two guarded runs agree bit for bit: no result depends on a byte outside a declared extent,
(d) every input allocation, slack included, is unchanged: no entry writes its inputs.
An optional output passed as NULL is simply a case of its own: its siblings must still come out as in every other case.

Device buffers are torch uint8 tensors, host buffers numpy arrays, pinned host buffers torch ``pin_memory`` tensors; the entry
sees raw addresses only.
"""
from __future__ import annotations

import collections

import numpy as np

GUARD_FILL = 0xA5
PLAIN_FILL = 0x5A
GUARD_MIN = 64 << 10
ALIGN = 256

CASES = collections.Counter()   # entry -> guarded cases run (the GPU module prints it)


class Fault:
    """One finding.  ``kind``: 'guard-before' | 'guard-after' (first / last: byte offsets from the payload's start / end, so
    before-guard offsets are negative), 'unwritten' | 'differs-from-plain' | 'slack-dependent' (offsets into the payload),
    'input-modified' (offsets from the input payload's start; negative = in the slack before it)."""

    def __init__(self, kind, buffer, first, last, count):
        self.kind, self.buffer, self.first, self.last, self.count = kind, buffer, int(first), int(last), int(count)

    def key(self):
        return (self.kind, self.buffer, self.first, self.last, self.count)

    def __repr__(self):
        return f"{self.buffer}: {self.kind}, {self.count} byte(s), first at {self.first:+d}, last at {self.last:+d}"


class BufferFault(AssertionError):
    def __init__(self, entry, label, faults):
        self.entry, self.label, self.faults = entry, label, list(faults)
        super().__init__(f"{entry} [{label}]: " + "; ".join(repr(f) for f in self.faults))


def _as_bytes(a) -> np.ndarray:
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Region:
    """``[pad | payload | pad]`` in host ('host'), pinned host ('pinned') or device ('device') memory.  Comparisons of device
    regions run on the device; bytes come back to the host only where something differs."""

    def __init__(self, name: str, nbytes: int, kind: str, pad: int, fill: int):
        self.name, self.nbytes, self.kind, self.pad = name, int(nbytes), kind, int(pad)
        total = 2 * self.pad + self.nbytes + ALIGN
        if kind == "host":
            self._raw = np.full(total, fill, np.uint8)
            base = self._raw.ctypes.data
        else:
            import torch

            if kind == "device":
                self._raw = torch.full((total,), fill, dtype=torch.uint8, device="cuda:0")
            else:
                self._raw = torch.full((total,), fill, dtype=torch.uint8).pin_memory()
            base = self._raw.data_ptr()
        self.lo = (-(base + self.pad)) % ALIGN + self.pad if self.pad else 0   # payload offset inside the allocation
        self.ptr = base + self.lo
        assert self.pad == 0 or self.ptr % ALIGN == 0
        self.hi = self.lo + self.nbytes

    def set_payload(self, data) -> None:
        data = _as_bytes(data)
        assert data.size == self.nbytes, (self.name, data.size, self.nbytes)
        if self.kind == "host":
            self._raw[self.lo:self.hi] = data
        else:
            import torch

            self._raw[self.lo:self.hi].copy_(torch.from_numpy(data.copy()))

    def state(self):
        return self._raw.copy() if self.kind == "host" else self._raw.clone()

    def _where(self, cond) -> np.ndarray:
        if self.kind == "host":
            return np.flatnonzero(cond)
        if not bool(cond.any()):
            return np.zeros(0, np.int64)
        return cond.nonzero().flatten().cpu().numpy()

    def changed(self, state) -> np.ndarray:
        """Offsets (inside the allocation) of the bytes that differ from an earlier ``state()``."""
        return self._where(self._raw != state)

    def dirty(self, lo: int, hi: int) -> np.ndarray:
        """Offsets, relative to ``lo``, of the bytes of [lo, hi) that are no longer the guard fill."""
        return self._where(self._raw[lo:hi] != GUARD_FILL)

    def payload(self) -> np.ndarray:
        v = self._raw[self.lo:self.hi]
        return v.copy() if self.kind == "host" else v.cpu().numpy().copy()

    def snapshot(self) -> np.ndarray:
        return self._raw.copy() if self.kind == "host" else self._raw.cpu().numpy().copy()


def guard_bytes(nbytes: int) -> int:
    return max(GUARD_MIN, int(nbytes))


def _span(kind, name, idx, origin):
    return Fault(kind, name, idx[0] - origin, idx[-1] - origin, idx.size)


def _diff(kind, name, a, b):
    idx = np.flatnonzero(a != b)
    return [_span(kind, name, idx, 0)] if idx.size else []


def guarded_call(call, inputs, outputs, kind="host", sync=None, slack=0x00, input_kinds=None, guarded=True):
    """ONE run.  ``inputs``: name -> array, ``fill -> array`` (an input with slack INSIDE it, e.g. gaps between packed frames) or
    None (NULL); ``outputs``: name -> payload bytes or None (NULL).  ``call(p)`` gets name -> address (or None) and returns the
    entry's code; ``sync()`` waits for the handle.  Returns ``(rc, payloads, faults)``; nothing here raises on a dirty guard."""
    input_kinds = input_kinds or {}
    regs_in, regs_out, before, p = {}, {}, {}, {}
    for name, a in inputs.items():
        if a is None:
            p[name] = None
            continue
        data = _as_bytes(a(slack) if callable(a) else a)
        r = Region(name, data.size, input_kinds.get(name, kind), guard_bytes(data.size) if guarded else 0, slack)
        r.set_payload(data)
        regs_in[name], p[name] = r, r.ptr
        before[name] = r.state()
    for name, n in outputs.items():
        if n is None:
            p[name] = None
            continue
        r = Region(name, n, kind, guard_bytes(n) if guarded else 0, GUARD_FILL if guarded else PLAIN_FILL)
        regs_out[name], p[name] = r, r.ptr
    if kind == "device" or "device" in input_kinds.values():
        import torch

        torch.cuda.synchronize()
    rc = call(p)
    if sync is not None:
        sync()
    faults, payloads = [], {}
    for name, r in regs_out.items():
        payloads[name] = r.payload()
        if guarded:
            idx = r.dirty(0, r.lo)
            if idx.size:
                faults.append(_span("guard-before", name, idx, r.lo))
            idx = r.dirty(r.hi, len(r._raw))
            if idx.size:
                faults.append(_span("guard-after", name, idx, 0))
    for name, r in regs_in.items():
        idx = r.changed(before[name])
        if idx.size:
            faults.append(_span("input-modified", name, idx, r.lo))
    return rc, payloads, faults


def run_guarded(entry, label, call, inputs, outputs, kind="host", sync=None, input_kinds=None, expect_rc=0):
    """The three runs described at the top.  Returns name -> payload (uint8) of the outputs; raises ``BufferFault``."""
    CASES[entry] += 1
    rc0, plain, _ = guarded_call(call, inputs, outputs, kind, sync, 0x00, input_kinds, guarded=False)
    assert rc0 == expect_rc, (entry, label, "plain buffers", rc0)
    runs, faults = [], []
    for slack in (0x00, 0xFF):
        rc, pay, f = guarded_call(call, inputs, outputs, kind, sync, slack, input_kinds)
        assert rc == expect_rc, (entry, label, f"slack {slack:#04x}", rc)
        runs.append(pay)
        for x in f:
            if x.key() not in [y.key() for y in faults]:
                faults.append(x)
    for name in runs[0]:
        a, b, pl = runs[0][name], runs[1][name], plain[name]
        faults += _diff("slack-dependent", name, a, b)
        idx = np.flatnonzero((a == GUARD_FILL) & (pl == PLAIN_FILL))
        if idx.size:
            faults.append(_span("unwritten", name, idx, 0))
        rest = (a != pl) & ~((a == GUARD_FILL) & (pl == PLAIN_FILL))
        if rest.any():
            faults.append(_span("differs-from-plain", name, np.flatnonzero(rest), 0))
    if faults:
        raise BufferFault(entry, label, faults)
    return runs[0]


def view(addr: int, nbytes: int) -> np.ndarray:
    """Host memory at a raw address as a uint8 array (for fake entries written in numpy)."""
    import ctypes as C

    return np.ctypeslib.as_array((C.c_ubyte * nbytes).from_address(addr))


def report() -> str:
    return "\n".join(f"buffer extents: {e}: {n} cases" for e, n in sorted(CASES.items()))
