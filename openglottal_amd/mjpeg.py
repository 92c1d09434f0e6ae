"""Motion-JPEG output (include/openglottal_hip_mjpeg.h): `scripts/infer.py:274-275` writes ``<stem>_out.avi`` through OpenCV's ``MJPG``
writer; here the annotated frames are coded as baseline JPEG files ON THE DEVICE and only the compressed bytes come back.

``Mjpeg`` wraps one ``og_mjpeg`` handle (its stream and the workspace of one micro-batch) and the host twins that run the same
inline functions on the CPU.  ``AviWriter`` puts the files into a plain RIFF ``AVI `` container (one ``MJPG`` video stream, ``idx1``,
no OpenDML: below 2 GiB), ``read_avi_mjpeg`` walks such a file and decodes its frames with Pillow.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from ._lib import OpenGlottalHipError, check, lib, ptr

RIFF_LIMIT = 2 ** 31 - 1   # bytes a file without OpenDML may reach
RESIDENT_CAP = 1 << 30     # device bytes `Mjpeg.encode_resident` spends on the worst-case output of one call


def limit(which: int) -> int:
    return int(lib().og_mjpeg_limit(which))


def bound(H: int, W: int) -> int:
    """Worst-case bytes of one frame's JPEG file."""
    b = lib().og_jpeg_bound(int(H), int(W))
    if b < 0:
        check(-1, "og_jpeg_bound")
    return int(b)


def _bgr(frames, ndim: int) -> np.ndarray:
    a = np.ascontiguousarray(frames, dtype=np.uint8)
    if a.ndim != ndim or a.shape[-1] != 3:
        raise OpenGlottalHipError(f"expected u8 BGR frames {'[B,H,W,3]' if ndim == 4 else '[H,W,3]'}, got {a.shape}")
    return a


def tables(quality: int = 75, H: int = 8, W: int = 8):
    """``(qlum [64] u8, qchroma [64] u8, header bytes)``: the quantisation tables in natural order and SOI through SOS of an H x W frame."""
    ql, qc = np.empty(64, np.uint8), np.empty(64, np.uint8)
    hdr = np.empty(limit(6), np.uint8)
    n = C.c_int()
    check(lib().og_jpeg_tables_host(int(quality), int(H), int(W), ptr(ql), ptr(qc), ptr(hdr), hdr.size, C.addressof(n)), "og_jpeg_tables_host")
    return ql, qc, hdr[:n.value].tobytes()


def coefficients_host(frame, quality: int = 75) -> np.ndarray:
    """Quantised coefficients ``[M,3,64]`` int16 of one BGR frame: MCUs in scan order, Y Cb Cr, zigzag order."""
    f = _bgr(frame, 3)
    H, W = f.shape[:2]
    out = np.empty((((H + 7) // 8) * ((W + 7) // 8), 3, 64), np.int16)
    check(lib().og_jpeg_coefficients_host(ptr(f), H, W, int(quality), ptr(out)), "og_jpeg_coefficients_host")
    return out


def encode_host(frame, quality: int = 75) -> bytes:
    """One BGR frame as a complete JPEG file, on the CPU: the bytes the device produces."""
    f = _bgr(frame, 3)
    H, W = f.shape[:2]
    out = np.empty(bound(H, W), np.uint8)
    n = C.c_int()
    check(lib().og_jpeg_encode_host(ptr(f), H, W, int(quality), ptr(out), out.size, C.addressof(n)), "og_jpeg_encode_host")
    return out[:n.value].tobytes()


def split(blob, sizes) -> list[bytes]:
    """The files of ``encode``'s result, one ``bytes`` per frame."""
    b = np.asarray(blob, np.uint8)
    ends = np.cumsum(np.asarray(sizes, np.int64))
    return [b[e - s:e].tobytes() for s, e in zip(np.asarray(sizes, np.int64), ends)]


class Mjpeg:
    """One ``og_mjpeg`` handle.  The device is the current one at the first call that touches it."""

    def __init__(self, quality: int = 75, chunk: int = 128):
        self._h = lib().og_mjpeg_create()
        if not self._h:
            raise OpenGlottalHipError("og_mjpeg_create failed")
        self.set_quality(quality)
        self.set_chunk(chunk)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_mjpeg_destroy(h)
            except Exception:
                pass

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_mjpeg_set_chunk(self._h, int(chunk)), "og_mjpeg_set_chunk")
        self.chunk = int(chunk)

    def set_quality(self, quality: int) -> None:
        check(lib().og_mjpeg_set_quality(self._h, int(quality)), "og_mjpeg_set_quality")
        self.quality = int(quality)

    def sync(self) -> None:
        check(lib().og_mjpeg_sync(self._h), "og_mjpeg_sync")

    def encode(self, frames):
        """Host in, host out: ``[B,H,W,3]`` u8 BGR -> ``(blob u8, sizes int32 [B])``; the files lie back to back in ``blob``."""
        a = _bgr(frames, 4)
        B, H, W = a.shape[:3]
        out = np.empty(B * bound(H, W) if B else 0, np.uint8)
        sizes = np.empty(B, np.int32)
        total = C.c_longlong()
        check(lib().og_mjpeg_encode_stream_u8(self._h, ptr(a), B, H, W, ptr(out), out.size, ptr(sizes), C.addressof(total)),
              "og_mjpeg_encode_stream_u8")
        return out[:total.value].copy(), sizes

    def encode_dev(self, frames_dev, B: int, H: int, W: int, out_dev, cap: int, sizes_dev, total_dev) -> None:
        """Resident, asynchronous variant (torch CUDA tensors or raw ints): ``out_dev`` of ``cap >= B * bound(H, W)`` bytes,
        ``sizes_dev`` ``[B]`` int32, ``total_dev`` one int64."""
        check(lib().og_mjpeg_encode_u8_dev(self._h, ptr(frames_dev), B, H, W, ptr(out_dev), int(cap), ptr(sizes_dev), ptr(total_dev)),
              "og_mjpeg_encode_u8_dev")

    def encode_resident(self, frames_dev):
        """``[B,H,W,3]`` u8 CUDA tensor -> ``(blob u8, sizes int32)`` on the host; only the bytes produced cross.  The worst-case
        buffer ``encode_dev`` asks for is kept to ``RESIDENT_CAP`` bytes by coding the frames in as many calls as that takes."""
        import torch

        B, H, W = (int(v) for v in frames_dev.shape[:3])
        if B == 0:
            return np.zeros(0, np.uint8), np.zeros(0, np.int32)
        dev = frames_dev.device
        step = max(1, min(B, RESIDENT_CAP // bound(H, W)))
        cap = step * bound(H, W)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        sizes = torch.empty(B, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)   # (the handle runs on a stream of its own)
        blobs = []
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            self.encode_dev(frames_dev[b0:b0 + nb], nb, H, W, out, cap, sizes[b0:b0 + nb], total)
            self.sync()
            blobs.append(out[:int(total.item())].cpu().numpy())
        return (blobs[0] if len(blobs) == 1 else np.concatenate(blobs)), sizes.cpu().numpy()

    # the host twins, at this handle's quality
    def encode_host(self, frame) -> bytes:
        return encode_host(frame, self.quality)

    def coefficients_host(self, frame) -> np.ndarray:
        return coefficients_host(frame, self.quality)

    def tables(self, H: int = 8, W: int = 8):
        return tables(self.quality, H, W)

    def plan(self, B: int, H: int, W: int):
        return plan(B, H, W, self.chunk)


def plan(B: int, H: int, W: int, chunk: int = 128):
    """Dry run of the streamed pass: ``(records, workspace_bytes)``; a record is a dict of the plan line's fields."""
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = lib().og_mjpeg_plan(B, H, W, chunk, out, len(out), C.byref(ws))
    if n < 0:
        check(n, "og_mjpeg_plan")
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = []
    for line in out.value.decode().splitlines():
        parts = line.split("|")
        recs.append({k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, parts)})
    assert len(recs) == n
    return recs, ws.value


# ── the container ────────────────────────────────────────────────────────────────────────────────────────────────────
class AviWriter:
    """A plain RIFF ``AVI `` file with one ``MJPG`` video stream: ``hdrl`` (``avih``, ``strl`` with ``strh`` and ``strf``), ``movi``
    with one ``00dc`` chunk per frame (padded to even length), ``idx1``.  ``write(blob, sizes)`` appends frames, ``close()`` writes the
    index and patches the sizes and the frame count.  No OpenDML: a frame that would take the file past 2**31 - 1 bytes is refused
    before it is written."""

    _HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))   # "hdrl" + avih + LIST strl (strh, strf)

    def __init__(self, path: str, width: int, height: int, fps: float = 25.0):
        self.path, self.width, self.height, self.fps = path, int(width), int(height), float(fps)
        self.limit = RIFF_LIMIT
        self._index = []          # (offset from the "movi" fourcc, size) per frame
        self._max = 0
        self._f = open(path, "wb")
        self._f.write(self._headers(0, 0, 0))
        self._movi = self._f.tell() - 4          # position of the "movi" fourcc
        self._at = self._f.tell()

    def _headers(self, n: int, movi_bytes: int, riff_bytes: int) -> bytes:
        rate, scale = int(round(self.fps * 1000)), 1000
        w, h = self.width, self.height
        avih = struct.pack("<4sI14I", b"avih", 56, int(round(1e6 / self.fps)), 0, 0, 0x10, n, 0, 1, self._max, w, h, 0, 0, 0, 0)   # AVIF_HASINDEX
        strh = struct.pack("<4sI4s4sIHHIIIIIIII4H", b"strh", 56, b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, self._max, 0xFFFFFFFF, 0,
                           0, 0, w, h)
        strf = struct.pack("<4sIIiiHH4sIiiII", b"strf", 40, 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = struct.pack("<4sI4s", b"LIST", 4 + len(strh) + len(strf), b"strl") + strh + strf
        hdrl = struct.pack("<4sI4s", b"LIST", 4 + len(avih) + len(strl), b"hdrl") + avih + strl
        return struct.pack("<4sI4s", b"RIFF", riff_bytes, b"AVI ") + hdrl + struct.pack("<4sI4s", b"LIST", 4 + movi_bytes, b"movi")

    def write(self, blob, sizes) -> None:
        b = np.asarray(blob, np.uint8)
        at = 0
        for s in (int(v) for v in np.asarray(sizes).reshape(-1)):
            padded = s + (s & 1)
            # what the file would be with this frame: the chunks so far, this one, and an index entry for each
            if self._at + 8 + padded + 8 + 16 * (len(self._index) + 1) > self.limit:
                raise OpenGlottalHipError(f"{self.path}: frame {len(self._index)} would take the file past {self.limit} bytes, the most an "
                                          "AVI without OpenDML can hold; it was not written")
            self._f.write(struct.pack("<4sI", b"00dc", s))
            self._f.write(b[at:at + s].tobytes())
            if s & 1:
                self._f.write(b"\0")
            self._index.append((self._at - self._movi, s))
            self._max = max(self._max, s)
            self._at += 8 + padded
            at += s
        if at != b.size:
            raise OpenGlottalHipError(f"sizes add up to {at} bytes, the blob holds {b.size}")

    def close(self) -> None:
        if self._f is None:
            return
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, s) for off, s in self._index)   # AVIIF_KEYFRAME
        self._f.write(struct.pack("<4sI", b"idx1", len(idx)) + idx)
        end = self._f.tell()
        self._f.seek(0)
        self._f.write(self._headers(len(self._index), self._at - self._movi - 4, end - 8))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def riff_chunks(data: bytes, lo: int, hi: int):
    """``(fourcc, payload offset, size)`` of the chunks in ``data[lo:hi]``; a chunk that does not fit is an error."""
    at = lo
    while at < hi:
        if at + 8 > hi:
            raise OpenGlottalHipError(f"truncated RIFF chunk header at byte {at}")
        cc, n = struct.unpack_from("<4sI", data, at)
        if at + 8 + n > hi:
            raise OpenGlottalHipError(f"RIFF chunk {cc!r} at byte {at} runs past its parent")
        yield cc, at + 8, n
        at += 8 + n + (n & 1)


def avi_stream(path: str):
    """``(fccHandler of the first video stream or None, [JPEG bytes per 00dc chunk])`` of a RIFF AVI file."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise OpenGlottalHipError(f"{path} is not a RIFF AVI file")
    handler, frames = None, []
    for cc, at, n in riff_chunks(data, 12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0])):
        if cc != b"LIST":
            continue
        kind = data[at:at + 4]
        if kind == b"hdrl":
            for cc2, at2, n2 in riff_chunks(data, at + 4, at + n):
                if cc2 == b"LIST" and data[at2:at2 + 4] == b"strl" and handler is None:
                    for cc3, at3, n3 in riff_chunks(data, at2 + 4, at2 + n2):
                        if cc3 == b"strh" and data[at3:at3 + 4] == b"vids":
                            handler = data[at3 + 4:at3 + 8]
        elif kind == b"movi":
            for cc2, at2, n2 in riff_chunks(data, at + 4, at + n):
                if cc2 in (b"00dc", b"00db"):
                    frames.append(data[at2:at2 + n2])
    return handler, frames


def decode_jpeg_bgr(jpeg: bytes) -> np.ndarray:
    import io

    from PIL import Image

    im = Image.open(io.BytesIO(jpeg))
    im.load()
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def read_avi_mjpeg(path: str) -> list[np.ndarray]:
    """The frames of an ``MJPG`` AVI as BGR u8 arrays: a RIFF walk plus Pillow's decoder."""
    handler, frames = avi_stream(path)
    if handler is None or handler.upper() != b"MJPG":
        raise OpenGlottalHipError(f"{path}: the video stream is {handler!r}, only MJPG is decoded without OpenCV")
    return [decode_jpeg_bgr(j) for j in frames]


# ── decoding on the device (include/decode/openglottal_hip_mjpd.h) ──────────────────────────────────────────────────────────────────
STATUS = {0: "ok", 1: "truncated scan", 2: "invalid Huffman code", 3: "coefficient index past 63", 4: "value outside the baseline range",
          5: "restart marker count or order", 6: "unsupported form", 7: "size, sampling or restart interval differ from the call's"}
SAMPLING = {0: "gray", 1: "4:4:4", 2: "4:2:2", 3: "4:2:0"}
SPLIT = {"off": 0, "auto": 1}   # og_mjps_set_split's mode


class _Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "ncomp", "sampling", "Ri", "M", "nI", "tables")] + \
               [("scan_offset", C.c_int64), ("scan_length", C.c_int64), ("status", C.c_int32), ("reserved", C.c_int32)]


def decode_limit(which: int) -> int:
    return int(lib().og_mjpd_limit(which))


def _u8(jpeg) -> np.ndarray:
    return np.frombuffer(jpeg, np.uint8) if isinstance(jpeg, (bytes, bytearray, memoryview)) else np.ascontiguousarray(jpeg, np.uint8).reshape(-1)


def parse(jpeg) -> dict:
    """The headers of one JPEG file: ``H W ncomp sampling Ri M nI tables scan_offset scan_length status`` and, for a file the
    decoder refuses (``status`` 6), ``why``.  No entropy decoding."""
    a = _u8(jpeg)
    info = _Info()
    check(lib().og_jpegd_parse_host(ptr(a) if a.size else C.c_void_p(C.addressof(info)), a.size, C.addressof(info)), "og_jpegd_parse_host")
    d = {n: int(getattr(info, n)) for n, _ in _Info._fields_ if n != "reserved"}
    if d["status"]:
        d["why"] = (lib().og_last_error() or b"").decode()
    return d


def decode_host(jpeg, statuses: bool = False):
    """One JPEG file -> ``[H,W,3]`` u8 BGR on the CPU: the bytes the device produces (and, inside the header's bound, Pillow's).
    ``statuses=True`` returns ``(frame or None, status)`` instead of raising on a non-zero status."""
    a = _u8(jpeg)
    info = parse(a)
    if info["status"]:
        if statuses:
            return None, info["status"]
        raise OpenGlottalHipError(f"the JPEG decoder refuses the file: {info['why']}")
    out = np.empty((info["H"], info["W"], 3), np.uint8)
    st = C.c_int(-1)
    check(lib().og_jpegd_decode_host(ptr(a), a.size, ptr(out), out.size, C.addressof(st)), "og_jpegd_decode_host")
    if statuses:
        return out, st.value
    if st.value:
        raise OpenGlottalHipError(f"the JPEG file is damaged: {STATUS.get(st.value, st.value)}")
    return out


def split_limit(which: int) -> int:
    """``og_mjps_limit``: 0 the default ``sub``, 1 and 2 its bounds, 3 lanes per window, 4 bytes of a window, 5 the kernel's LDS."""
    return int(lib().og_mjps_limit(which))


def decode_split_host(jpeg, sub: int = 0, lanes: int = 256, statuses: bool = False, stats: bool = False):
    """``decode_host`` through the split entropy pass (include/split/openglottal_hip_mjps.h), the lanes walked in a loop: the same
    frame and status for every file.  ``sub``: bytes per lane (0: the default), ``lanes``: per window.  ``stats=True`` appends
    ``dict(lanes, windows, rounds, decodes)`` to the result."""
    a = _u8(jpeg)
    info = parse(a)
    counts = np.zeros(4, np.int32)
    names = ("lanes", "windows", "rounds", "decodes")
    if info["status"]:
        if not statuses:
            raise OpenGlottalHipError(f"the JPEG decoder refuses the file: {info['why']}")
        return (None, info["status"], dict(zip(names, [0] * 4))) if stats else (None, info["status"])
    out = np.empty((info["H"], info["W"], 3), np.uint8)
    st = C.c_int(-1)
    check(lib().og_jpegs_decode_host(ptr(a), a.size, int(sub), int(lanes), ptr(out), out.size, C.addressof(st), ptr(counts)),
          "og_jpegs_decode_host")
    if not statuses and st.value:
        raise OpenGlottalHipError(f"the JPEG file is damaged: {STATUS.get(st.value, st.value)}")
    res = (out, st.value) if statuses else (out,)
    if stats:
        res += ({k: int(v) for k, v in zip(names, counts)},)
    return res if len(res) > 1 else res[0]


def _pack(jpegs):
    """``(blob u8, offsets int64 [B + 1])`` of a list of files."""
    parts = [_u8(j) for j in jpegs]
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=offsets[1:])
    blob = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return (blob if blob.size else np.zeros(1, np.uint8)), offsets


def records_host(jpegs):
    """What the resident entry needs beside the bytes: ``(blob, offsets, recs int32 [B,8], tabs u8 [nsets, limit(3)], form)`` with
    ``form = dict(H, W, sampling, Ri)`` of the first file the parser accepts."""
    blob, offsets = _pack(jpegs)
    B = offsets.size - 1
    recs = np.zeros((B, 8), np.int32)
    tabs = np.zeros((max(B, 1), decode_limit(3)), np.uint8)
    out = (C.c_int * 5)()
    p = [C.addressof(out) + 4 * i for i in range(5)]
    check(lib().og_jpegd_records_host(ptr(blob), ptr(offsets), B, ptr(recs), ptr(tabs), tabs.shape[0], *p), "og_jpegd_records_host")
    return blob, offsets, recs, tabs[:out[0]].copy(), {"H": out[1], "W": out[2], "sampling": out[3], "Ri": out[4]}


class MjpegDecoder:
    """One ``og_mjpd`` handle: baseline JPEG files in, BGR frames out, decoded on the device.  All files of one call have one size,
    one sampling form and one restart interval (the first accepted file's)."""

    def __init__(self, chunk: int = 128, split: str = "off", sub=None):
        self._h = lib().og_mjpd_create()
        if not self._h:
            raise OpenGlottalHipError("og_mjpd_create failed")
        self.set_chunk(chunk)
        self.set_split(split, sub)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_mjpd_destroy(h)
            except Exception:
                pass

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_mjpd_set_chunk(self._h, int(chunk)), "og_mjpd_set_chunk")
        self.chunk = int(chunk)

    def set_split(self, split: str = "off", sub=None) -> None:
        """``"off"`` (the default): a lane per restart interval.  ``"auto"``: files WITHOUT restart markers are decoded by
        ``k_mjps_entropy``, ``sub`` bytes per lane (``None``: the measured default); files with markers are decoded as before."""
        if split not in SPLIT:
            raise OpenGlottalHipError(f"split must be one of {sorted(SPLIT)}, got {split!r}")
        check(lib().og_mjps_set_split(self._h, SPLIT[split], int(sub or 0)), "og_mjps_set_split")
        self.split, self.sub = split, int(sub or 0)

    def sync(self) -> None:
        check(lib().og_mjpd_sync(self._h), "og_mjpd_sync")

    @staticmethod
    def _raise(status, jpegs) -> None:
        bad = np.flatnonzero(status)
        if bad.size:
            i = int(bad[0])
            why = STATUS.get(int(status[i]), str(int(status[i])))
            if status[i] == 6:
                why += ": " + parse(jpegs[i]).get("why", "")
            raise OpenGlottalHipError(f"frame {i} of {len(status)} was not decoded (status {int(status[i])}): {why}")

    def _stream(self, jpegs, to_device: bool, statuses: bool):
        jpegs = list(jpegs)
        B = len(jpegs)
        first = next((i for i in (parse(j) for j in jpegs) if not i["status"]), None)
        H, W = (first["H"], first["W"]) if first else (0, 0)
        status = np.zeros(B, np.int32)
        blob, offsets = _pack(jpegs)
        if to_device:
            import torch

            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()   # (the handle runs on a stream of its own)
            host, dev, cap = None, out.data_ptr() if out.numel() else None, out.numel()
        else:
            out = np.empty((B, H, W, 3), np.uint8)
            host, dev, cap = ptr(out) if out.size else None, None, out.size
        hw = (C.c_int * 2)()
        if B and first:
            check(lib().og_mjpd_decode_stream(self._h, ptr(blob), ptr(offsets), B, host, dev, cap, ptr(status), C.addressof(hw),
                                              C.addressof(hw) + 4), "og_mjpd_decode_stream")
        elif B:
            status[:] = 6
        if statuses:
            return out, status
        self._raise(status, jpegs)
        return out

    def decode(self, jpegs, statuses: bool = False):
        """A list of JPEG files -> ``[B,H,W,3]`` u8 BGR on the host; only the compressed bytes go up.  Raises on the first frame with
        a non-zero status unless ``statuses=True``, which returns ``(frames, status int32 [B])``."""
        return self._stream(jpegs, False, statuses)

    def decode_resident(self, jpegs, statuses: bool = False):
        """The same, the frames staying on the device: a ``[B,H,W,3]`` u8 CUDA tensor that never visited the host."""
        return self._stream(jpegs, True, statuses)

    def set_tables(self, tabs, sampling: int, Ri: int) -> None:
        t = np.ascontiguousarray(tabs, np.uint8)
        check(lib().og_mjpd_set_tables(self._h, ptr(t), int(t.shape[0]) if t.ndim == 2 else 0, int(sampling), int(Ri)), "og_mjpd_set_tables")

    def decode_dev(self, blob_dev, offsets_dev, recs_dev, B: int, H: int, W: int, frames_dev, cap: int, status_dev) -> None:
        """Resident, asynchronous variant (torch CUDA tensors or raw ints) after ``set_tables``: see ``records_host``."""
        check(lib().og_mjpd_decode_u8_dev(self._h, ptr(blob_dev), ptr(offsets_dev), ptr(recs_dev), B, H, W, ptr(frames_dev), int(cap),
                                          ptr(status_dev)), "og_mjpd_decode_u8_dev")

    def plan(self, B: int, H: int, W: int, sampling: int = 1, Ri: int = 16):
        return decode_plan(B, H, W, sampling, Ri, self.chunk, self.split, self.sub)


def decode_plan(B: int, H: int, W: int, sampling: int = 1, Ri: int = 16, chunk: int = 128, split: str = "off", sub: int = 0):
    """Dry run of the streamed decode: ``(records, workspace_bytes)`` as ``plan`` gives them.  ``split`` other than ``"off"`` goes
    through ``og_mjps_plan``."""
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    if split == "off":
        n, what = lib().og_mjpd_plan(B, H, W, sampling, Ri, chunk, out, len(out), C.byref(ws)), "og_mjpd_plan"
    else:
        n, what = lib().og_mjps_plan(B, H, W, sampling, Ri, chunk, SPLIT.get(split, -1), int(sub or 0), out, len(out), C.byref(ws)), "og_mjps_plan"
    if n < 0:
        check(n, what)
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = [{k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, line.split("|"))} for line in out.value.decode().splitlines()]
    assert len(recs) == n
    return recs, ws.value


def jpeg_files(path: str) -> list[bytes]:
    """The compressed frames of an ``MJPG`` ``.avi`` file, or of a directory of ``.jpg`` / ``.jpeg`` files in name order."""
    import os

    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith((".jpg", ".jpeg")))
        if not names:
            raise OpenGlottalHipError(f"{path} holds no .jpg files")
        out = []
        for n in names:
            with open(os.path.join(path, n), "rb") as f:
                out.append(f.read())
        return out
    handler, frames = avi_stream(path)
    if handler is None or handler.upper() != b"MJPG":
        raise OpenGlottalHipError(f"{path}: the video stream is {handler!r}, only MJPG is decoded")
    return frames


class CompressedVideo:
    """The JPEG files of one video and the decoder that turns them into frames: what ``cli infer --decode device`` hands to the frame
    loops in place of decoded frames.  ``len`` is the frame count, ``[i]`` one frame decoded by the host twin (for a size or a seed
    frame), ``blocks_resident`` CUDA blocks that never visit the host, ``frames_host`` the whole video decoded block by block on the
    device and collected on the host (the detector's frame loop reads host frames)."""

    def __init__(self, files, decoder: MjpegDecoder | None = None):
        self.files = list(files)
        self.decoder = decoder if decoder is not None else MjpegDecoder()
        info = parse(self.files[0]) if self.files else {"H": 0, "W": 0, "status": 0}
        if info["status"]:
            raise OpenGlottalHipError(f"the JPEG decoder refuses the first frame: {info['why']}")
        self.H, self.W = info["H"], info["W"]
        self.compressed_bytes = sum(len(f) for f in self.files)

    def __len__(self) -> int:
        return len(self.files)

    def __getitem__(self, i):
        return decode_host(self.files[i])

    def blocks(self, block: int, resident: bool = False):
        """``(first frame index, frames)`` per block of ``block`` files: the one loop that hands files to the decoder."""
        for b0 in range(0, len(self.files), int(block)):
            part = self.files[b0:b0 + int(block)]
            yield b0, (self.decoder.decode_resident(part) if resident else self.decoder.decode(part))

    def blocks_resident(self, block: int):
        for _, frames in self.blocks(block, True):
            yield frames

    def frames_host(self, block: int = 1024) -> np.ndarray:
        if not self.files:
            return np.zeros((0, 0, 0, 3), np.uint8)
        out = np.empty((len(self.files), self.H, self.W, 3), np.uint8)
        for b0, frames in self.blocks(block):
            out[b0:b0 + len(frames)] = frames
        return out

def iter_avi_blocks(path: str, block: int, decoder: MjpegDecoder, resident: bool = False):
    """``(first frame index, frames)`` per block of ``block`` frames of an ``MJPG`` AVI (or a directory of ``.jpg`` files), decoded on
    the device (``CompressedVideo.blocks``); the decoded video is never held in host memory as a whole.  ``resident``: the blocks are
    CUDA tensors."""
    return CompressedVideo(jpeg_files(path), decoder).blocks(block, resident)


def open_compressed(path: str, mode: str = "device", split: str = "off"):
    """``CompressedVideo`` of an ``MJPG`` ``.avi`` or a directory of ``.jpg`` frames for ``--decode device``; with ``mode="auto"``
    ``None`` -- and one line on stderr saying why -- when the parser refuses the first frame, so that the caller takes the host loop.
    ``split``: ``--decode-split``, the decoder's ``set_split``."""
    import sys

    try:
        return CompressedVideo(jpeg_files(path), MjpegDecoder(split=split))
    except OpenGlottalHipError as e:
        if mode != "auto":
            raise
        print(f"--decode auto: {path} is decoded on the host: {e}", file=sys.stderr)
        return None
