"""PNG input decoded on the device (include_ext/openglottal_hip_png.h): the frames and ground-truth masks that `scripts/eval_bagls.py`,
`eval_girafe.py`, `sweep_bagls_conf.py` and `infer.py --mode images` read through OpenCV go up COMPRESSED; inflate, unfilter and the
expansion to B G R (or gray) run on the device.  PNG is lossless: the host twin (`decode_host`) gives Pillow's `convert("RGB")` /
`convert("L")` bytes for every file it accepts, and the device gives the twin's bytes and statuses.

``PngDecoder`` wraps one ``og_png`` handle.  The files of one call may differ in size and form; a call returns one ``[B,H,W,C]`` array
when the sizes agree and a list of ``[H,W,C]`` arrays otherwise.

PNG output is coded on the device as well (include_enc/openglottal_hip_pnge.h): ``PngEncoder`` wraps one ``og_pnge`` handle
and turns frames of one shape into complete files; ``encode_host`` is its twin, byte for byte.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import OpenGlottalHipError, check, lib, ptr
from .mjpeg import CompressedVideo, _pack, _u8

STATUS = {0: "ok", 1: "truncated stream", 2: "invalid deflate data", 3: "distance before the first output byte",
          4: "output past H * (1 + rb) bytes", 5: "zlib wrapper or Adler-32", 6: "unsupported form", 7: "filter type above 4"}
CTYPE = {0: "gray", 2: "RGB", 3: "palette", 4: "gray+alpha", 6: "RGBA"}


class _Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "ctype", "depth", "samples", "rb", "bpp", "npal", "nidat", "status")] + \
               [("raw_bytes", C.c_int64), ("zlib_bytes", C.c_int64)]


def limit(which: int) -> int:
    return int(lib().og_png_limit(which))


def parse(png) -> dict:
    """The chunks of one PNG file: ``H W ctype depth samples rb bpp npal nidat raw_bytes zlib_bytes status`` and, for a file the
    decoder refuses (``status`` 6), ``why``.  Nothing is inflated."""
    a = _u8(png)
    info = _Info()
    check(lib().og_pngd_parse_host(ptr(a) if a.size else C.c_void_p(C.addressof(info)), a.size, C.addressof(info)), "og_pngd_parse_host")
    d = {n: int(getattr(info, n)) for n, _ in _Info._fields_}
    if d["status"]:
        d["why"] = (lib().og_last_error() or b"").decode()
    return d


def inflate_host(stream, cap: int):
    """One zlib stream through the twin's inflate: ``(bytes produced, status)``; at most ``cap`` bytes."""
    a = _u8(stream)
    out = np.zeros(max(int(cap), 1), np.uint8)
    n, st = C.c_size_t(), C.c_int(-1)
    check(lib().og_pngd_inflate_host(ptr(a) if a.size else ptr(out), a.size, ptr(out), int(cap), C.addressof(n), C.addressof(st)),
          "og_pngd_inflate_host")
    return out[:n.value].tobytes(), st.value


def decode_host(png, channels: int = 3, statuses: bool = False):
    """One PNG file -> ``[H,W,channels]`` u8 on the CPU (3: B G R, 1: gray): the bytes the device produces, and Pillow's.
    ``statuses=True`` returns ``(pixels or None, status)`` instead of raising on a non-zero status."""
    a = _u8(png)
    info = parse(a)
    if info["status"]:
        if statuses:
            return None, info["status"]
        raise OpenGlottalHipError(f"the PNG decoder refuses the file: {info['why']}")
    out = np.empty((info["H"], info["W"], int(channels)), np.uint8)
    st = C.c_int(-1)
    check(lib().og_pngd_decode_host(ptr(a), a.size, int(channels), ptr(out), out.size, C.addressof(st)), "og_pngd_decode_host")
    if statuses:
        return out, st.value
    if st.value:
        raise OpenGlottalHipError(f"the PNG file is damaged: {STATUS.get(st.value, st.value)}")
    return out


def _ihdr_pixels(a: np.ndarray) -> int:
    """H * W as the IHDR states it, 0 if there is none: an upper bound of what the file can take in the output."""
    if a.size < 24:
        return 0
    w, h = (int.from_bytes(a[i:i + 4].tobytes(), "big") for i in (16, 20))
    return h * w if 0 < h * w <= limit(0) else 0


def records_host(pngs, channels: int = 3):
    """What the resident entry needs: ``dict(zblob, zoffsets, recs, pals, out_bytes, raw_bytes, max_pixels)``; ``recs`` is a
    structured array of ``og_png_rec`` (H W ctype depth palette status out_offset raw_offset)."""
    blob, offsets = _pack(pngs)
    B = offsets.size - 1
    recs = np.zeros(B, REC)
    zblob = np.zeros(max(int(offsets[-1]), 1), np.uint8)
    zoffsets = np.zeros(B + 1, np.int64)
    pals = np.zeros((max(B, 1), 768), np.uint8)
    npals = C.c_int()
    totals = np.zeros(3, np.int64)
    check(lib().og_pngd_records_host(ptr(blob), ptr(offsets), B, int(channels), ptr(recs), ptr(zblob), zblob.size, ptr(zoffsets), ptr(pals),
                                     pals.shape[0], C.addressof(npals), ptr(totals)), "og_pngd_records_host")
    return {"zblob": zblob[:max(int(zoffsets[-1]), 1)].copy(), "zoffsets": zoffsets, "recs": recs, "pals": pals[:npals.value].copy(),
            "out_bytes": int(totals[0]), "raw_bytes": int(totals[1]), "max_pixels": int(totals[2])}


REC = np.dtype([(n, np.int32) for n in ("H", "W", "ctype", "depth", "palette", "status")] + [("out_offset", np.int64), ("raw_offset", np.int64)])
assert REC.itemsize == 40


class PngDecoder:
    """One ``og_png`` handle: PNG files in, pixels out, decoded on the device.  The files of a call may differ in size and form."""

    def __init__(self, chunk: int = 128):
        self._h = lib().og_png_create()
        if not self._h:
            raise OpenGlottalHipError("og_png_create failed")
        self.set_chunk(chunk)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_png_destroy(h)
            except Exception:
                pass

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_png_set_chunk(self._h, int(chunk)), "og_png_set_chunk")
        self.chunk = int(chunk)

    def sync(self) -> None:
        check(lib().og_png_sync(self._h), "og_png_sync")

    @staticmethod
    def _raise(status, files) -> None:
        bad = np.flatnonzero(status)
        if bad.size:
            i = int(bad[0])
            why = STATUS.get(int(status[i]), str(int(status[i])))
            if status[i] == 6:
                why += ": " + parse(files[i]).get("why", "")
            raise OpenGlottalHipError(f"file {i} of {len(status)} was not decoded (status {int(status[i])}): {why}")

    def _stream(self, files, channels: int, to_device: bool, statuses: bool):
        parts = [_u8(f) for f in files]
        B, Cn = len(parts), int(channels)
        blob, offsets = _pack(parts)
        cap = sum(_ihdr_pixels(a) for a in parts) * Cn
        status = np.zeros(B, np.int32)
        out_offsets = np.zeros(B + 1, np.int64)
        hw = np.zeros((max(B, 1), 2), np.int32)
        if to_device:
            import torch

            flat = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()   # (the handle runs on a stream of its own)
            host, dev = None, flat.data_ptr()
        else:
            flat = np.empty(max(cap, 1), np.uint8)
            host, dev = ptr(flat), None
        check(lib().og_png_decode_stream(self._h, ptr(blob), ptr(offsets), B, Cn, host, dev, cap, ptr(out_offsets), ptr(hw), ptr(status)),
              "og_png_decode_stream")
        if not statuses:
            self._raise(status, parts)
        shapes = [(int(h), int(w), Cn) for h, w in hw[:B]]
        if B and len(set(shapes)) == 1 and out_offsets[B] == B * int(np.prod(shapes[0])):
            out = flat[:int(out_offsets[B])].reshape((B,) + shapes[0])
        else:
            out = [flat[int(out_offsets[i]):int(out_offsets[i + 1])].reshape(s) for i, s in enumerate(shapes)]
        return (out, status) if statuses else out

    def decode(self, files, channels: int = 3, statuses: bool = False):
        """A list of PNG files -> u8 pixels on the host, ``[B,H,W,C]`` when the sizes agree, else a list of ``[H,W,C]``; only the
        compressed bytes go up.  Raises on the first file with a non-zero status unless ``statuses=True``, which returns
        ``(pixels, status int32 [B])``: a file with a non-zero status is all zeros, a refused one (6) has shape ``(0, 0, C)``."""
        return self._stream(files, channels, False, statuses)

    def decode_resident(self, files, channels: int = 3, statuses: bool = False):
        """The same, the pixels staying on the device: CUDA tensors that never visited the host."""
        return self._stream(files, channels, True, statuses)

    def set_palettes(self, pals) -> None:
        p = np.ascontiguousarray(pals, np.uint8).reshape(-1, 768)
        check(lib().og_png_set_palettes(self._h, ptr(p) if p.size else None, int(p.shape[0])), "og_png_set_palettes")

    def decode_dev(self, zblob_dev, zoffsets_dev, recs_dev, B: int, channels: int, raw_bytes: int, max_pixels: int, out_dev, cap: int,
                   status_dev) -> None:
        """Resident, asynchronous variant (torch CUDA tensors or raw ints) after ``set_palettes``: see ``records_host``."""
        check(lib().og_png_decode_u8_dev(self._h, ptr(zblob_dev), ptr(zoffsets_dev), ptr(recs_dev), int(B), int(channels), int(raw_bytes),
                                         int(max_pixels), ptr(out_dev), int(cap), ptr(status_dev)), "og_png_decode_u8_dev")

    def plan(self, forms, channels: int = 3):
        return plan(forms, channels, self.chunk)


def plan(forms, channels: int = 3, chunk: int = 128):
    """Dry run of the streamed decode over files of ``forms`` ``[(H, W, ctype, depth), ...]``: ``(records, workspace_bytes)``; a
    record is a dict of the plan line's fields."""
    f = np.ascontiguousarray(forms, np.int32).reshape(-1, 4)
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = lib().og_png_plan(ptr(f), int(f.shape[0]), int(channels), int(chunk), out, len(out), C.byref(ws))
    if n < 0:
        check(n, "og_png_plan")
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = [{k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, line.split("|"))} for line in out.value.decode().splitlines()]
    assert len(recs) == n
    return recs, ws.value


# ── PNG output encoded on the device (include_enc/openglottal_hip_pnge.h) ────────────────────────────────────────────────────────────
def _frames4(frames) -> np.ndarray:
    a = np.ascontiguousarray(frames, np.uint8)
    if a.ndim == 3:
        a = a[..., None]
    if a.ndim != 4 or a.shape[3] not in (1, 3):
        raise OpenGlottalHipError(f"frames must be [B,H,W] or [B,H,W,C] u8 with C = 1 (gray) or 3 (B G R), not {a.shape}")
    return a


def encode_limit(which: int) -> int:
    return int(lib().og_pnge_limit(which))


def encode_bound(H: int, W: int, C: int = 3, segment: int = 32768) -> int:
    """Worst-case bytes of one encoded file: every segment stored."""
    n = int(lib().og_pnge_bound(int(H), int(W), int(C), int(segment)))
    if n < 0:
        check(-1, "og_pnge_bound")
    return n


def filter_host(frame) -> bytes:
    """The raw stream of one ``[H,W,C]`` frame: per row the filter type of least cost and the filtered bytes."""
    a = _frames4(np.asarray(frame)[None])[0]
    H, W, Cn = a.shape
    out = np.empty(H * (1 + W * Cn), np.uint8)
    check(lib().og_pnge_filter_host(ptr(a), H, W, Cn, ptr(out), out.size), "og_pnge_filter_host")
    return out.tobytes()


def deflate_host(raw, segment: int = 32768) -> bytes:
    """Raw bytes -> the encoder's zlib stream: run-length tokens, one dynamic (or stored) block per ``segment`` bytes."""
    a = _u8(raw)
    out = np.empty(6 + a.size + 5 * ((a.size + int(segment) - 1) // int(segment)) + 8, np.uint8)
    n = C.c_size_t()
    check(lib().og_pnge_deflate_host(ptr(a), a.size, int(segment), ptr(out), out.size, C.addressof(n)), "og_pnge_deflate_host")
    return out[:n.value].tobytes()


def encode_host(frame, segment: int = 32768) -> bytes:
    """One ``[H,W]`` / ``[H,W,1]`` gray or ``[H,W,3]`` B G R frame -> a complete PNG file on the CPU: the bytes the device produces."""
    a = _frames4(np.asarray(frame)[None])[0]
    H, W, Cn = a.shape
    out = np.empty(encode_bound(H, W, Cn, segment), np.uint8)
    n = C.c_int()
    check(lib().og_pnge_encode_host(ptr(a), H, W, Cn, int(segment), ptr(out), out.size, C.addressof(n)), "og_pnge_encode_host")
    return out[:n.value].tobytes()


class PngEncoder:
    """One ``og_pnge`` handle: frames of one shape in, complete PNG files out, encoded on the device."""

    def __init__(self, chunk: int = 128, segment: int = 32768):
        self._h = lib().og_pnge_create()
        if not self._h:
            raise OpenGlottalHipError("og_pnge_create failed")
        self.set_chunk(chunk)
        self.set_segment(segment)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_pnge_destroy(h)
            except Exception:
                pass

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_pnge_set_chunk(self._h, int(chunk)), "og_pnge_set_chunk")
        self.chunk = int(chunk)

    def set_segment(self, segment: int) -> None:
        check(lib().og_pnge_set_segment(self._h, int(segment)), "og_pnge_set_segment")
        self.segment = int(segment)

    def sync(self) -> None:
        check(lib().og_pnge_sync(self._h), "og_pnge_sync")

    def encode(self, frames):
        """``[B,H,W,C]`` u8 on the host -> ``(blob u8, sizes int32 [B])``: the B files back to back; only the bytes used come back."""
        a = _frames4(frames)
        B, H, W, Cn = a.shape
        cap = B * encode_bound(H, W, Cn, self.segment)
        out = np.empty(max(cap, 1), np.uint8)
        sizes = np.zeros(B, np.int32)
        total = C.c_longlong()
        check(lib().og_pnge_encode_stream_u8(self._h, ptr(a), B, H, W, Cn, ptr(out), cap, ptr(sizes), C.addressof(total)), "og_pnge_encode_stream_u8")
        return out[:total.value].copy(), sizes

    def encode_resident(self, frames_ptr, B: int, H: int, W: int, C_: int = 3):
        """Frames resident on the device (a CUDA tensor or a raw address) -> ``(blob, sizes, total)`` as CUDA tensors: u8 of
        ``B * encode_bound`` bytes of which the first ``total[0]`` hold the files, int32 ``[B]``, int64 ``[1]``.  Asynchronous: call
        ``sync()`` before reading them from another stream."""
        import torch

        cap = int(B) * encode_bound(H, W, C_, self.segment)
        blob = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(max(int(B), 1), dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()   # (the handle runs on a stream of its own)
        check(lib().og_pnge_encode_u8_dev(self._h, ptr(frames_ptr), int(B), int(H), int(W), int(C_), ptr(blob), cap, ptr(sizes), ptr(total)),
              "og_pnge_encode_u8_dev")
        return blob, sizes[:int(B)], total

    def files_resident(self, frames_ptr, B: int, H: int, W: int, C_: int = 3) -> list[bytes]:
        """``encode_resident`` and the files fetched: only their bytes cross the bus."""
        blob, sizes, total = self.encode_resident(frames_ptr, B, H, W, C_)
        self.sync()
        sizes = sizes.cpu().numpy()
        data = blob[:int(total[0])].cpu().numpy()
        ends = np.cumsum(sizes.astype(np.int64))
        return [data[int(e - n):int(e)].tobytes() for e, n in zip(ends, sizes)]

    def label_bbox_dev(self, labels_dev, B: int, H: int, W: int):
        """``[B,H,W]`` u8 labels resident on the device -> int32 ``[B,4]`` CUDA tensor: the tight box ``x0 y0 x1+1 y1+1`` of
        ``label > 0``, ``0 0 0 0`` for an empty label (``k_label_bbox``).  Waited for."""
        import torch

        boxes = torch.zeros((max(int(B), 1), 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        check(lib().og_pnge_label_bbox_u8_dev(self._h, ptr(labels_dev), int(B), int(H), int(W), ptr(boxes)), "og_pnge_label_bbox_u8_dev")
        self.sync()
        return boxes[:int(B)]

    def crop_tiles_dev(self, frames_dev, B: int, H: int, W: int, channels: int, boxes_dev, size: int):
        """``k_crop_tiles`` alone: ``[B,H,W,channels]`` u8 frames and int32 ``[B,4]`` boxes on the device -> ``[B,size,size]`` u8 gray
        tiles there, ready for ``encode_resident(tiles, B, size, size, 1)``.  Waited for."""
        import torch

        tiles = torch.empty((max(int(B), 1), int(size), int(size)), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        check(lib().og_pnge_crop_tiles_u8_dev(self._h, ptr(frames_dev), int(B), int(H), int(W), int(channels), ptr(boxes_dev), int(size), ptr(tiles)),
              "og_pnge_crop_tiles_u8_dev")
        self.sync()
        return tiles[:int(B)]

    def files(self, frames) -> list[bytes]:
        """The files of ``encode`` as a list of ``bytes``."""
        blob, sizes = self.encode(frames)
        ends = np.cumsum(sizes.astype(np.int64))
        return [blob[int(e - n):int(e)].tobytes() for e, n in zip(ends, sizes)]

    def plan(self, B: int, H: int, W: int, C_: int = 3):
        return encode_plan(B, H, W, C_, self.segment, self.chunk)


def encode_plan(B: int, H: int, W: int, C_: int = 3, segment: int = 32768, chunk: int = 128):
    """Dry run of the streamed encode: ``(records, workspace_bytes)``; a record is a dict of the plan line's fields."""
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = lib().og_pnge_plan(int(B), int(H), int(W), int(C_), int(segment), int(chunk), out, len(out), C.byref(ws))
    if n < 0:
        check(n, "og_pnge_plan")
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = [{k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, line.split("|"))} for line in out.value.decode().splitlines()]
    assert len(recs) == n
    return recs, ws.value


# ── files and directories ───────────────────────────────────────────────────────────────────────────────────────────────────────────
def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def png_files(path: str) -> list[bytes]:
    """The ``.png`` files of a directory in name order, as bytes."""
    names = sorted(n for n in os.listdir(path) if n.lower().endswith(".png"))
    if not names:
        raise OpenGlottalHipError(f"{path} holds no .png files")
    return [_read(os.path.join(path, n)) for n in names]


def bagls_pairs(path: str, max_images: int = 0):
    """``(image paths, label paths)`` of a BAGLS-style directory by the listing rule of `scripts/eval_bagls.py:135-145`: the ``N.png``
    files that are no ``N_seg.png``, sorted, cut to ``max_images`` when that is not 0, and then the pairs without a label left out."""
    imgs = sorted(os.path.join(path, n) for n in os.listdir(path) if n.endswith(".png") and not n.endswith("_seg.png"))
    if max_images:
        imgs = imgs[:int(max_images)]
    pairs = [(p, p[:-4] + "_seg.png") for p in imgs]
    pairs = [(p, s) for p, s in pairs if os.path.exists(s)]
    return [p for p, _ in pairs], [s for _, s in pairs]


def read_pairs(image_files, label_files, decoder: PngDecoder | None = None):
    """``(frames, gts)`` of paired PNG files (paths or bytes), decoded on the device: frames at C = 3 (``[H,W,3]`` B G R), labels at
    C = 1 (``[H,W]``) -- what ``evaluate``, ``evaluate_device``, ``sweep.conf_sweep`` and ``sweep.hold_ablation`` take.  One array each
    when the sizes agree, else lists."""
    image_files, label_files = list(image_files), list(label_files)
    if len(image_files) != len(label_files):
        raise OpenGlottalHipError(f"{len(image_files)} images but {len(label_files)} labels")
    d = decoder if decoder is not None else PngDecoder()
    load = lambda fs: [f if isinstance(f, (bytes, bytearray, memoryview, np.ndarray)) else _read(os.fspath(f)) for f in fs]   # noqa: E731
    frames = d.decode(load(image_files), 3)
    gts = d.decode(load(label_files), 1)
    gts = gts[..., 0] if isinstance(gts, np.ndarray) else [g[..., 0] for g in gts]
    return frames, gts


class CompressedImages(CompressedVideo):
    """The PNG files of an image sequence of ONE size and the decoder that turns them into frames: what ``cli infer --mode images
    --decode device`` hands to the frame loops (``CompressedVideo``'s interface)."""

    def __init__(self, files, decoder: PngDecoder | None = None):
        self.files = list(files)
        self.decoder = decoder if decoder is not None else PngDecoder()
        infos = [parse(f) for f in self.files]
        for i, info in enumerate(infos):
            if info["status"]:
                raise OpenGlottalHipError(f"the PNG decoder refuses frame {i}: {info['why']}")
        sizes = {(i["H"], i["W"]) for i in infos}
        if len(sizes) > 1:
            raise OpenGlottalHipError(f"the .png frames have {len(sizes)} different sizes; an image sequence has one")
        self.H, self.W = sizes.pop() if sizes else (0, 0)
        self.compressed_bytes = sum(len(f) for f in self.files)

    def __getitem__(self, i):
        return decode_host(self.files[i])


def open_compressed(path: str, mode: str = "device"):
    """``CompressedImages`` of a directory of ``.png`` frames for ``--decode device``; with ``mode="auto"`` ``None`` -- and one line on
    stderr saying why -- when the parser refuses a frame or the sizes differ, so that the caller takes the host loop."""
    import sys

    try:
        return CompressedImages(png_files(path))
    except OpenGlottalHipError as e:
        if mode != "auto":
            raise
        print(f"--decode auto: {path} is decoded on the host: {e}", file=sys.stderr)
        return None
