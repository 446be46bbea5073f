"""Video output of the offscreen renderer: Motion-JPEG in an AVI container, the JPEG scans coded on the device (`phc_jpeg_encode`, include/phc_amd.h;
csrc/phc_jpeg.hip).

    python -m phc_amd.run test=True ... +render.video=out +render.format=avi [+render.quality=90]

The device codes the entropy-coded scan of every frame; the host builds the frame header once per (width, height, quality, restart interval), puts it in
front of each scan, EOI behind it, and appends the result to an AVI 1.0 file as one `00dc` chunk.  Any player reads the file: the stream is baseline JPEG
with the standard's typical Huffman tables carried in every frame.  Nothing here runs unless `render.format` asks for it: the training and benchmark
paths never import this module.
"""
import ctypes as C
import os
import struct

import numpy as np
import torch

from . import _lib as L
from . import abi

# MCUs (16 x 16 pixels) per restart segment.  A segment is the unit of parallelism of the entropy coder (one lane each), so the interval wants to be short:
# 2 gives 600 segments for one 640 x 480 view and 2400 for a 2 x 2 grid.  Each segment costs its RSTn marker (2 bytes), half a byte of padding on average and
# three DC values coded without a predictor; at 1 that overhead doubles for twice the lanes, at 4 the frame has 300 lanes' worth of work only.
DEFAULT_RESTART_INTERVAL = 2

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29,
          22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# ISO/IEC 10918-1 Tables K.1 / K.2, row-major
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Tables K.3 - K.6: (class << 4 | id, BITS, HUFFVAL); csrc/phc_jpeg.h codes with the same arrays
_AC_TAIL = tuple(r << 4 | s for r in range(16) for s in range(1, 11))   # (only to state the symbol set: every run / size pair, EOB and ZRL)
HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a535455565758595a"
        "636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4"
        "e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a"
        "636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4"
        "e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)
assert all(sum(b) == len(v) for _, b, v in HUFFMAN) and all(sorted(v) == sorted(_AC_TAIL + (0x00, 0xf0)) for t, _, v in HUFFMAN if t & 0x10)


def quant_tables(quality):
    """-> uint8 [2, 64], zigzag order: Tables K.1 / K.2 scaled by libjpeg's rule, s = 5000 / q below 50, else 200 - 2 q; clamp((t s + 50) / 100, 1, 255)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"render.quality={quality}: 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    nat = np.array([K1_LUMA, K2_CHROMA], dtype=np.int64)
    return np.clip((nat * s + 50) // 100, 1, 255).astype(np.uint8)[:, list(ZIGZAG)].copy()


def _segment(marker, payload):
    return bytes((0xff, marker)) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(width, height, quality, restart_interval):
    """Everything in front of the entropy-coded scan: SOI, APP0 (JFIF 1.01, square pixels), DQT x 2, SOF0 (8-bit, Y 2x2 / Cb 1x1 / Cr 1x1), DHT x 4, DRI, SOS."""
    w, h, ri = int(width), int(height), int(restart_interval)
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError(f"a JPEG frame is 1 .. 65535 pixels wide and high, not {w} x {h}")
    if ri < 1:
        raise ValueError(f"restart interval {ri}: at least 1 MCU")
    ri = min(ri, ((w + 15) // 16) * ((h + 15) // 16))   # (the device codes an interval above the frame's MCU count as one segment)
    if ri > 65535:
        raise ValueError(f"restart interval {ri}: DRI carries 16 bits")
    qt = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xe0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i in range(2):
        out += _segment(0xdb, bytes((i,)) + qt[i].tobytes())
    out += _segment(0xc0, struct.pack(">BHHB", 8, h, w, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, bits, vals in HUFFMAN:
        out += _segment(0xc4, bytes((tc_th,)) + bytes(bits) + bytes(vals))
    out += _segment(0xdd, struct.pack(">H", ri))
    return out + _segment(0xda, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


class JpegEncoder:
    """phc_jpeg_encode behind tensors: keeps the scratch block and the output block of the largest call so far."""

    def __init__(self, lib=None):
        self.lib = lib or L.load()
        self._scratch = self._out = None

    def _room(self, name, nbytes, device):
        t = getattr(self, name)
        if t is None or t.numel() < nbytes or t.device != device:
            t = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
            setattr(self, name, t)
        return t

    def scans(self, frames, quality=90, restart_interval=DEFAULT_RESTART_INTERVAL, coef=False):
        """frames: uint8 [F, H, W, 4] on a HIP device (rows and frames may be strided; a pixel's four bytes are contiguous).  -> list of F scans (bytes);
        with coef=True also the quantised coefficients int16 [F, 6 M, 64] (device)."""
        if frames.device.type != "cuda":
            raise RuntimeError(f"phc_jpeg_encode runs on a HIP device; the frames are on {frames.device} (there is no CPU fallback)")
        if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[3] != 4 or frames.stride(3) != 1 or frames.stride(2) != 4:
            raise ValueError("frames: uint8 [F, H, W, 4] with contiguous pixels")
        F, H, W = (int(v) for v in frames.shape[:3])
        ri = int(restart_interval)
        bound = int(self.lib.phc_jpeg_frame_bound(W, H, ri))
        need = int(self.lib.phc_jpeg_scratch_bytes(F, W, H, ri))
        if bound < 0 or need < 0:
            raise ValueError(f"phc_jpeg_encode refuses {F} frames of {W} x {H} at restart interval {ri}")
        dev = frames.device
        out = self._room("_out", F * bound, dev)
        scratch = self._room("_scratch", need, dev)
        length = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
        co = torch.empty((F, 6 * ((W + 15) // 16) * ((H + 15) // 16), 64), dtype=torch.int16, device=dev) if coef else None
        qt = quant_tables(quality)
        row, frame = int(frames.stride(1)), int(frames.stride(0))
        a = abi.jpeg_args_struct(F, W, H, ri, row, frame if F > 1 else max(frame, H * row), bound, scratch.numel(), rgba=frames.data_ptr(), qtab=qt, out=out,
                                 length=length, scratch=scratch, coef=co)
        L.check(self.lib.phc_jpeg_encode(C.byref(a), torch.cuda.current_stream().cuda_stream), "phc_jpeg_encode")
        n = length[:F].cpu().tolist()                                                      # one copy of F lengths ...
        packed = torch.cat([out[f * bound:f * bound + n[f]] for f in range(F)]).cpu().numpy().tobytes() if F else b""   # ... and one of the scans alone
        ends = np.cumsum([0] + n)
        scans = [packed[ends[f]:ends[f + 1]] for f in range(F)]
        return (scans, co) if coef else scans

    def encode(self, frames, quality=90, restart_interval=DEFAULT_RESTART_INTERVAL):
        """-> list of F complete JPEG files (bytes)."""
        head = jpeg_header(frames.shape[2], frames.shape[1], quality, restart_interval)
        return [head + s + b"\xff\xd9" for s in self.scans(frames, quality, restart_interval)]


_ENCODER = None


def encode_frames(frames_on_device, quality=90, restart_interval=DEFAULT_RESTART_INTERVAL):
    """uint8 [F, H, W, 4] (or one [H, W, 4]) on a HIP device -> list of complete JPEG byte strings, coded in one phc_jpeg_encode call."""
    global _ENCODER
    if _ENCODER is None:
        _ENCODER = JpegEncoder()
    f = frames_on_device if frames_on_device.ndim == 4 else frames_on_device[None]
    return _ENCODER.encode(f, quality, restart_interval)


AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10
AVI_PART_BYTES = 1 << 30   # AVI 1.0 sizes are 32-bit; players and muxers agree on 1 GiB parts


class AviWriter:
    """AVI 1.0 (RIFF) with one `vids` / `MJPG` stream: `add(jpeg)` appends a frame as a `00dc` chunk (padded to even length), `close()` writes `idx1` and patches
    the sizes and counts.  A part that would pass `part_bytes` is closed and `<name>-partNN.avi` opened (`paths` lists them all)."""

    def __init__(self, path, width, height, fps, part_bytes=AVI_PART_BYTES):
        self.width, self.height, self.fps = int(width), int(height), int(round(float(fps)))
        if self.fps < 1 or self.width < 1 or self.height < 1:
            raise ValueError("AviWriter: width, height and fps are at least 1")
        self.path, self.part_bytes = str(path), int(part_bytes)
        self.paths, self.frames = [], 0
        self._f = None
        self._open(self.path)

    def _open(self, path):
        w, h = self.width, self.height
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), 0, 0, AVIF_HASINDEX, 0, 0, 1, 0, w, h, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIiI4H", 0, 0, 0, 0, 1, self.fps, 0, 0, 0, -1, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"RIFF" + b"\0\0\0\0" + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
        o_avih = head.index(b"avih") + 8
        o_strh = head.index(b"strh") + 8
        self._patch = dict(max_bytes_per_sec=o_avih + 4, total_frames=o_avih + 16, suggested=o_avih + 28, length=o_strh + 32, strh_suggested=o_strh + 36,
                           movi_size=len(head) + 4)
        head += b"LIST" + b"\0\0\0\0" + b"movi"
        self._movi = len(head) - 4            # idx1 offsets count from the `movi` fourcc
        self._f = open(path, "wb")
        self._f.write(head)
        self._pos, self._index, self._largest = len(head), [], 0
        self.paths.append(path)

    def add(self, jpeg):
        n = len(jpeg)
        chunk = 8 + n + (n & 1)
        if self._index and self._pos + chunk + 8 + 16 * (len(self._index) + 1) > self.part_bytes:
            self._finish()
            stem, ext = os.path.splitext(self.path)
            self._open(f"{stem}-part{len(self.paths) + 1:02d}{ext}")
        self._f.write(b"00dc" + struct.pack("<I", n) + jpeg + (b"\0" if n & 1 else b""))
        self._index.append((self._pos - self._movi, n))
        self._pos += chunk
        self._largest = max(self._largest, n)
        self.frames += 1

    def _finish(self):
        f, k = self._f, len(self._index)
        f.write(b"idx1" + struct.pack("<I", 16 * k) + b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, n) for off, n in self._index))
        end = self._pos + 8 + 16 * k
        total = sum(n for _, n in self._index)
        for key, val in (("max_bytes_per_sec", min(0xffffffff, total * self.fps // max(k, 1))), ("total_frames", k), ("suggested", self._largest), ("length", k),
                         ("strh_suggested", self._largest), ("movi_size", self._pos - self._movi)):
            f.seek(self._patch[key])
            f.write(struct.pack("<I", val))
        f.seek(4)
        f.write(struct.pack("<I", end - 8))
        f.close()
        self._f = None

    def close(self):
        if self._f is not None:
            self._finish()
