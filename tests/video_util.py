"""Shared by tests/test_video_cpu.py and tests/test_video_gpu.py: the host build of phc_amd/csrc/phc_jpeg.h (tests/jpeg_shim.cpp, g++), callers of it and of
the C ABI with guard bytes around every output, and the three things the encoder is measured against, all written from ISO/IEC 10918-1 and the RIFF / AVI
documents and not from phc_jpeg.h or phc_amd/video.py:
  (a) `oracle`      the transform in fp64 numpy: colour, edge extension, 2 x 2 chroma mean, DCT by the cosine formula, quantiser, rounding, zigzag;
  (b) `decode`      a baseline entropy decoder (Annex F): markers, DQT / DHT / DRI, RSTn, byte unstuffing -> the quantised coefficients;
  (c) `read_avi`    a RIFF walker for the AVI files.
The test images and the constructed blocks live here too, so that the CPU and the GPU tests run the same cases under the same rules."""
import ctypes as C
import functools
import struct

import numpy as np

import host_build

GUARD, PAD = 0xA5, 64
U32 = 2.0 ** -24     # fp32 unit round-off


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("jpeg_shim.cpp", "phc_jpeg.hip")
    lib.jpeg_args_check_of.argtypes = [C.POINTER(L.JpegArgs)]
    lib.jpeg_encode_host.argtypes = [C.POINTER(L.JpegArgs)]
    lib.jpeg_frame_bound_of.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.jpeg_frame_bound_of.restype = C.c_int64
    lib.jpeg_scratch_bytes_of.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.jpeg_scratch_bytes_of.restype = C.c_int64
    lib.jpeg_huff_table.argtypes = [C.c_void_p]
    lib.jpeg_huff_table.restype = None
    return lib


# ---------------------------------------------------------------------------------------------------------------- the standard, restated
def zigzag():
    """Figure A.6 by walking the anti-diagonals: -> list of 64 row-major indices."""
    out = []
    for d in range(15):
        cells = [(v, d - v) for v in range(8) if 0 <= d - v < 8]          # (v, u), v ascending
        out += [8 * v + u for v, u in (cells if d % 2 else cells[::-1])]   # even diagonals run upward (v descending)
    return out


K1 = """16 11 10 16 24 40 51 61  12 12 14 19 26 58 60 55  14 13 16 24 40 57 69 56  14 17 22 29 51 87 80 62
        18 22 37 56 68 109 103 77  24 35 55 64 81 104 113 92  49 64 78 87 103 121 120 101  72 92 95 98 112 100 103 99"""
K2 = """17 18 24 47 99 99 99 99  18 21 26 66 99 99 99 99  24 26 56 99 99 99 99 99  47 66 99 99 99 99 99 99""" + " 99" * 32


def qtables(quality):
    """-> int64 [2, 64] in zigzag order: K.1 / K.2 under libjpeg's scaling."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    nat = np.array([[int(t) for t in K1.split()], [int(t) for t in K2.split()]], dtype=np.int64)
    return np.clip((nat * s + 50) // 100, 1, 255)[:, zigzag()]


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[0] /= np.sqrt(2.0)
    return m


def tie_tolerance():
    """How far the fp32 transform can be from the fp64 one, as an absolute error of a coefficient S before the division, to first order in u = 2^-24:
      colour   a sample is three products of a byte (<= 255) with a constant rounded to fp32, two sums and the level shift: 3 x 2 + 3 roundings of numbers
               <= 255 -> e0 = 9 u 255 (the 2 x 2 mean of bytes is exact);
      a pass   an eight-term sum of products with the rounded matrix entries: (8 + 1) u sum|m||s|, and it carries the error of its input times
               A = max_u sum_x |m(u, x)| (row u = 0: 8 / (2 sqrt 2) = 2.83).  Level-shifted samples are <= 128, so sum|m||s| <= 128 A in the row pass and
               <= 128 A^2 in the column pass:  e1 = A e0 + 9 u 128 A,  e2 = A e1 + 9 u 128 A^2.
    -> e2 (2.2e-3).  A coefficient is a tie when its unrounded |S| / q lies within e2 / q + 2 u |S| / q of k + 1/2 (the division and the + 0.5 round once each)."""
    A = np.abs(dct_matrix()).sum(1).max()
    e0 = 9 * U32 * 255
    e1 = A * e0 + 9 * U32 * 128 * A
    return A * e1 + 9 * U32 * 128 * A * A


def oracle(rgb, qt):
    """rgb uint8 [H, W, 3], qt [2, 64] zigzag -> (coef int64 [6 M, 64], tie bool [6 M, 64]): planes Y (raster over a 2 mcux wide grid), Cb, Cr."""
    H, W = rgb.shape[:2]
    eh, ew = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    p = np.pad(rgb.astype(np.float64), ((0, eh - H), (0, ew - W), (0, 0)), mode="edge")
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = -0.168735892 * R - 0.331264108 * G + 0.5 * B + 128
    Cr = 0.5 * R - 0.418687589 * G - 0.081312411 * B + 128
    mean = lambda c: c.reshape(eh // 2, 2, ew // 2, 2).mean(axis=(1, 3))
    m, zz, e2 = dct_matrix(), zigzag(), tie_tolerance()
    coef, tie = [], []
    for plane, q in ((Y, qt[0]), (mean(Cb), qt[1]), (mean(Cr), qt[1])):
        h, w = plane.shape
        blocks = (plane - 128.0).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        S = np.einsum("vy,nyx,ux->nvu", m, blocks, m).reshape(-1, 64)[:, zz]
        r = np.abs(S) / q
        c = np.sign(S) * np.floor(r + 0.5)
        coef.append(c.astype(np.int64))
        tie.append(np.abs(r - np.floor(r) - 0.5) <= e2 / q + 2 * U32 * r)
    return np.concatenate(coef), np.concatenate(tie)


class _Bits:
    def __init__(self, data):
        self.d, self.pos, self.n = data, 0, len(data) * 8

    def bit(self):
        if self.pos >= self.n:
            raise ValueError("entropy-coded segment ends inside a code")
        b = (self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v


def _huff_decoder(bits, vals):
    table, code, n = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            table[(ln, code)] = vals[n]
            code, n = code + 1, n + 1
        code <<= 1
    return table


def _symbol(br, table):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | br.bit()
        if (ln, code) in table:
            return table[(ln, code)]
    raise ValueError("no Huffman code of 16 bits or fewer matches")


def _extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


def decode(jpeg):
    """A complete baseline JPEG (three components, 2x2 / 1x1 / 1x1, one interleaved scan) -> dict: coef int64 [6 M, 64] (the layout of `oracle`), width,
    height, qt [2, 64], ri, rst (the n of every RSTn in order), segments, scan (first byte, one past the last byte of entropy-coded data and markers)."""
    assert jpeg[:2] == b"\xff\xd8", "SOI"
    i, qt, huff, ri, W, H = 2, {}, {}, 0, None, None
    while True:
        assert jpeg[i] == 0xFF, f"marker expected at {i}"
        m, ln = jpeg[i + 1], struct.unpack(">H", jpeg[i + 2:i + 4])[0]
        seg = jpeg[i + 4:i + 2 + ln]
        i += 2 + ln
        if m == 0xDB:
            assert seg[0] >> 4 == 0, "8-bit quantiser tables"
            qt[seg[0] & 15] = np.array(list(seg[1:65]), dtype=np.int64)
        elif m == 0xC0:
            prec, H, W, nc = struct.unpack(">BHHB", seg[:6])
            assert prec == 8 and nc == 3 and list(seg[6:15]) == [1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1], "SOF0: 8 bit, Y 2x2 / Cb 1x1 / Cr 1x1"
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                n = sum(seg[p + 1:p + 17])
                huff[seg[p]] = _huff_decoder(list(seg[p + 1:p + 17]), list(seg[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xDD:
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xDA:
            assert list(seg) == [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0], "SOS: one interleaved scan, tables 0 / 1 / 1"
            break
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, f"unexpected marker {m:#x}"
    start = i
    # split at the markers: inside entropy-coded data 0xFF is followed by 0x00 (a stuffed byte), by D0 .. D7 (RSTn) or by D9 (EOI)
    parts, rst, cur = [], [], bytearray()
    while True:
        b = jpeg[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nxt = jpeg[i + 1]
        if nxt == 0:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= nxt <= 0xD7:
            parts.append(bytes(cur))
            rst.append(nxt - 0xD0)
            cur = bytearray()
            i += 2
        else:
            assert nxt == 0xD9 and i + 2 == len(jpeg), "EOI ends the file"
            parts.append(bytes(cur))
            break
    mcux, mcuy = (W + 15) // 16, (H + 15) // 16
    nm = mcux * mcuy
    per = ri if ri else nm
    assert len(parts) == (nm + per - 1) // per, "one segment per restart interval"
    coef = np.zeros((6 * nm, 64), dtype=np.int64)
    mcu = 0
    for part in parts:
        br, pred = _Bits(part), [0, 0, 0]
        for _ in range(min(per, nm - mcu)):
            mx, my = mcu % mcux, mcu // mcux
            for b in range(6):
                c = 0 if b < 4 else b - 3
                idx = (2 * my + (b >> 1)) * (2 * mcux) + 2 * mx + (b & 1) if b < 4 else (4 + c - 1) * nm + mcu
                s = _symbol(br, huff[0x00 | (c > 0)])
                assert s <= 11
                pred[c] += _extend(br.bits(s), s)
                coef[idx, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = _symbol(br, huff[0x10 | (c > 0)])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            assert r == 0, "EOBn belongs to progressive scans"
                            break
                        k += 16
                        continue
                    k += r
                    assert k < 64 and s <= 10, "run past the block"
                    coef[idx, k] = _extend(br.bits(s), s)
                    k += 1
            mcu += 1
        left = br.n - br.pos
        assert left < 8 and br.bits(left) == (1 << left) - 1, "a segment's last byte is padded with 1-bits, fewer than eight"
    assert mcu == nm
    return dict(coef=coef, width=W, height=H, qt=np.stack([qt[0], qt[1]]), ri=ri, rst=rst, segments=len(parts), scan=(start, len(jpeg) - 2))


def read_avi(path):
    """Walk an AVI 1.0 file -> dict(avih [14 dwords], strh (fccType, fccHandler, fields), strf, frames [(offset of the chunk header from the `movi` fourcc,
    size, bytes)], idx [(ckid, flags, offset, size)], riff_size, file_size, odd_padded: every odd-sized chunk was followed by a pad byte)."""
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:12] == b"AVI "
    out = dict(riff_size=struct.unpack("<I", d[4:8])[0], file_size=len(d), frames=[], idx=[])

    def walk(lo, hi):
        p = lo
        while p < hi:
            cc, n = d[p:p + 4], struct.unpack("<I", d[p + 4:p + 8])[0]
            body = p + 8
            if cc == b"LIST":
                kind = d[body:body + 4]
                if kind == b"movi":
                    out["movi"] = body
                    q = body + 4
                    while q < body + n:
                        c2, n2 = d[q:q + 4], struct.unpack("<I", d[q + 4:q + 8])[0]
                        assert c2 == b"00dc"
                        out["frames"].append((q - body, n2, d[q + 8:q + 8 + n2]))
                        q += 8 + n2 + (n2 & 1)
                    assert q == body + n, "the movi list ends with its last chunk"
                else:
                    walk(body + 4, body + n)
            elif cc == b"avih":
                out["avih"] = struct.unpack("<14I", d[body:body + n])
            elif cc == b"strh":
                out["strh"] = (d[body:body + 4], d[body + 4:body + 8]) + struct.unpack("<IHHIIIIIIiI4H", d[body + 8:body + n])
            elif cc == b"strf":
                out["strf"] = struct.unpack("<IiiHH4sIiiII", d[body:body + n])
            elif cc == b"idx1":
                out["idx"] = [struct.unpack("<4sIII", d[body + 16 * k:body + 16 * k + 16]) for k in range(n // 16)]
            p = body + n + (n & 1)
        assert p == hi
    walk(12, len(d))
    return out


def check_avi(path, width, height, fps, frames):
    """Every header field, count, offset and size of an AviWriter file; -> the frames' bytes."""
    a = read_avi(path)
    assert a["riff_size"] == a["file_size"] - 8
    h = a["avih"]
    assert h[0] == round(1e6 / fps) and h[3] & 0x10 and h[4] == frames and h[6] == 1 and (h[8], h[9]) == (width, height)
    s = a["strh"]
    assert s[0] == b"vids" and s[1] == b"MJPG" and (s[6], s[7]) == (1, fps) and s[9] == frames and tuple(s[-2:]) == (width, height)
    f = a["strf"]
    assert f[0] == 40 and (f[1], f[2], f[3], f[4], f[5]) == (width, height, 1, 24, b"MJPG")
    assert len(a["frames"]) == len(a["idx"]) == frames
    for (off, n, _), (ck, flags, ioff, isz) in zip(a["frames"], a["idx"]):
        assert ck == b"00dc" and flags & 0x10 and (ioff, isz) == (off, n) and off % 2 == 0
    assert h[7] == s[10] == max(n for _, n, _ in a["frames"])
    return [b for _, _, b in a["frames"]]


# ---------------------------------------------------------------------------------------------------------------- images
def scene(W, H):
    """Flat-shaded and render-like: a constant sky, a checker ground, shaded discs."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.empty((H, W, 3), dtype=np.float64)
    img[:] = (158, 191, 230)
    ground = y >= H * 0.55
    check = ((x // max(2, W // 6) + y // max(2, H // 8)) % 2).astype(bool)
    img[ground & check] = (204, 204, 194)
    img[ground & ~check] = (148, 153, 158)
    for cx, cy, r, col in ((0.3, 0.4, 0.18, (230, 140, 77)), (0.62, 0.5, 0.12, (77, 140, 217)), (0.5, 0.75, 0.1, (90, 190, 115))):
        d2 = ((x - cx * W) ** 2 + (y - cy * H) ** 2) / (r * min(W, H)) ** 2
        inside = d2 < 1
        shade = 0.35 + 0.65 * np.sqrt(np.clip(1 - d2, 0, 1))
        img[inside] = (np.array(col)[None, :] * shade[inside][:, None])
    return np.floor(img + 0.5).astype(np.uint8)


def gradient(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([255 * x / max(W - 1, 1), 255 * y / max(H - 1, 1), 255 * (x + y) / max(W + H - 2, 1)], axis=-1).astype(np.uint8)


def noise(W, H, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _from_coefficient(k, amplitude):
    """An 8 x 8 grey block whose only large DCT coefficient sits at zigzag position k."""
    S = np.zeros(64)
    S[zigzag()[k]] = amplitude
    m = dct_matrix()
    return np.clip(np.floor(m.T @ S.reshape(8, 8) @ m + 128.5), 0, 255)


def constructed(kind):
    """32 x 16 images (two MCUs) for the coder's branches -> rgb uint8."""
    g = np.full((16, 32), 128.0)
    if kind == "zrl":            # one coefficient far down the zigzag: a run of 39 zeros in front of it
        g[0:8, 0:8] = _from_coefficient(40, 300.0)
    elif kind == "coef63":       # the last coefficient non-zero: the block ends without EOB
        g[0:8, 8:16] = _from_coefficient(63, 400.0)
    elif kind == "dc_max":       # black and white flat blocks side by side at quality 100: DC differences of +-2040, category 11
        g[:, :] = np.where((np.arange(32) // 8) % 2, 255.0, 0.0)[None, :]
    elif kind == "ac_max":       # saturated alternating pixels at quality 100: |S(7,7)| = 837, category 10
        y, x = np.mgrid[0:16, 0:32]
        g[:, :] = np.where((x + y) % 2, 255.0, 0.0)
    else:
        raise KeyError(kind)
    return np.repeat(g[..., None], 3, axis=2).astype(np.uint8)


def category(v):
    return int(abs(int(v))).bit_length()


def coder_facts(coef, W, H, ri):
    """What the oracle's coefficients make the coder do: longest zero run in front of a non-zero AC coefficient, whether a block has coefficient 63 non-zero,
    whether a block has no AC coefficient at all, the largest DC-difference and AC categories."""
    mcux, mcuy = (W + 15) // 16, (H + 15) // 16
    nm = mcux * mcuy
    run_max, dc_cat = 0, 0
    for blk in coef:
        nz = np.nonzero(blk[1:])[0]
        if len(nz):
            run_max = max(run_max, int(np.diff(np.concatenate([[-1], nz])).max()) - 1)
    per = min(ri, nm)
    for m0 in range(0, nm, per):
        pred = [0, 0, 0]
        for mcu in range(m0, min(m0 + per, nm)):
            mx, my = mcu % mcux, mcu // mcux
            for b in range(6):
                c = 0 if b < 4 else b - 3
                idx = (2 * my + (b >> 1)) * (2 * mcux) + 2 * mx + (b & 1) if b < 4 else (3 + c) * nm + mcu
                dc_cat = max(dc_cat, category(coef[idx, 0] - pred[c]))
                pred[c] = coef[idx, 0]
    return dict(run_max=run_max, coef63=bool((coef[:, 63] != 0).any()), zero_ac=bool((coef[:, 1:] == 0).all(axis=1).any()), dc_cat=dc_cat,
                ac_cat=max(category(v) for v in np.abs(coef[:, 1:]).max(axis=1)))


# name -> (image, quality, restart interval, the facts the oracle must show for it)
CASES = {
    "one_mcu": (lambda: scene(16, 16), 90, 2, {}),
    "edges_17x9": (lambda: noise(17, 9, 1), 50, 1, {}),
    "48x32_ri1": (lambda: scene(48, 32), 90, 1, {"zero_ac": True}),
    "48x32_ri2": (lambda: scene(48, 32), 90, 2, {}),
    "48x32_single": (lambda: scene(48, 32), 90, 1000, {}),
    "wrap_16x160": (lambda: gradient(16, 160), 50, 1, {}),
    "many_272x256": (lambda: scene(272, 256), 75, 1, {}),   # 1632 blocks and 272 segments: more than one workgroup in every pass, two tiles of the scan
    "q1": (lambda: noise(24, 24, 2), 1, 2, {}),
    "q50": (lambda: noise(24, 24, 2), 50, 2, {}),
    "q90": (lambda: noise(24, 24, 2), 90, 2, {}),
    "q100": (lambda: noise(24, 24, 2), 100, 2, {}),
    "zrl": (lambda: constructed("zrl"), 50, 2, {"run_min": 16}),
    "coef63": (lambda: constructed("coef63"), 50, 2, {"coef63": True}),
    "dc_max": (lambda: constructed("dc_max"), 100, 2, {"dc_cat": 11}),
    "ac_max": (lambda: constructed("ac_max"), 100, 2, {"ac_cat": 10}),
    "stuffed": (lambda: noise(32, 32, 3), 100, 2, {"stuffed": True}),
}


def rgba_of(rgb, alpha_seed=5):
    """RGBA with a random alpha plane (the encoder ignores it)."""
    a = np.random.default_rng(alpha_seed).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], axis=2))


def header(W, H, quality, ri):
    from phc_amd import video
    return video.jpeg_header(W, H, quality, ri)


def check_frame(name, rgb, quality, ri, scan, coef, expect=None):
    """One coded frame against oracles (a) and (b): `scan` the produced bytes, `coef` the produced coefficients [6 M, 64].  -> share of tie coefficients."""
    H, W = rgb.shape[:2]
    qt = qtables(quality)
    want, tie = oracle(rgb, qt)
    coef = np.asarray(coef, dtype=np.int64)
    assert coef.shape == want.shape, name
    assert tie.mean() <= 0.02, f"{name}: {tie.mean():.4f} of the coefficients are ties"
    bad = (coef != want) & ~tie
    assert not bad.any(), f"{name}: {int(bad.sum())} coefficients off a tie differ from the fp64 transform, first at {np.argwhere(bad)[0]}"
    assert np.abs(coef - want).max() <= 1, f"{name}: a tie coefficient is more than 1 from the oracle"
    jpeg = header(W, H, quality, ri) + scan + b"\xff\xd9"
    got = decode(jpeg)
    assert (got["width"], got["height"]) == (W, H) and (got["qt"] == qt).all(), name
    assert (got["coef"] == coef).all(), f"{name}: the stream does not decode to the coefficients it was coded from"
    nm = ((W + 15) // 16) * ((H + 15) // 16)
    nseg = (nm + min(ri, nm) - 1) // min(ri, nm)
    assert got["ri"] == min(ri, nm) and got["segments"] == nseg and got["rst"] == [i % 8 for i in range(nseg - 1)], name
    assert got["scan"] == (len(jpeg) - 2 - len(scan), len(jpeg) - 2), name
    facts = coder_facts(want, W, H, ri)
    for key, val in (expect or {}).items():
        if key == "run_min":
            assert facts["run_max"] >= val, f"{name}: the longest zero run is {facts['run_max']}"
        elif key == "stuffed":
            assert b"\xff\x00" in scan, f"{name}: no stuffed byte"
        else:
            assert facts[key] == val, f"{name}: {key} is {facts[key]}"
    return float(tie.mean())


# ---------------------------------------------------------------------------------------------------------------- callers
def _guarded(nbytes, align=16):
    buf = np.full(nbytes + 2 * PAD + align, GUARD, dtype=np.uint8)
    off = PAD + (-(buf.ctypes.data + PAD)) % align
    return buf, off


def _intact(buf, off, nbytes):
    return bool((buf[:off] == GUARD).all() and (buf[off + nbytes:] == GUARD).all())


def host_encode(rgba, quality, ri, want_coef=True, qt=None, row_pad=0):
    """The host build on rgba uint8 [F, H, W, 4] -> (scans, coef [F, 6 M, 64] or None, guards intact).  row_pad: extra bytes between rows (a multiple of 4)."""
    from phc_amd import _lib as L
    lib = shim()
    F, H, W = rgba.shape[:3]
    src = np.full((F, H, 4 * W + row_pad), 0x3C, dtype=np.uint8)
    src[:, :, :4 * W] = rgba.reshape(F, H, 4 * W)
    q = np.ascontiguousarray(qtables(quality) if qt is None else qt, dtype=np.uint8)
    nm = ((W + 15) // 16) * ((H + 15) // 16)
    bound, need = lib.jpeg_frame_bound_of(W, H, ri), lib.jpeg_scratch_bytes_of(F, W, H, ri)
    sizes = dict(out=F * bound, length=4 * F, coef=F * 6 * nm * 128, scratch=need)
    bufs = {k: _guarded(v) for k, v in sizes.items()}
    a = L.JpegArgs()
    a.num_frames, a.width, a.height, a.restart_interval = F, W, H, ri
    a.row_stride, a.frame_stride = src.strides[1], src.strides[0]
    a.rgba, a.qtab = src.ctypes.data, q.ctypes.data
    addr = {k: b.ctypes.data + off for k, (b, off) in bufs.items()}
    a.out, a.out_stride, a.length, a.coef = addr["out"], bound, addr["length"], addr["coef"] if want_coef else None
    a.scratch, a.scratch_bytes = addr["scratch"], need
    rc = lib.jpeg_encode_host(C.byref(a))
    assert rc == 0, rc
    view = lambda k, dt: bufs[k][0][bufs[k][1]:bufs[k][1] + sizes[k]].view(dt)
    n = view("length", np.int32)
    out = view("out", np.uint8)
    scans = [out[f * bound:f * bound + n[f]].tobytes() for f in range(F)]
    coef = view("coef", np.int16).reshape(F, 6 * nm, 64).copy() if want_coef else None
    return scans, coef, all(_intact(b, off, sizes[k]) for k, (b, off) in bufs.items())
