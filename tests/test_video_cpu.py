"""Video output without a GPU: the host build of phc_amd/csrc/phc_jpeg.h (tests/jpeg_shim.cpp) against the fp64 transform (a), the baseline entropy decoder (b)
(tests/video_util.py, both written from ISO/IEC 10918-1) and Pillow (c); the argument checks of the entry point; phc_amd/video.py's header and AVI writer; the
`render.format` / `render.quality` keys.  The same cases run on the device in tests/test_video_gpu.py."""
import ctypes as C
import io
import os
import struct
import types

import numpy as np
import pytest

import video_util as vu
import host_build


def _lib():
    from phc_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_symbols_struct_and_default_interval():
    L, lib = _lib()
    from phc_amd import video
    assert {"phc_jpeg_encode", "phc_jpeg_scratch_bytes", "phc_jpeg_frame_bound"} <= set(L.EXPORTED_SYMBOLS) and lib.phc_abi_version() == 37
    assert C.sizeof(L.JpegArgs) == vu.shim().jpeg_args_size()
    mcus = (640 // 16) * (480 // 16)
    assert 300 <= mcus // video.DEFAULT_RESTART_INTERVAL, "a 640 x 480 frame gives at least a few hundred segments"
    for w, h, ri, f in ((640, 480, 2, 3), (17, 9, 1, 1), (16, 160, 1000, 2)):   # the library and the host build size their buffers alike
        assert lib.phc_jpeg_frame_bound(w, h, ri) == vu.shim().jpeg_frame_bound_of(w, h, ri)
        assert lib.phc_jpeg_scratch_bytes(f, w, h, ri) == vu.shim().jpeg_scratch_bytes_of(f, w, h, ri)
    assert lib.phc_jpeg_frame_bound(0, 9, 1) == -1 and lib.phc_jpeg_scratch_bytes(-1, 16, 16, 1) == -1 and lib.phc_jpeg_frame_bound(16, 65536, 1) == -1


def test_worst_case_bound_follows_from_the_code_lengths():
    """22 bits of DC (the longest DC code + 11 extra bits), 26 per AC coefficient (the longest AC code + 10), 63 coefficients; a segment's slot is those bits in
    bytes, doubled for stuffing, + 2 for RSTn; a frame's bound is slots x segments."""
    from phc_amd import video
    longest = {t: max(i + 1 for i, n in enumerate(bits) if n) for t, bits, _ in video.HUFFMAN}
    per_block = max(longest[0x00], longest[0x01]) + 11 + 63 * (max(longest[0x10], longest[0x11]) + 10)
    assert per_block == 1660 == vu.shim().jpeg_block_max_bits()
    for w, h, ri in ((16, 16, 1), (48, 32, 2), (48, 32, 1000), (640, 480, 2)):
        nm = ((w + 15) // 16) * ((h + 15) // 16)
        per = min(ri, nm)
        assert vu.shim().jpeg_frame_bound_of(w, h, ri) == -(-nm // per) * (2 * -(-6 * per * per_block // 8) + 2)


def _annex_c(bits, vals):
    out, code, n = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[n]] = (code << 5) | ln
            code, n = code + 1, n + 1
        code <<= 1
    return out


def _pillow_tables(quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(vu.noise(32, 32)).save(b, "JPEG", quality=quality, subsampling=2)
    d, i, dqt, dht = b.getvalue(), 2, {}, {}
    while d[i + 1] != 0xDA:
        m, ln = d[i + 1], struct.unpack(">H", d[i + 2:i + 4])[0]
        seg, p = d[i + 4:i + 2 + ln], 0
        while m == 0xDB and p < len(seg):
            dqt[seg[p]] = list(seg[p + 1:p + 65])
            p += 65
        while m == 0xC4 and p < len(seg):
            n = sum(seg[p + 1:p + 17])
            dht[seg[p]] = (list(seg[p + 1:p + 17]), list(seg[p + 17:p + 17 + n]))
            p += 17 + n
        i += 2 + ln
    return dqt, dht


def test_tables_are_the_standards():
    """The Huffman tables the kernel codes with are the ones the header declares, and both are the ones Pillow (libjpeg) emits as its standard tables; the
    quantiser tables are libjpeg's for the same quality."""
    from phc_amd import video
    words = np.zeros(2 * 12 + 2 * 256, dtype=np.uint32)
    vu.shim().jpeg_huff_table(words.ctypes.data)
    native = {0x00: words[0:12], 0x01: words[12:24], 0x10: words[24:280], 0x11: words[280:536]}
    dqt, dht = _pillow_tables(75)
    for t, bits, vals in video.HUFFMAN:
        assert (list(bits), list(vals)) == dht[t]
        want = _annex_c(bits, list(vals))
        assert {s: int(w) for s, w in enumerate(native[t]) if w} == want
    for q in (1, 10, 49, 50, 75, 90, 100):
        assert (video.quant_tables(q) == vu.qtables(q)).all()
        dqt, _ = _pillow_tables(q)
        assert [list(r) for r in video.quant_tables(q)] == [dqt[0], dqt[1]]
    for bad in (0, 101):
        with pytest.raises(ValueError, match="render.quality"):
            video.quant_tables(bad)


# ---------------------------------------------------------------------------------------------------------------- transform and entropy stage
@pytest.mark.parametrize("quality", [50, 75, 90, 100])
def test_tie_share_of_the_oracle_stays_under_the_cap(quality):
    """Asserted on the oracle alone: coefficients the fp32 transform may round the other way are at most 2 % of an image's."""
    for img in (vu.scene(96, 64), vu.gradient(96, 64), vu.noise(96, 64)):
        _, tie = vu.oracle(img, vu.qtables(quality))
        print(quality, f"{tie.mean():.5f}")
        assert tie.mean() <= 0.02
    assert 1e-3 < vu.tie_tolerance() < 4e-3


@pytest.mark.parametrize("name", list(vu.CASES))
def test_host_build_matches_both_oracles(name):
    img, quality, ri, expect = vu.CASES[name]
    rgb = img()
    scans, coef, intact = vu.host_encode(vu.rgba_of(rgb)[None], quality, ri)
    assert intact, "guard bytes around out / length / coef / scratch"
    vu.check_frame(name, rgb, quality, ri, scans[0], coef[0], expect)


def test_frames_strides_and_the_nullable_output():
    """F = 3 distinct frames in one call give what three calls give; a padded row stride and coef = NULL change nothing; repeats are byte-identical."""
    imgs = [vu.scene(40, 24), vu.noise(40, 24, 7), vu.gradient(40, 24)]
    rgba = np.stack([vu.rgba_of(i, s) for s, i in enumerate(imgs)])
    scans, coef, intact = vu.host_encode(rgba, 90, 2)
    assert intact and len({len(s) for s in scans}) == 3
    for f in range(3):
        one, c1, ok = vu.host_encode(rgba[f:f + 1], 90, 2)
        assert ok and one[0] == scans[f] and (c1[0] == coef[f]).all()
        vu.check_frame(f"frame {f}", imgs[f], 90, 2, scans[f], coef[f])
    again, _, _ = vu.host_encode(rgba, 90, 2)
    padded, _, ok = vu.host_encode(rgba, 90, 2, row_pad=20)
    plain, none, ok2 = vu.host_encode(rgba, 90, 2, want_coef=False)
    assert again == scans and padded == scans and plain == scans and none is None and ok and ok2
    other_alpha, _, _ = vu.host_encode(np.stack([vu.rgba_of(i, 99) for i in imgs]), 90, 2)
    assert other_alpha == scans, "alpha is ignored"


def _valid_args(L, keep):
    """A complete, acceptable phc_jpeg_args_t over numpy buffers filled with a guard byte."""
    W, H, ri = 20, 12, 2
    lib = vu.shim()
    bound, need = lib.jpeg_frame_bound_of(W, H, ri), lib.jpeg_scratch_bytes_of(2, W, H, ri)
    b = dict(rgba=np.zeros((2, H, W, 4), np.uint8), q=np.ones(128, np.uint8), out=np.full(2 * bound, vu.GUARD, np.uint8), length=np.full(2, -7, np.int32),
             coef=np.full(2 * 12 * 64 + 8, -7, np.int16), scratch=np.full(need + 16, vu.GUARD, np.uint8))
    keep.append(b)
    a = L.JpegArgs()
    a.num_frames, a.width, a.height, a.restart_interval, a.row_stride, a.frame_stride = 2, W, H, ri, 4 * W, 4 * W * H
    al = lambda arr: arr.ctypes.data + (-arr.ctypes.data) % 16
    a.rgba, a.qtab, a.out, a.out_stride, a.length = b["rgba"].ctypes.data, b["q"].ctypes.data, b["out"].ctypes.data, bound, b["length"].ctypes.data
    a.coef, a.scratch, a.scratch_bytes = al(b["coef"]), al(b["scratch"]), need
    return a, b


EINVAL_CASES = {
    "rgba": lambda a, b: setattr(a, "rgba", None), "qtab": lambda a, b: setattr(a, "qtab", None), "out": lambda a, b: setattr(a, "out", None),
    "length": lambda a, b: setattr(a, "length", None), "scratch": lambda a, b: setattr(a, "scratch", None),
    "width 0": lambda a, b: setattr(a, "width", 0), "width 65536": lambda a, b: setattr(a, "width", 65536),
    "height 0": lambda a, b: setattr(a, "height", 0), "height 65536": lambda a, b: setattr(a, "height", 65536),
    "frames -1": lambda a, b: setattr(a, "num_frames", -1), "interval 0": lambda a, b: setattr(a, "restart_interval", 0),
    "quantiser 0": lambda a, b: b["q"].__setitem__(77, 0), "row stride": lambda a, b: setattr(a, "row_stride", 4 * 20 - 4),
    "odd row stride": lambda a, b: setattr(a, "row_stride", 4 * 20 + 2), "frame stride": lambda a, b: setattr(a, "frame_stride", 4 * 20 * 11),
    "capacity": lambda a, b: setattr(a, "out_stride", a.out_stride - 1), "scratch size": lambda a, b: setattr(a, "scratch_bytes", a.scratch_bytes - 1),
    "coef alignment": lambda a, b: setattr(a, "coef", a.coef + 2), "scratch alignment": lambda a, b: setattr(a, "scratch", a.scratch + 4),
}


@pytest.mark.parametrize("what", list(EINVAL_CASES))
def test_refused_arguments_touch_nothing(what):
    """PHC_EINVAL from the library's entry point (before any device work: this runs without a GPU) and from the host build, outputs untouched."""
    L, lib = _lib()
    keep = []
    for call in (lambda a: lib.phc_jpeg_encode(C.byref(a), None), lambda a: vu.shim().jpeg_encode_host(C.byref(a))):
        a, b = _valid_args(L, keep)
        assert vu.shim().jpeg_args_check_of(C.byref(a)) == 0
        EINVAL_CASES[what](a, b)
        assert call(a) == -1, what
        assert (b["out"] == vu.GUARD).all() and (b["length"] == -7).all() and (b["coef"] == -7).all() and (b["scratch"] == vu.GUARD).all()
    assert lib.phc_jpeg_encode(None, None) == -1


def test_no_frames_is_no_work_and_huge_frames_are_unsupported():
    L, lib = _lib()
    keep = []
    a, b = _valid_args(L, keep)
    a.num_frames = 0
    assert lib.phc_jpeg_encode(C.byref(a), None) == 0 and vu.shim().jpeg_encode_host(C.byref(a)) == 0
    assert (b["out"] == vu.GUARD).all() and (b["length"] == -7).all()
    a, b = _valid_args(L, keep)
    a.width = a.height = 65535
    a.row_stride, a.frame_stride, a.restart_interval = 4 * 65535, 4 * 65535 * 65535, 1
    assert lib.phc_jpeg_encode(C.byref(a), None) == -2, "a frame bound above 2^31 - 1"


def test_host_sanitizer_program():
    """tests/jpeg_asan_main.cpp (its own main; nothing is loaded into Python): the longest-coding inputs on heap arrays of exact size, under AddressSanitizer
    and UndefinedBehaviorSanitizer."""
    returncode, stdout, stderr = host_build.run_sanitized("jpeg_asan_main.cpp")
    print(stdout[-2000:], stderr[-4000:])
    assert returncode == 0 and "jpeg_asan: ok" in stdout


# ---------------------------------------------------------------------------------------------------------------- Pillow
def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_pillow_reads_every_case():
    from PIL import Image
    for name, (img, quality, ri, _) in vu.CASES.items():
        rgb = img()
        scans, _, _ = vu.host_encode(vu.rgba_of(rgb)[None], quality, ri, want_coef=False)
        im = Image.open(io.BytesIO(vu.header(rgb.shape[1], rgb.shape[0], quality, ri) + scans[0] + b"\xff\xd9"))
        im.load()
        assert im.size == (rgb.shape[1], rgb.shape[0]) and im.mode == "RGB", name


@pytest.mark.parametrize("quality", [50, 75, 90])
@pytest.mark.parametrize("image", ["scene", "gradient", "noise"])
def test_against_pillows_encoder(image, quality):
    """The same image through this encoder and through Pillow's (same quality, 4:2:0, standard Huffman tables), both decoded by Pillow: PSNR against the source
    at most 1 dB below Pillow's, size within 10 % of Pillow's.  One segment (an interval past the frame), so that the two streams differ in the DCT and colour
    rounding alone; what the default interval adds is measured in profiles/video/README.md.
    Qualities: the ones whose quantiser steps (>= 2 at quality 90) stand above the one difference of substance between the two pipelines -- libjpeg rounds the
    Y / Cb / Cr samples and the chroma means to 8 bits before its DCT, this encoder transforms them unrounded.  That rounding is noise of variance 1 / 12 per
    sample and, the transform being orthonormal, per coefficient.  At quality 100 every step is 1 and the noise itself is coded (|N(0, 0.29)| > 0.5 for 8 % of
    the coefficients), while half of a step of 2 is 3.4 sigma away (0.05 %), so at 100 the sizes compare the two sample precisions and not the two readings of the standard; profiles/video/README.md has those figures."""
    from PIL import Image
    rgb = getattr(vu, image)(160, 120)
    scans, _, _ = vu.host_encode(vu.rgba_of(rgb)[None], quality, 1 << 20, want_coef=False)
    ours = vu.header(160, 120, quality, 1 << 20) + scans[0] + b"\xff\xd9"
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=2)
    theirs = b.getvalue()
    p_ours, p_theirs = (_psnr(np.asarray(Image.open(io.BytesIO(d)).convert("RGB")), rgb) for d in (ours, theirs))
    print(image, quality, f"PSNR {p_ours:.2f} / {p_theirs:.2f} dB, {len(ours)} / {len(theirs)} bytes")
    assert p_ours >= p_theirs - 1.0
    assert abs(len(ours) - len(theirs)) <= 0.10 * len(theirs)


# ---------------------------------------------------------------------------------------------------------------- container and keys
def _tiny_jpegs(n, W=20, H=12):
    out = []
    for k in range(n):
        scans, _, _ = vu.host_encode(vu.rgba_of(vu.noise(W, H, k))[None], 75, 2, want_coef=False)
        out.append(vu.header(W, H, 75, 2) + scans[0] + b"\xff\xd9")
    return out


def test_avi_writer_alone(tmp_path):
    from phc_amd import video
    frames = _tiny_jpegs(5)
    assert any(len(f) % 2 for f in frames) and any(len(f) % 2 == 0 for f in frames), "odd and even chunk sizes both occur"
    w = video.AviWriter(str(tmp_path / "a.avi"), 20, 12, 30)
    for f in frames:
        w.add(f)
    w.close()
    w.close()
    assert w.paths == [str(tmp_path / "a.avi")] and w.frames == 5
    assert vu.check_avi(w.paths[0], 20, 12, 30, 5) == frames
    for f in frames:
        assert vu.decode(f)["width"] == 20
    with pytest.raises(ValueError):
        video.AviWriter(str(tmp_path / "b.avi"), 20, 12, 0)


def test_avi_rolls_over_to_a_second_part(tmp_path):
    from phc_amd import video
    frames = _tiny_jpegs(7)
    limit = 224 + 3 * (max(len(f) for f in frames) + 9 + 16) + 8      # header + room for three of the largest chunks with their index entries
    w = video.AviWriter(str(tmp_path / "roll.avi"), 20, 12, 25, part_bytes=limit)
    for f in frames:
        w.add(f)
    w.close()
    assert len(w.paths) >= 2 and w.paths[1] == str(tmp_path / "roll-part02.avi")
    got = []
    for p in w.paths:
        assert os.path.getsize(p) <= limit
        n = len(vu.read_avi(p)["frames"])
        got += vu.check_avi(p, 20, 12, 25, n)
    assert got == frames


def test_header_layout():
    from phc_amd import video
    h = video.jpeg_header(17, 9, 50, 5)
    marks, i = [], 2
    while i < len(h):
        marks.append(h[i + 1])
        i += 2 + struct.unpack(">H", h[i + 2:i + 4])[0]
    assert h[:2] == b"\xff\xd8" and marks == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA] and i == len(h)
    assert h[6:11] == b"JFIF\0"
    assert video.jpeg_header(17, 9, 50, 5)[-14 - 6:-14] == b"\xff\xdd\x00\x04\x00\x02", "DRI: an interval past the frame's two MCUs is the frame"
    for bad in ((0, 9, 50, 1), (17, 65536, 50, 1), (17, 9, 0, 1), (17, 9, 50, 0)):
        with pytest.raises(ValueError):
            video.jpeg_header(*bad)


def test_format_and_quality_keys(tmp_path):
    from phc_amd import render as R
    assert R.video_options({}) == ("png", 90) and R.video_options({"format": "both", "quality": 35}) == ("both", 35)
    with pytest.raises(ValueError, match="render.format"):
        R.video_options({"format": "gif"})
    for q in (0, 101):
        with pytest.raises(ValueError, match="render.quality"):
            R.video_options({"quality": q})
    task = types.SimpleNamespace(device="cpu", num_envs=2)
    for fmt in ("avi", "both"):
        with pytest.raises(RuntimeError, match="HIP device"):
            R.TaskRecorder(task, {"video": str(tmp_path / "v"), "format": fmt})
        rec = R.VideoRecorder(str(tmp_path / fmt), fmt=fmt)
        with pytest.raises(RuntimeError, match="HIP device"):
            rec.add(np.zeros((12, 20, 4), np.uint8))
    with pytest.raises(ValueError, match="render.format"):
        R.TaskRecorder(task, {"video": str(tmp_path / "v"), "format": "mp4"})


def test_png_remains_the_default_byte_for_byte(tmp_path):
    from phc_amd import render as R
    img = vu.rgba_of(vu.scene(20, 12))
    rec = R.VideoRecorder(str(tmp_path / "rec"))
    rec.add(img)
    rec.close()
    R.write_png(str(tmp_path / "ref.png"), img)
    assert rec.fmt == "png" and rec.avi_path is None and os.listdir(tmp_path / "rec") == ["frame_000000.png"]
    assert open(tmp_path / "rec" / "frame_000000.png", "rb").read() == open(tmp_path / "ref.png", "rb").read()
