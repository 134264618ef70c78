"""Frame pipelines (C ABI section 6): sequences of same-shaped frames with the PCIe copies, the kernels
and the host Tier-2 of consecutive frames overlapped.  Mirrors how one ojph::codestream object is re-used
through restart() for the frames of a sequence (ojph_codestream.h:204): the caller writes samples into
memory the library hands out and receives finished codestreams -- or the other way round -- `depth`
frames in flight.  Plumbing only: ctypes views of the pipe's pinned host memory, no arithmetic here.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import capi
from .capi import check
from .plan import Plan, make_params


_CONTAINER = {8: np.uint8, 16: np.uint16, 32: np.int32}      # numpy view of a frame slot by container width


def _view(ptr, nbytes):
    return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8)


def _frame_view(pipe, ptr, nbytes):
    """numpy view of a pinned frame in the pipe's current hand-over"""
    raw = _view(ptr, nbytes)
    if pipe.packed:                                   # one bit string
        return raw
    if pipe.video:                                    # [H, row_bytes] (4:2:2, 4:4:4); 4:2:0: [H + ch, row_bytes], the chroma plane's rows behind the luma plane's
        h = pipe.plan.comp_info(0)["h"]
        rows = h + (h + 1) // 2 if pipe.video in VIDEO420_FORMATS else h
        return raw.reshape(rows, nbytes // rows)
    if pipe.pixels is not None:                       # [H,W,C] in the file's sample type (big endian: the raw bytes)
        c, h, w = pipe.plan.frame_shape
        dt = np.uint8 if pipe.pixels[0] == 8 else np.dtype(">u2" if pipe.pixels[1] else "<u2")
        return raw.view(dt).reshape(h, w, c)
    return raw.view(_CONTAINER[pipe.container]).reshape(pipe.plan.frame_shape)


class _Handover:
    """The hand-over setters of both pipes (ojphgpu_{enc,dec}_pipe_set_pixels / _set_packed / _set_video; None or 0: planes
    again): before the first acquire() of an encoder pipe / submit() of a decoder pipe, repeatable until then, one kind at a
    time.  A refusal raises OjphError (capi.E_INVALID) and leaves the pipe as it was."""
    pixels = packed = video = colour = chroma = None

    def _set(self, kind, *args):
        name = "%s_pipe_set_%s" % (self._side, kind)
        check(getattr(self._lib, "ojphgpu_" + name)(self._h, *args), name)

    def set_pixels(self, bits, big_endian=False):
        self._set("pixels", int(bits or 0), int(bool(big_endian)))
        self.pixels = (int(bits), bool(big_endian)) if bits else None

    def set_packed(self, bits):
        self._set("packed", int(bits or 0))
        self.packed = int(bits) if bits else None

    def set_video(self, fmt):
        """judged on the pipe's plan (a view's: the view's; a region with odd x0 is refused): three unsigned components of
        one depth the format holds, the chroma half as wide -- and, for the 4:2:0 names of VIDEO420_FORMATS, half as high (a
        region with odd y0 is refused too); for the 4:4:4 names of VIDEO444_FORMATS all three of one size, a region at any
        origin"""
        self._set("video", _video_code(self.plan, fmt, "%s_pipe_set_video" % self._side))
        self.video = fmt

    def set_video_colour(self, fmt, colour):
        """the buffer holds R, G, B (fmt = "bgra" | "rgba" | "argb" | "r210" | "r10k"), the plan Y, Cb, Cr 4:4:4, 4:2:2 or 4:2:0:
        colour = a standard's name ("bt601" | "bt709" | "bt2020": full-range RGB of the plan's depth, narrow-range YCbCr) or a
        Colour; the matrix, the ranges, the change of depth and the chroma filter run on the device between the buffer and the
        planes (ojphgpu_{enc,dec}_pipe_set_video_colour; ojphgpu.h section 7e).  Excludes set_video; fmt None: planes again"""
        spec = _colour_spec(colour)
        self._set("video_colour", _video_code(self.plan, fmt, "%s_pipe_set_video_colour" % self._side), C.byref(spec))
        self.video = fmt
        self.colour = (colour if isinstance(colour, Colour) else Colour(colour)) if fmt else None

    def set_video_chroma(self, fmt, mode="cosited"):
        """the buffer holds Y, Cb, Cr in the chroma format of fmt (any name of the three families but the five RGB ones), the plan
        in its own -- 4:4:4, 4:2:2, 4:2:0 or 4:4:0: chroma is halved (taps (1, 2, 1), cosited) or doubled (linear) on the device
        between the buffer and the planes, as rechroma_frame states it (ojphgpu_{enc,dec}_pipe_set_video_chroma; ojphgpu.h section
        7f).  Equal cells: exactly set_video.  Excludes set_video and set_video_colour; fmt None: planes again"""
        if mode not in capi.CHROMA:
            raise ValueError("chroma mode %r: one of %s" % (mode, ", ".join(sorted(capi.CHROMA))))
        self._set("video_chroma", _video_code(self.plan, fmt, "%s_pipe_set_video_chroma" % self._side), capi.CHROMA[mode])
        self.video = fmt
        self.chroma = mode if fmt else None


def pack_bits(samples, bits):
    """numpy: unsigned samples (any shape, flattened in C order) -> the little-endian bit string ojphgpu_unpack_bits
    reads (sample i = bits [i * bits, (i + 1) * bits)), padded to a whole group of 32 samples"""
    v = np.ascontiguousarray(samples).reshape(-1)
    n = v.size
    pad = (-n) % 32
    if bits == 12:                                    # two samples in three bytes, without the bit matrix
        a = np.zeros(n + pad, np.uint16); a[:n] = v
        lo, hi = a[0::2], a[1::2]
        out = np.empty((lo.size, 3), np.uint8)
        out[:, 0] = lo & 0xFF; out[:, 1] = (lo >> 8) | ((hi & 0xF) << 4); out[:, 2] = hi >> 4
        return out.reshape(-1)
    v = v.astype(np.uint64)
    if pad:
        v = np.concatenate([v, np.zeros(pad, np.uint64)])
    b = ((v[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & 1).astype(np.uint8)       # LSB first
    return np.packbits(b.reshape(-1), bitorder="little")


def unpack_bits(packed, bits, n):
    """numpy inverse of pack_bits: -> n samples (uint32)"""
    b = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8), bitorder="little")[: n * bits].reshape(n, bits).astype(np.uint32)
    return (b << np.arange(bits, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)


# The video formats (ojphgpu.h sections 7b - 7d), the one table of this side (csrc/video_formats.h is the library's): name ->
# (OJPHGPU_VIDEO_* constant, family, the depth the name fixes or None, lowest and highest depth of the column, the depth taken
# when none is given or None: one must be, bytes per unit of pixels: row_bytes = unit_bytes * ceil(width / unit_pixels))
_VIDEO_TABLE = {
    "uyvy": (0x01, 422, None, 1, 8, None, 4, 2), "yuy2": (0x02, 422, None, 1, 8, None, 4, 2), "v210": (0x03, 422, None, 1, 10, None, 128, 48),
    "y2xx": (0x04, 422, None, 9, 16, None, 8, 2), "y210": (0x04, 422, 10, 9, 16, 10, 8, 2), "y212": (0x04, 422, 12, 9, 16, 12, 8, 2),
    "y216": (0x04, 422, 16, 9, 16, 16, 8, 2),
    "nv12": (0x11, 420, None, 1, 8, 8, 2, 2), "nv21": (0x12, 420, None, 1, 8, 8, 2, 2), "p0xx": (0x13, 420, None, 9, 16, None, 4, 2),
    "p010": (0x13, 420, 10, 9, 16, 10, 4, 2), "p012": (0x13, 420, 12, 9, 16, 12, 4, 2), "p016": (0x13, 420, 16, 9, 16, 16, 4, 2),
    "v410": (0x21, 444, None, 1, 10, 10, 4, 1), "y410": (0x22, 444, None, 1, 10, 10, 4, 1), "r210": (0x23, 444, None, 1, 10, 10, 4, 1),
    "r10k": (0x24, 444, None, 1, 10, 10, 4, 1), "y4xx": (0x25, 444, None, 9, 16, 16, 8, 1), "y412": (0x25, 444, 12, 9, 16, 12, 8, 1),
    "y416": (0x25, 444, 16, 9, 16, 16, 8, 1), "ayuv": (0x26, 444, None, 1, 8, 8, 4, 1), "bgra": (0x27, 444, None, 1, 8, 8, 4, 1),
    "rgba": (0x28, 444, None, 1, 8, 8, 4, 1), "argb": (0x29, 444, None, 1, 8, 8, 4, 1),
}
# a family's names -> (OJPHGPU_VIDEO_* constant, the depth the name fixes or None)
VIDEO_FORMATS, VIDEO420_FORMATS, VIDEO444_FORMATS = ({n: (t[0], t[2]) for n, t in _VIDEO_TABLE.items() if t[1] == family} for family in (422, 420, 444))


def _entry(family, fmt):                              # a name's row of the table; family 0: any
    t = _VIDEO_TABLE.get(fmt)
    if t is None or family not in (0, t[1]):
        raise ValueError("video format %r: one of %s" % (fmt, ", ".join(sorted(n for n, u in _VIDEO_TABLE.items() if family in (0, u[1])))))
    return t


def _format(family, fmt, bit_depth):
    """-> (OJPHGPU_VIDEO_* constant, bit depth); refused: a depth outside the format's column or not the one the name fixes"""
    code, _, fixed, lo, hi, default, _, _ = _entry(family, fmt)
    if bit_depth is None and default is None:
        raise ValueError("video format %r needs a bit depth" % fmt)
    b = int(default if bit_depth is None else bit_depth)
    if not lo <= b <= hi or (fixed is not None and b != fixed):
        raise ValueError("video format %r does not hold %d-bit samples" % (fmt, b))
    return code, b


def _layout(family, fmt, width, height):
    """-> (row_bytes, chroma_offset, frame_bytes) of the tight layout; chroma_offset 0 where there is no second plane"""
    unit_bytes, unit_pixels = _entry(family, fmt)[6:]
    if width < 1 or height < 1:
        raise ValueError("video layout: a frame has at least one sample")
    row = unit_bytes * (-(-int(width) // unit_pixels))
    ch = (int(height) + 1) // 2 if family == 420 else 0
    return row, row * int(height) if ch else 0, row * (int(height) + ch)


def video_format(fmt, bit_depth):
    """-> (OJPHGPU_VIDEO_* constant, bit depth) of a 4:2:2 name and a depth of its column; a name that fixes no depth needs one"""
    return _format(422, fmt, bit_depth)


def video420_format(fmt, bit_depth):
    """... of a 4:2:0 name; without a depth: the one the name fixes, nv12 / nv21: 8, p0xx needs one"""
    return _format(420, fmt, bit_depth)


def video444_format(fmt, bit_depth):
    """... of a 4:4:4 name; without a depth: the one the name fixes, else the widest of the column"""
    return _format(444, fmt, bit_depth)


def video_layout(fmt, width, height):
    """-> (row_bytes, frame_bytes) of a width x height frame, as ojphgpu_video_layout"""
    return _layout(422, fmt, width, height)[::2]


def video420_layout(fmt, width, height):
    """-> (row_bytes, chroma_offset, frame_bytes), as ojphgpu_video420_layout: `height` luma rows, then ceil(height / 2) chroma rows"""
    return _layout(420, fmt, width, height)


def video444_layout(fmt, width, height):
    """-> (row_bytes, frame_bytes) of the tight layout of a width x height frame, as ojphgpu_video444_layout"""
    return _layout(444, fmt, width, height)[::2]


def _video_code(plan, fmt, what):
    """the constant a pipe's _set_video takes for a format name (None: 0, planes); a name that fixes a depth the plan's
    samples do not have is refused here as the library refuses the rest"""
    if fmt is None:
        return 0
    code, _, fixed = _entry(0, fmt)[:3]
    if fixed is not None and plan.comp_format(0)[0] != fixed:
        raise capi.OjphError(capi.E_INVALID, "%s: %r on %d-bit samples" % (what, fmt, plan.comp_format(0)[0]))
    return code


def pack_video(planes, fmt, bit_depth=None):
    """numpy: planes = [Y [H,W], Cb [H,cw], Cr [H,cw]] (cw = ceil(W / 2)) -> the frame as one 4:2:2 video buffer, uint8
    [H, row_bytes]: the host-side statement of ojphgpu_pack_video.  Samples are clamped to [0, 2^bit_depth - 1]; padding
    (the second luma of an odd row's last pair, the fields and groups a v210 row is padded with, bits 30-31 of a v210 dword,
    the low bits of a Y2XX word) is zero."""
    code, b = video_format(fmt, bit_depth)
    y, cb, cr = [np.clip(np.asarray(p).astype(np.int64), 0, (1 << b) - 1) for p in planes]
    h, w = y.shape
    cw = (w + 1) // 2
    if cb.shape != (h, cw) or cr.shape != (h, cw):
        raise ValueError("pack_video: chroma planes of %s, not %s" % (cb.shape, (h, cw)))
    np_ = 24 * ((w + 47) // 48) if code == 3 else cw          # pairs of a row, with the padding of v210
    f = np.zeros((h, np_, 4), np.int64)                        # the pairs as Y0 Y1 Cb Cr
    f[:, :cw, 0][:, : (w + 1) // 2] = y[:, 0::2]
    f[:, : w // 2, 1] = y[:, 1::2]
    f[:, :cw, 2], f[:, :cw, 3] = cb, cr
    if code in (1, 2):
        return f[:, :, [2, 0, 3, 1] if code == 1 else [0, 2, 1, 3]].astype(np.uint8).reshape(h, 4 * cw)
    if code == 4:
        return np.ascontiguousarray((f[:, :, [0, 2, 1, 3]] << (16 - b)).astype("<u2")).view(np.uint8).reshape(h, 8 * cw)
    t = f[:, :, [2, 0, 3, 1]].reshape(h, np_ * 4 // 3, 3)      # v210: the fields in order Cb Y0 Cr Y1, three to a dword
    return np.ascontiguousarray((t[:, :, 0] | t[:, :, 1] << 10 | t[:, :, 2] << 20).astype("<u4")).view(np.uint8).reshape(h, -1)


def unpack_video(buf, fmt, width, height, bit_depth=None):
    """numpy inverse of pack_video: the bytes of a 4:2:2 video buffer -> [Y [H,W], Cb [H,cw], Cr [H,cw]] (uint16).  A sample
    is its field (Y2XX: word >> (16 - bit_depth)); padding is not looked at and no value is range-checked."""
    code, b = video_format(fmt, bit_depth)
    w, h = int(width), int(height)
    cw = (w + 1) // 2
    row, total = video_layout(fmt, w, h)
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if raw.size != total:
        raise ValueError("unpack_video: %d bytes, the frame has %d" % (raw.size, total))
    raw = raw.reshape(h, row)
    if code in (1, 2):
        f = raw.reshape(h, cw, 4)[:, :, [1, 3, 0, 2] if code == 1 else [0, 2, 1, 3]].astype(np.uint16)
    elif code == 4:
        f = (raw.view("<u2").reshape(h, cw, 4)[:, :, [0, 2, 1, 3]] >> (16 - b)).astype(np.uint16)
    else:
        d = raw.view("<u4")
        t = np.stack([d & 0x3FF, (d >> 10) & 0x3FF, (d >> 20) & 0x3FF], axis=2).reshape(h, -1, 4)   # pairs as Cb Y0 Cr Y1
        f = t[:, :cw, [1, 3, 0, 2]].astype(np.uint16)
    y = f[:, :, :2].reshape(h, 2 * cw)[:, :w]
    return [np.ascontiguousarray(y), np.ascontiguousarray(f[:, :, 2]), np.ascontiguousarray(f[:, :, 3])]


def pack_video420(planes, fmt, bit_depth=None):
    """numpy: planes = [Y [H,W], Cb [ch,cw], Cr [ch,cw]] (cw = ceil(W / 2), ch = ceil(H / 2)) -> the frame as one 4:2:0 video
    buffer in the tight layout, uint8 [H + ch, row_bytes]: H luma rows, then ch rows of (Cb, Cr) pairs (nv21: (Cr, Cb)): the
    host-side statement of ojphgpu_pack_video420.  Samples are clamped to [0, 2^bit_depth - 1]; padding (the sample behind an
    odd luma row, the low bits of a P0XX word) is zero."""
    code, b = video420_format(fmt, bit_depth)
    y, cb, cr = [np.clip(np.asarray(p).astype(np.int64), 0, (1 << b) - 1) for p in planes]
    if y.ndim != 2 or y.size == 0:
        raise ValueError("pack_video420: the luma plane is [H, W]")
    h, w = y.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if cb.shape != (ch, cw) or cr.shape != (ch, cw):
        raise ValueError("pack_video420: chroma planes of %s and %s, not %s" % (cb.shape, cr.shape, (ch, cw)))
    f = np.zeros((h + ch, 2 * cw), np.int64)
    f[:h, :w] = y
    f[h:, 0::2], f[h:, 1::2] = (cr, cb) if code == 0x12 else (cb, cr)
    if code == 0x13:
        return np.ascontiguousarray((f << (16 - b)).astype("<u2")).view(np.uint8).reshape(h + ch, 4 * cw)
    return f.astype(np.uint8)


def unpack_video420(buf, fmt, width, height, bit_depth=None):
    """numpy inverse of pack_video420: the bytes of a 4:2:0 video buffer in the tight layout -> [Y [H,W], Cb [ch,cw], Cr
    [ch,cw]] (uint16).  A sample is its element (P0XX: word >> (16 - bit_depth)); padding is not looked at and no value is
    range-checked."""
    code, b = video420_format(fmt, bit_depth)
    w, h = int(width), int(height)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    row, _, total = video420_layout(fmt, w, h)
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if raw.size != total:
        raise ValueError("unpack_video420: %d bytes, the frame has %d" % (raw.size, total))
    raw = raw.reshape(h + ch, row)
    f = (raw.view("<u2") >> (16 - b)).astype(np.uint16) if code == 0x13 else raw.astype(np.uint16)
    c0, c1 = f[h:, 0::2], f[h:, 1::2]
    cb, cr = (c1, c0) if code == 0x12 else (c0, c1)
    return [np.ascontiguousarray(f[:h, :w]), np.ascontiguousarray(cb), np.ascontiguousarray(cr)]


# 4:4:4 packed video (ojphgpu.h section 7d), one interleaved word per pixel: the bit layouts of the numpy pair below.
# The 10-bit dword formats: constant -> (dword byte order, first bit of component 0, 1, 2, the constant bits).  v410 and Y410
# name Cb (component 1) first, R210 and R10k carry R (component 0) on top
_VIDEO444_DWORD = {0x21: ("<u4", (12, 2, 22), 0), 0x22: ("<u4", (10, 0, 20), 3 << 30), 0x23: (">u4", (20, 10, 0), 0), 0x24: (">u4", (22, 12, 2), 0)}
# the byte formats: constant -> the byte of component 0, 1, 2 and of alpha
_VIDEO444_BYTES = {0x26: (2, 1, 0, 3), 0x27: (2, 1, 0, 3), 0x28: (0, 1, 2, 3), 0x29: (1, 2, 3, 0)}


def pack_video444(planes, fmt, bit_depth=None):
    """numpy: planes = three [H,W] (Y, Cb, Cr or R, G, B, as the format names them) -> the frame as one 4:4:4 packed buffer in
    the tight layout, uint8 [H, row_bytes]: the host-side statement of ojphgpu_pack_video444.  Samples are clamped to [0,
    2^bit_depth - 1]; padding bits and the low bits of a Y4XX word are zero, alpha is opaque."""
    code, b = video444_format(fmt, bit_depth)
    if len(planes) != 3:
        raise ValueError("pack_video444: three planes")
    c = [np.clip(np.asarray(p).astype(np.int64), 0, (1 << b) - 1) for p in planes]
    if c[0].ndim != 2 or c[0].size == 0 or c[1].shape != c[0].shape or c[2].shape != c[0].shape:
        raise ValueError("pack_video444: three planes [H, W] of one size")
    h, w = c[0].shape
    if code in _VIDEO444_DWORD:
        order, at, const = _VIDEO444_DWORD[code]
        d = c[0] << at[0] | c[1] << at[1] | c[2] << at[2] | const
        return np.ascontiguousarray(d.astype(order)).view(np.uint8).reshape(h, 4 * w)
    if code == 0x25:                                           # words Cb, Y, Cr, A
        f = np.stack([c[1], c[0], c[2], np.full((h, w), (1 << b) - 1, np.int64)], axis=2) << (16 - b)
        return np.ascontiguousarray(f.astype("<u2")).view(np.uint8).reshape(h, 8 * w)
    f = np.zeros((h, w, 4), np.uint8)
    i0, i1, i2, ia = _VIDEO444_BYTES[code]
    f[:, :, i0], f[:, :, i1], f[:, :, i2], f[:, :, ia] = c[0], c[1], c[2], 0xFF
    return f.reshape(h, 4 * w)


def unpack_video444(buf, fmt, width, height, bit_depth=None):
    """numpy inverse of pack_video444: the bytes of a 4:4:4 packed buffer in the tight layout -> three [H,W] (uint16).  A
    sample is its field (Y4XX: word >> (16 - bit_depth)); padding and alpha are not looked at and no value is range-checked."""
    code, b = video444_format(fmt, bit_depth)
    w, h = int(width), int(height)
    row, total = video444_layout(fmt, w, h)
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if raw.size != total:
        raise ValueError("unpack_video444: %d bytes, the frame has %d" % (raw.size, total))
    raw = raw.reshape(h, row)
    if code in _VIDEO444_DWORD:
        order, at, _ = _VIDEO444_DWORD[code]
        d = raw.view(order).astype(np.uint32)
        return [np.ascontiguousarray(((d >> a) & 0x3FF).astype(np.uint16)) for a in at]
    if code == 0x25:
        f = raw.view("<u2").reshape(h, w, 4) >> (16 - b)
        return [np.ascontiguousarray(f[:, :, i].astype(np.uint16)) for i in (1, 0, 2)]
    f = raw.reshape(h, w, 4)
    return [np.ascontiguousarray(f[:, :, i].astype(np.uint16)) for i in _VIDEO444_BYTES[code][:3]]


def fit_container(out_depths):
    """the narrowest container an encoder takes for components of these depths: 8, 16 or 32 bits"""
    deepest = max(int(b) for b in out_depths)
    return 8 if deepest <= 8 else 16 if deepest <= 16 else 32


def fit_frame(planes, src_depths, out_depths, signs):
    """numpy statement of the recoder's fit (ojphgpu_frame_fit as codec.Recoder uses it; include/ojphgpu.h section 5e): the
    decoded planes of a source (any integer arrays; a sample may lie past its nominal range) -> the planes an encoder of the
    output depths takes.  Per component, s = source depth - output depth: (v + 2^(s - 1)) >> s for s > 0 (an arithmetic
    shift, round half up, in 64 bits), v << -s for s < 0, then the clamp to the output's nominal range -- always, also at
    s == 0.  Every plane comes back in the narrowest container the encoder takes for all of them (fit_container): int8 /
    int16 for a signed component, uint8 / uint16 otherwise, or int32."""
    bits = fit_container(out_depths)
    out = []
    for q, bs, bo, sg in zip(planes, src_depths, out_depths, signs):
        v, s, bo = np.asarray(q).astype(np.int64), int(bs) - int(bo), int(bo)
        if s > 0:
            v = (v + (1 << (s - 1))) >> s
        elif s < 0:
            v = v << -s
        lo, hi = (-(1 << (bo - 1)), (1 << (bo - 1)) - 1) if sg else (0, (1 << bo) - 1)
        dt = np.int32 if bits == 32 else np.dtype("%s%d" % ("i" if sg else "u", bits // 8))
        out.append(np.clip(v, lo, min(hi, 2 ** 31 - 1)).astype(dt))
    return out


def resample_plane(q, fx, fy, px=0, py=0):
    """numpy statement of the recoder's resampling (ojphgpu_frame_resample before its fit; include/ojphgpu.h section 5e): one
    plane halved where fx / fy is 2.  Output sample i of a halved direction stands ON source sample 2 i + p (p = the parity
    of the source component's origin on its own grid): taps (1, 2, 1) around it, indices clamped into the plane, summed
    exactly in 64 bits and rounded once -- (acc + 2^(k-1)) >> k with k = 2 per halved direction.  -> int64"""
    if fx not in (1, 2) or fy not in (1, 2) or px not in (0, 1) or py not in (0, 1):
        raise ValueError("resample_plane: factors are 1 or 2, phases 0 or 1")
    v = np.asarray(q).astype(np.int64)
    hs, ws = v.shape
    wo = (ws - px + 1) // 2 if fx == 2 else ws               # == ceil((xs0 + ws) / 2) - ceil(xs0 / 2); may be 0
    ho = (hs - py + 1) // 2 if fy == 2 else hs

    def taps(n, no, f, p):
        if f == 1:
            return [(np.arange(no), 1)]
        c = 2 * np.arange(no) + p                            # always < n
        return [(np.clip(c - 1, 0, n - 1), 1), (c, 2), (np.clip(c + 1, 0, n - 1), 1)]
    acc = np.zeros((ho, wo), np.int64)
    for iy, wy in taps(hs, ho, fy, py):
        for ix, wx in taps(ws, wo, fx, px):
            acc += wy * wx * v[np.ix_(iy, ix)]
    k = 2 * ((fx == 2) + (fy == 2))                          # 0, 2 or 4
    return (acc + (1 << (k - 1)) >> k) if k else acc


def resample_frame(planes, factors, phases=None):
    """resample_plane per component: factors = [(fx, fy), ...], phases = [(px, py), ...] (None: zeros)"""
    phases = [(0, 0)] * len(planes) if phases is None else phases
    return [resample_plane(q, fx, fy, px, py) for q, (fx, fy), (px, py) in zip(planes, factors, phases)]


def _rechroma_taps(n, no, s, d):
    """one direction of rechroma_plane: n source samples of factor s -> no outputs of factor d, as [(indices, weight), ...] and
    the bits the weights sum to"""
    x = np.arange(no)
    if s == d:
        return [(x, 1)], 0
    if d == 2 * s:                                    # resample_plane's taps at phase 0
        return [(np.clip(2 * x - 1, 0, n - 1), 1), (2 * x, 2), (np.clip(2 * x + 1, 0, n - 1), 1)], 2
    return [(x // 2, 1), (np.where(x & 1, np.minimum((x + 1) // 2, n - 1), x // 2), 1)], 1      # ycc_to_rgb's pair


def rechroma_plane(q, s, d, size=None):
    """numpy statement of ojphgpu_frame_rechroma on one chroma plane (include/ojphgpu.h section 7f): q [hs, ws] of the cell s =
    (sub_x, sub_y) -> the plane of the cell d, each factor 1 or 2.  Per direction: equal factors: the index as it is; d == 2 s
    (halved): output i stands ON source sample 2 i, taps (1, 2, 1), indices clamped into the plane, 2 bits -- resample_plane at
    phase 0; s == 2 d (doubled): 2 C[x / 2] for even x, C[(x - 1) / 2] + C[min((x + 1) / 2, n - 1)] for odd x, 1 bit -- ycc_to_rgb's
    rule.  The 2-D product of the two directions' taps, exact in 64 bits, rounded once: (acc + 2^(k-1)) >> k; k == 0 is a copy.
    No clamp: the weights are positive and sum to 2^k.  size = (w, h) of the luma plane: a plane of a cell (cx, cy) is ceil(w /
    cx) x ceil(h / cy) (None: a doubled direction gives twice the source's length).  -> int64"""
    (sx, sy), (dx, dy) = s, d
    if any(f not in (1, 2) for f in (sx, sy, dx, dy)):
        raise ValueError("rechroma_plane: cell factors are 1 or 2")
    v = np.asarray(q).astype(np.int64)
    if v.ndim != 2 or v.size == 0:
        raise ValueError("rechroma_plane: a plane is [H, W]")
    hs, ws = v.shape
    if size is None:
        size = (ws * sx, hs * sy)
    w, h = int(size[0]), int(size[1])
    if (-(-w // sx), -(-h // sy)) != (ws, hs):
        raise ValueError("rechroma_plane: a plane of %s, the cell %s of a %d x %d frame has %s" % ((hs, ws), (sx, sy), w, h, (-(-h // sy), -(-w // sx))))
    wo, ho = -(-w // dx), -(-h // dy)
    tx, kx = _rechroma_taps(ws, wo, sx, dx)
    ty, ky = _rechroma_taps(hs, ho, sy, dy)
    acc = np.zeros((ho, wo), np.int64)
    for iy, wy in ty:
        for ix, wx in tx:
            acc += wy * wx * v[np.ix_(iy, ix)]
    k = kx + ky
    return (acc + (1 << (k - 1)) >> k) if k else acc


def rechroma_frame(planes, src_cell, dst_cell):
    """planes = [Y [H, W], Cb, Cr of src_cell] -> [Y as it is, Cb, Cr of dst_cell] (int64): rechroma_plane per chroma plane"""
    y = np.asarray(planes[0]).astype(np.int64)
    if len(planes) != 3 or y.ndim != 2 or y.size == 0:
        raise ValueError("rechroma_frame: three planes, the luma plane [H, W]")
    size = (y.shape[1], y.shape[0])
    return [y] + [rechroma_plane(q, src_cell, dst_cell, size) for q in planes[1:]]


def video_cell(fmt):
    """-> the chroma cell (sub_x, sub_y) of a video format's name"""
    return {422: (2, 1), 420: (2, 2), 444: (1, 1)}[_entry(0, fmt)[1]]


def video_chroma_fit(plan, fmt, container=16, decoding=False, mode="cosited"):
    """ojphgpu_video_chroma_fit: the judgement of set_video_chroma on a plan alone, without a pipe or a device (OjphError
    E_INVALID where the setter would refuse) -> dict(src_cell, dst_cell = the stage's two cells (equal: the plain set_video
    hand-over), src_off, dst_off = where its planes stand, w, h, bytes = of the video buffer)"""
    f, n = capi.ChromaFrame(), C.c_uint64()
    m = capi.CHROMA.get(mode, mode)
    check(capi.lib().ojphgpu_video_chroma_fit(plan.handle, int(container), int(bool(decoding)), _video_code(plan, fmt, "video_chroma_fit"), int(m),
                                              C.byref(f), C.byref(n)), "video_chroma_fit")
    return dict(w=int(f.w), h=int(f.h), src_cell=(int(f.sfx), int(f.sfy)), dst_cell=(int(f.dfx), int(f.dfy)), src_off=tuple(int(x) for x in f.src_off),
                dst_off=tuple(int(x) for x in f.dst_off), bytes=int(n.value))


# RGB <-> YCbCr (ojphgpu.h section 7e): the numpy statement of ojphgpu_colour_table_make and of the two stages
COLOUR_STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}      # name -> (Kr, Kb)
ColourTable = collections.namedtuple("ColourTable", "m off lo hi k")     # m: 3 x 3 ints, off / lo / hi: 3 ints, k: fraction bits


class Colour(collections.namedtuple("Colour", "standard rgb_range ycc_range rgb_depth")):
    """what a pipe's colour= takes beside a standard's name: the ranges, and the depth of the RGB side (0: the plan's)"""
    def __new__(cls, standard, rgb_range="full", ycc_range="narrow", rgb_depth=0):
        if standard not in COLOUR_STANDARDS or rgb_range not in ("full", "narrow") or ycc_range not in ("full", "narrow"):
            raise ValueError("Colour: a standard of %s, ranges full or narrow" % ", ".join(sorted(COLOUR_STANDARDS)))
        return super().__new__(cls, standard, rgb_range, ycc_range, int(rgb_depth))


def _llround(x):                                      # C's llround: to nearest, halves away from zero
    a = abs(x)
    f = math.floor(a)
    f += (a - f) >= 0.5                               # (a - f is exact)
    return int(f) if x >= 0 else -int(f)


def colour_range(depth, rng):
    """-> (offset of RGB or luma, its span, offset of chroma, its span) of a depth-bit signal, full or narrow range"""
    depth = int(depth)
    if not 8 <= depth <= 16 or rng not in ("full", "narrow"):
        raise ValueError("colour_range: depths 8 .. 16, full or narrow")
    s = 1 << (depth - 8)
    return (0, (1 << depth) - 1, 128 * s, (1 << depth) - 1) if rng == "full" else (16 * s, 219 * s, 128 * s, 224 * s)


def colour_table(standard, direction, rgb_depth, ycc_depth, rgb_range="full", ycc_range="narrow"):
    """numpy statement of ojphgpu_colour_table_make (include/ojphgpu.h section 7e): every double expression in the order the
    library writes it -> ColourTable"""
    if standard not in COLOUR_STANDARDS or direction not in ("forward", "inverse"):
        raise ValueError("colour_table: a standard of %s, forward or inverse" % ", ".join(sorted(COLOUR_STANDARDS)))
    Kr, Kb = COLOUR_STANDARDS[standard]
    Kg = 1.0 - Kr - Kb
    off_rgb, span_rgb_i, _, _ = colour_range(rgb_depth, rgb_range)
    off_y, span_y, off_c, span_c = colour_range(ycc_depth, ycc_range)
    off_ycc, span_rgb, span_ycc = (off_y, off_c, off_c), float(span_rgb_i), (float(span_y), float(span_c), float(span_c))
    m = [[0] * 3 for _ in range(3)]
    off = [0] * 3
    if direction == "forward":
        A = ((Kr, Kg, Kb),
             (-Kr / (2.0 * (1.0 - Kb)), -Kg / (2.0 * (1.0 - Kb)), (1.0 - Kb) / (2.0 * (1.0 - Kb))),
             ((1.0 - Kr) / (2.0 * (1.0 - Kr)), -Kg / (2.0 * (1.0 - Kr)), -Kb / (2.0 * (1.0 - Kr))))
        for c in range(3):
            m[c][0] = _llround(A[c][0] * span_ycc[c] / span_rgb * 65536.0)
            m[c][2] = _llround(A[c][2] * span_ycc[c] / span_rgb * 65536.0)
            total = _llround(span_ycc[0] / span_rgb * 65536.0) if c == 0 else 0
            m[c][1] = total - m[c][0] - m[c][2]                  # green: the row's rounded total minus the other two
            off[c] = (off_ycc[c] << 16) - off_rgb * sum(m[c])
        top = (1 << int(ycc_depth)) - 1
    else:
        Ci = ((1.0, 0.0, 2.0 * (1.0 - Kr)),
              (1.0, -(2.0 * Kb * (1.0 - Kb) / Kg), -(2.0 * Kr * (1.0 - Kr) / Kg)),
              (1.0, 2.0 * (1.0 - Kb), 0.0))
        for c in range(3):
            for i in range(3):
                m[c][i] = 0 if Ci[c][i] == 0.0 else _llround(Ci[c][i] * span_rgb / span_ycc[i] * 65536.0)
            off[c] = (off_rgb << 16) - sum(m[c][i] * off_ycc[i] for i in range(3))
        top = (1 << int(rgb_depth)) - 1
    return ColourTable(tuple(tuple(r) for r in m), tuple(off), (0, 0, 0), (top, top, top), 16)


def _wrap64(x):                                       # a Python int as the int64 of the same 64 bits
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return np.int64(x - (1 << 64) if x >> 63 else x)


def _colour_spec(colour):
    col = colour if isinstance(colour, Colour) else Colour(colour)
    return capi.ColourSpec(capi.COLOUR_STANDARD[col.standard], capi.COLOUR_RANGE[col.rgb_range], capi.COLOUR_RANGE[col.ycc_range], col.rgb_depth)


def video_colour_fit(plan, fmt, colour, container=16, decoding=False):
    """ojphgpu_video_colour_fit: the judgement of set_video_colour on a plan alone, without a pipe or a device (OjphError
    E_INVALID where the setter would refuse) -> dict(table = the ColourTable the pipe would use, fx, fy, bytes = of the RGB
    buffer)"""
    spec, t, f, n = _colour_spec(colour), capi.ColourTable(), capi.ColourFrame(), C.c_uint64()
    check(capi.lib().ojphgpu_video_colour_fit(plan.handle, int(container), int(bool(decoding)), _video_code(plan, fmt, "video_colour_fit"), C.byref(spec),
                                              C.byref(t), C.byref(f), C.byref(n)), "video_colour_fit")
    table = ColourTable(tuple(tuple(int(x) for x in r) for r in t.m), tuple(int(x) for x in t.off), tuple(int(x) for x in t.lo),
                        tuple(int(x) for x in t.hi), int(t.k))
    return dict(table=table, fx=int(f.fx), fy=int(f.fy), bytes=int(n.value))


def _colour_finish(acc, table, c, kk):
    k = int(table.k)
    with np.errstate(over="ignore"):
        v = (acc + _wrap64(int(table.off[c]) << kk) + np.int64(1 << (k + kk - 1))) >> np.int64(k + kk)
    return np.clip(v, int(table.lo[c]), int(table.hi[c]))


def _colour_check(table, fx, fy):
    if fx not in (1, 2) or fy not in (1, 2) or int(table.k) != 16:
        raise ValueError("colour stage: factors are 1 or 2, k is 16")


def rgb_to_ycc(planes, table, fx=1, fy=1):
    """numpy statement of ojphgpu_frame_rgb_to_ycc (include/ojphgpu.h section 7e): planes = R, G, B [H, W] (unsigned samples as
    they stand) -> [Y [H, W], Cb [ch, cw], Cr [ch, cw]] (int64), cw = ceil(W / 2) where fx == 2, ch alike.  Per pixel t_c = m[c]
    . (R, G, B); a chroma sample stands ON source sample (fx i, fy j): taps (1, 2, 1) over t_c in every halved direction,
    indices clamped into the plane (resample_plane's filter and siting at phase 0), one rounding, the clamp to [lo, hi].  All
    sums in 64-bit two's complement."""
    _colour_check(table, fx, fy)
    a = [np.asarray(p).astype(np.int64) for p in planes]
    if len(a) != 3 or a[0].ndim != 2 or a[0].size == 0 or a[1].shape != a[0].shape or a[2].shape != a[0].shape:
        raise ValueError("rgb_to_ycc: three planes [H, W] of one size")
    h, w = a[0].shape

    def taps(n, f):
        if f == 1:
            return [(np.arange(n), 1)]
        c = 2 * np.arange((n + 1) // 2)
        return [(np.clip(c - 1, 0, n - 1), 1), (c, 2), (np.clip(c + 1, 0, n - 1), 1)]
    out = []
    with np.errstate(over="ignore"):
        for c in range(3):
            t = sum(_wrap64(table.m[c][i]) * a[i] for i in range(3))
            gx, gy = (fx, fy) if c else (1, 1)
            acc = 0
            for iy, wy in taps(h, gy):
                for ix, wx in taps(w, gx):
                    acc = acc + np.int64(wy * wx) * t[np.ix_(iy, ix)]
            out.append(_colour_finish(acc, table, c, 2 * ((gx == 2) + (gy == 2))))
    return out


def ycc_to_rgb(planes, table, fx=1, fy=1):
    """numpy statement of ojphgpu_frame_ycc_to_rgb: planes = Y [H, W], Cb, Cr [ch, cw] (samples as they stand, not clamped
    first) -> [R, G, B] [H, W] (int64).  Chroma at luma column x of a halved direction: 2 C[x / 2] for even x, C[(x - 1) / 2] +
    C[min((x + 1) / 2, cw - 1)] for odd x; rows alike, the product in 2-D; luma enters as Y << kk, kk = 1 per halved direction;
    the matrix, one rounding, the clamp to [lo, hi]."""
    _colour_check(table, fx, fy)
    y, cb, cr = [np.asarray(p).astype(np.int64) for p in planes]
    if y.ndim != 2 or y.size == 0:
        raise ValueError("ycc_to_rgb: the luma plane is [H, W]")
    h, w = y.shape
    cw, ch = (w + 1) // 2 if fx == 2 else w, (h + 1) // 2 if fy == 2 else h
    if cb.shape != (ch, cw) or cr.shape != (ch, cw):
        raise ValueError("ycc_to_rgb: chroma planes of %s and %s, not %s" % (cb.shape, cr.shape, (ch, cw)))

    def pair(n, nc, f):                               # the two chroma samples under each of n luma positions (weights 1, 1)
        x = np.arange(n)
        if f == 1:
            return [x]
        return [x // 2, np.where(x & 1, np.minimum((x + 1) // 2, nc - 1), x // 2)]
    kk = (fx == 2) + (fy == 2)
    v = [y << np.int64(kk)]
    for q in (cb, cr):
        v.append(sum(q[np.ix_(iy, ix)] for iy in pair(h, ch, fy) for ix in pair(w, cw, fx)))
    with np.errstate(over="ignore"):
        return [_colour_finish(sum(_wrap64(table.m[c][i]) * v[i] for i in range(3)), table, c, kk) for c in range(3)]


class EncoderPipe(_Handover):
    _side = "enc"

    def __init__(self, plan: Plan = None, params=None, device=0, depth=4, container=16, host_threads=0, pixels=None, packed=None, max_bytes=None,
                 max_sse=None, min_psnr=None, video=None, cap_bytes=0, colour=None, chroma=None, **kw):
        """pixels=(bits, big_endian): the frames are handed over pixel-interleaved ([H,W,C] of 8- or 16-bit samples, the
        order of .ppm files / capture buffers; 16-bit samples byte-swapped when big_endian) and turned into planes on
        the device.  video="uyvy" | "yuy2" | "v210" | "y210" | "y212" | "y216": the frames are handed over as one 4:2:2 video
        buffer (uint8 [H, row_bytes], pack_video's layout) and unpacked on the device; video="nv12" | "nv21" | "p010" | "p012" |
        "p016": as one 4:2:0 video buffer (uint8 [H + ceil(H / 2), row_bytes], pack_video420's tight layout); video="v410" | "y410" |
        "r210" | "r10k" | "y412" | "y416" | "ayuv" | "bgra" | "rgba" | "argb": as one 4:4:4 packed buffer (uint8 [H, row_bytes],
        pack_video444's layout).  colour="bt601" | "bt709" | "bt2020" or a Colour, with one of the RGB names among them ("bgra" |
        "rgba" | "argb" | "r210" | "r10k"): the buffer holds R, G, B and is coded as the plan's Y, Cb, Cr -- 4:4:4, 4:2:2 or 4:2:0
        -- converted on the device (set_video_colour).  chroma="cosited", with any other video name: the buffer's chroma format
        need not be the plan's (v210 into a 4:2:0 plan, nv12 into a 4:2:2 one, ...): halved or doubled on the device
        (set_video_chroma).  max_bytes: every frame is coded to that byte budget (set_budget); max_sse / min_psnr: ... to that
        quality target (set_quality) -- one or the other; cap_bytes=N with a target: to the target, but never above N bytes
        (set_quality(..., cap_bytes=N); from the start, or never)"""
        from .codec import _torch
        _torch()
        if cap_bytes and max_sse is None and min_psnr is None:
            raise ValueError("cap_bytes needs a quality target (max_sse or min_psnr); a byte budget alone is max_bytes")
        self.plan = plan if plan is not None else Plan(params if params is not None else make_params(**kw))
        self.container = int(container)
        self.depth = int(depth)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        check(self._lib.ojphgpu_enc_pipe_create(self.plan.handle, device, self.depth, self.container, host_threads,
                                                C.byref(self._h)), "enc_pipe_create")
        if pixels is not None:
            self.set_pixels(*pixels)
        if packed:
            self.set_packed(packed)
        if colour is not None and video is None:
            raise ValueError("colour= goes with video= (an RGB format)")
        if chroma is not None and (video is None or colour is not None):
            raise ValueError("chroma= goes with video= (a Y, Cb, Cr format), not with colour=")
        if colour is not None:
            self.set_video_colour(video, colour)
        elif chroma is not None:
            self.set_video_chroma(video, chroma)
        elif video is not None:
            self.set_video(video)
        if max_bytes:
            self.set_budget(max_bytes)
        if max_sse is not None or min_psnr is not None:
            self.set_quality(max_sse=max_sse, min_psnr=min_psnr, cap_bytes=cap_bytes)
        self.in_flight = 0

    def set_budget(self, max_bytes):
        """Every frame is coded at the finest step of the rate grid whose codestream is at most max_bytes long, the search
        started from the previous frame's answer (ojphgpu_enc_pipe_set_budget).  Switched on before the first acquire();
        afterwards the budget may change between frames -- the value at submit() is the frame's -- but not go to 0.  A frame
        no step fits raises OjphError (capi.E_BUDGET) from its collect()."""
        check(self._lib.ojphgpu_enc_pipe_set_budget(self._h, int(max_bytes)), "enc_pipe_set_budget")

    def rate_info(self):
        """of the frame collected last: dict(grid_index, qstep, bytes, bytes_finer, passes, first_guess), as
        codec.Encoder.rate_info"""
        info = capi.RateInfo()
        check(self._lib.ojphgpu_enc_pipe_rate_info(self._h, C.byref(info)), "enc_pipe_rate_info")
        return {k: getattr(info, k) for k, _ in capi.RateInfo._fields_}

    def set_quality(self, max_sse=None, min_psnr=None, cap_bytes=None):
        """Every frame is coded at the coarsest step of the rate grid found to meet the target -- the squared error between
        the frame and the decode of its codestream, over all components, is at most max_sse (an integer; 0 is a target), or
        min_psnr in dB turned into one by plan.psnr_to_sse -- the search started from the previous frame's answer
        (ojphgpu_enc_pipe_set_quality).  Switched on before the first acquire(); afterwards the target may change between
        frames -- the value at submit() is the frame's -- but not be switched off.  Not together with a byte budget.  A frame
        whose target no step meets raises OjphError (capi.E_QUALITY) from its collect().

        cap_bytes=N > 0: under a byte cap (ojphgpu_enc_pipe_set_quality_capped) -- on from the first call or never; afterwards
        both values may change between frames, the cap not back to 0; cap_bytes=None leaves the cap as it is.  Such a frame
        never raises E_QUALITY: the finest step that fits is written instead (capped_info() tells), and a frame whose cap not
        even the coarsest step fits raises OjphError (capi.E_BUDGET) from its collect()."""
        from .plan import psnr_to_sse
        if (max_sse is None) == (min_psnr is None):
            raise ValueError("set_quality: max_sse or min_psnr, one of them")
        t = int(max_sse) if max_sse is not None else psnr_to_sse(self.plan, float(min_psnr))
        if not 0 <= t < 2 ** 64:
            raise ValueError("set_quality: max_sse must fit 64 bits")
        if cap_bytes is None:
            check(self._lib.ojphgpu_enc_pipe_set_quality(self._h, t), "enc_pipe_set_quality")
            return
        if not 0 <= int(cap_bytes) < 2 ** 64:
            raise ValueError("set_quality: cap_bytes must fit 64 bits")
        check(self._lib.ojphgpu_enc_pipe_set_quality_capped(self._h, t, int(cap_bytes)), "enc_pipe_set_quality_capped")

    def capped_info(self):
        """of the frame collected last, on a pipe with a byte cap: the dict of codec.Encoder.capped_info; after E_BUDGET the
        passes and comps == []"""
        info = capi.CappedInfo()
        check(self._lib.ojphgpu_enc_pipe_capped_info(self._h, C.byref(info)), "enc_pipe_capped_info")
        out = {k: getattr(info, k) for k, _ in capi.CappedInfo._fields_ if k != "reserved"}
        out["comps"] = []
        for c in range(int(self.plan.params.num_comps)):
            sse, pae = C.c_uint64(), C.c_uint32()
            if self._lib.ojphgpu_enc_pipe_quality_comp(self._h, c, C.byref(sse), C.byref(pae)) != capi.OK:
                break
            out["comps"].append((int(sse.value), int(pae.value)))
        return out

    def quality_info(self):
        """of the frame collected last: dict(grid_index, qstep, sse, sse_coarser, pae, passes, bytes, comps), as
        codec.Encoder.quality_info, plus first_guess = the first index its search tried; after E_QUALITY only passes and
        first_guess are meaningful and comps is empty"""
        info, first = capi.QualityInfo(), C.c_uint32()
        check(self._lib.ojphgpu_enc_pipe_quality_info(self._h, C.byref(info), C.byref(first)), "enc_pipe_quality_info")
        out = {k: getattr(info, k) for k, _ in capi.QualityInfo._fields_}
        out["first_guess"] = int(first.value)
        out["comps"] = []
        for c in range(int(self.plan.params.num_comps)):
            sse, pae = C.c_uint64(), C.c_uint32()
            if self._lib.ojphgpu_enc_pipe_quality_comp(self._h, c, C.byref(sse), C.byref(pae)) != capi.OK:
                break
            out["comps"].append((int(sse.value), int(pae.value)))
        return out

    def close(self):
        if self._h:
            self._lib.ojphgpu_enc_pipe_destroy(self._h)
            self._h = None

    __del__ = close

    def acquire(self):
        """-> writable numpy view ([C,H,W] uint16 / int32; flat when components differ in size) of the pinned
        memory the next frame goes into, or None when every slot is in flight (collect first)"""
        ptr, n = C.c_void_p(), C.c_size_t()
        rc = self._lib.ojphgpu_enc_pipe_acquire(self._h, C.byref(ptr), C.byref(n))
        if rc == capi.E_AGAIN:
            return None
        check(rc, "enc_pipe_acquire")
        return _frame_view(self, ptr.value, n.value)

    def submit(self):
        check(self._lib.ojphgpu_enc_pipe_submit(self._h), "enc_pipe_submit")
        self.in_flight += 1

    def collect(self, copy=True):
        """the oldest frame's codestream; copy=False returns a view of pinned memory valid until the next collect"""
        ptr, n = C.c_void_p(), C.c_size_t()
        if self.in_flight <= 0:              # nothing to collect: the counter stays where it is (the C call would say E_INVALID too)
            raise capi.OjphError(capi.E_INVALID, "enc_pipe_collect: nothing in flight")
        rc = self._lib.ojphgpu_enc_pipe_collect(self._h, C.byref(ptr), C.byref(n))
        self.in_flight -= 1                  # the oldest frame is taken whatever its outcome (a frame of its own may fail with E_INVALID)
        check(rc, "enc_pipe_collect")
        v = _view(ptr.value, n.value)
        return v.tobytes() if copy else v

    def stats(self):
        out = (C.c_double * 4)()
        check(self._lib.ojphgpu_enc_pipe_stats(self._h, out), "enc_pipe_stats")
        return dict(frames=int(out[0]), host_tier2_ms=out[1], latency_ms=out[2], tier2_threads=int(out[3]))

    def encode_sequence(self, frames, budgets=None, targets=None, caps=None):
        """frames: iterable of [C,H,W] arrays -> generator of codestreams, in order.  budgets (a pipe with a byte budget):
        one int for every frame, or an iterable parallel to frames; a frame no step fits raises from here as from collect().
        targets (a pipe with a quality target): the same with max_sse values; not both.  caps (with targets, on a pipe with a
        byte cap): one cap for every frame, or an iterable parallel to frames"""
        if budgets is not None and targets is not None:
            raise ValueError("encode_sequence: budgets or targets, not both")
        if caps is not None and targets is None:
            raise ValueError("encode_sequence: caps need targets")
        # one of three modes: what the values are called, the values (one for all frames, or one per frame), how one is set
        if caps is not None:
            import itertools
            many = hasattr(targets, "__iter__") or hasattr(caps, "__iter__")
            each = lambda v: iter(v) if hasattr(v, "__iter__") else itertools.repeat(v)
            # (pairs; the shorter of two lists ends the values, as one list does)
            what, values = "targets and caps", zip(each(targets), each(caps)) if many else (targets, caps)
            setter = lambda v: self.set_quality(max_sse=v[0], cap_bytes=v[1])
        elif targets is not None:
            what, values, setter, many = "targets", targets, lambda v: self.set_quality(max_sse=v), hasattr(targets, "__iter__")
        else:
            what, values, setter, many = "budgets", budgets, self.set_budget, hasattr(budgets, "__iter__")
        if values is not None and not many:
            setter(values)
            values = None
        values = iter(values) if values is not None else None
        for n, f in enumerate(frames):
            if values is not None:                        # (before the first acquire() this is what switches the mode on)
                b = next(values, None)
                if b is None:
                    raise ValueError("encode_sequence: %s ended after %d values, frames go on" % (what, n))
                setter(b)
            buf = self.acquire()
            while buf is None:
                yield self.collect()
                buf = self.acquire()
            np.copyto(buf, np.asarray(f).astype(buf.dtype, copy=False).reshape(buf.shape), casting="unsafe")
            self.submit()
        while self.in_flight:
            yield self.collect()


class DecoderPipe(_Handover):
    _side = "dec"

    def __init__(self, first_codestream: bytes, device=0, depth=4, container=16, host_threads=0, resilient=False, pixels=None, packed=None,
                 skip_res=None, region=None, video=None, colour=None, chroma=None):
        """pixels=(bits, big_endian): decoded frames come back pixel-interleaved ([H,W,C]), clamped to the bit depth.
        skip_res=n or (for_data, for_recon), region=(x0, y0, w, h): the pipe decodes that view of every frame, as
        video="uyvy" | ...: they come back as one 4:2:2 video buffer (uint8 [H, row_bytes], pack_video of the planes);
        video="nv12" | "nv21" | "p010" | ...: as one 4:2:0 video buffer (uint8 [H + ceil(H / 2), row_bytes], pack_video420 of them);
        video="v410" | "bgra" | ...: as one 4:4:4 packed buffer (uint8 [H, row_bytes], pack_video444 of them).
        colour="bt709" | ... or a Colour, with video="bgra" | "rgba" | "argb" | "r210" | "r10k": the decoded Y, Cb, Cr planes (4:4:4,
        4:2:2 or 4:2:0) come back as that RGB buffer, converted on the device (set_video_colour).
        chroma="cosited", with any other video name: the buffer's chroma format need not be the codestream's (a 4:2:0 feed out as
        uyvy, a 4:4:4 master as nv12, ...): halved or doubled on the device (set_video_chroma).
        codec.Decoder takes them (ojphgpu_dec_pipe_create_view); .plan, the frames and pixels / packed are the view's"""
        from .codec import _torch
        _torch()
        self.container = int(container)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        buf = np.frombuffer(first_codestream, dtype=np.uint8)
        a, b = (0, 0) if not skip_res else ((skip_res, skip_res) if isinstance(skip_res, int) else skip_res)
        reg = None if region is None else (C.c_uint32 * 4)(*[int(v) for v in region])
        check(self._lib.ojphgpu_dec_pipe_create_view(buf.ctypes.data, len(first_codestream), int(resilient), int(a), int(b), reg, device, depth,
                                                     self.container, host_threads, C.byref(self._h)), "dec_pipe_create")
        h = C.c_void_p()
        check(self._lib.ojphgpu_dec_pipe_plan(self._h, C.byref(h)), "dec_pipe_plan")
        self.plan = Plan(handle=h, owned=False)
        self.plan.skip = (int(a), int(b))
        self.plan.region = None if region is None else tuple(int(v) for v in region)
        if pixels is not None:
            self.set_pixels(*pixels)
        if packed:
            self.set_packed(packed)
        if colour is not None and video is None:
            raise ValueError("colour= goes with video= (an RGB format)")
        if chroma is not None and (video is None or colour is not None):
            raise ValueError("chroma= goes with video= (a Y, Cb, Cr format), not with colour=")
        if colour is not None:
            self.set_video_colour(video, colour)
        elif chroma is not None:
            self.set_video_chroma(video, chroma)
        elif video is not None:
            self.set_video(video)
        self.in_flight = 0

    def close(self):
        if self._h:
            self._lib.ojphgpu_dec_pipe_destroy(self._h)
            self._h = None

    __del__ = close

    def acquire(self, nbytes):
        """-> writable uint8 view of pinned memory for the next codestream, or None when every slot is in flight"""
        ptr = C.c_void_p()
        rc = self._lib.ojphgpu_dec_pipe_acquire(self._h, nbytes, C.byref(ptr))
        if rc == capi.E_AGAIN:
            return None
        check(rc, "dec_pipe_acquire")
        return _view(ptr.value, nbytes)

    def submit(self):
        check(self._lib.ojphgpu_dec_pipe_submit(self._h), "dec_pipe_submit")
        self.in_flight += 1

    def collect(self, copy=True):
        """the oldest frame.  When code-blocks failed on a non-resilient pipe the C ABI still hands the frame out
        (failed blocks zeroed) with OJPHGPU_E_BLOCK: the exception raised here carries it as .frame and the count as
        .failed_blocks (ojphgpu.h, ojphgpu_dec_pipe_collect)"""
        ptr, n, failed = C.c_void_p(), C.c_size_t(), C.c_uint32()
        if self.in_flight <= 0:              # nothing to collect: the counter stays where it is
            raise capi.OjphError(capi.E_INVALID, "dec_pipe_collect: nothing in flight")
        rc = self._lib.ojphgpu_dec_pipe_collect(self._h, C.byref(ptr), C.byref(n), C.byref(failed))
        self.in_flight -= 1                  # the oldest frame is taken whatever its outcome (a codestream of another geometry fails with E_INVALID)
        if rc != capi.E_BLOCK:
            check(rc, "dec_pipe_collect")
        v = _frame_view(self, ptr.value, n.value)
        if rc == capi.E_BLOCK:
            err = capi.OjphError(rc, "dec_pipe_collect: %d code-blocks" % failed.value)
            err.frame, err.failed_blocks = v.copy(), int(failed.value)
            raise err
        return v.copy() if copy else v

    def stats(self):
        out = (C.c_double * 4)()
        check(self._lib.ojphgpu_dec_pipe_stats(self._h, out), "dec_pipe_stats")
        n = C.c_uint32()
        check(self._lib.ojphgpu_dec_pipe_fused_retries(self._h, C.byref(n)), "dec_pipe_fused_retries")
        return dict(frames=int(out[0]), host_parse_ms=out[1], latency_ms=out[2], host_threads=int(out[3]), fused_retries=int(n.value))

    def view_info(self):
        """of the frame collected last (ojphgpu_dec_pipe_view_info): dict(blocks = code-blocks decoded, plan_blocks = code-blocks
        of the codestream, staged_bytes = bytes laid out for the block decoder (a plain pipe's cross PCIe; of a view's, the runs' do, the zeros between
        them do not), runs (0: a plain
        pipe, which uploads one byte range), coded_bytes = of the decoded blocks)"""
        out = (C.c_uint64 * 5)()
        check(self._lib.ojphgpu_dec_pipe_view_info(self._h, out), "dec_pipe_view_info")
        return dict(blocks=int(out[0]), plan_blocks=int(out[1]), staged_bytes=int(out[2]), runs=int(out[3]), coded_bytes=int(out[4]))

    def decode_sequence(self, codestreams):
        for cs in codestreams:
            buf = self.acquire(len(cs))
            while buf is None:
                yield self.collect()
                buf = self.acquire(len(cs))
            buf[:] = np.frombuffer(cs, dtype=np.uint8)
            self.submit()
        while self.in_flight:
            yield self.collect()


class TranscoderPipe:
    """A sequence of codestreams recoded to another packaging, quantisation step or byte budget (ojphgpu_tc_pipe): what
    codec.Transcoder gives source by source, with the parse, the upload, the download and Tier-2 of neighbouring frames
    overlapped with the device."""

    def __init__(self, first_codestream: bytes, device=0, depth=4, host_threads=0, resilient=False, max_bytes=None, **kw):
        """first_codestream: parsed for the geometry (every later source must have the same).  kw: what changes, as
        plan.transcode_params takes it (qstep, block, prog_order, precinct, precincts, tlm, tileparts).  max_bytes=N: every
        source is recoded to a byte budget (set_budget); an irreversible output needs qstep or a budget -- without either,
        acquire() raises OjphError (capi.E_INVALID)."""
        from .codec import _torch
        from .plan import parse_codestream, transcode_params, transcode_plan
        _torch()
        self.depth = int(depth)
        self.resilient = bool(resilient)
        self.src_plan = parse_codestream(first_codestream, resilient)
        self.params = transcode_params(self.src_plan, **kw)
        self.plan = transcode_plan(self.src_plan, self.params)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        buf = np.frombuffer(first_codestream, dtype=np.uint8)
        check(self._lib.ojphgpu_tc_pipe_create(buf.ctypes.data, len(first_codestream), int(self.resilient), self.plan.handle, device, self.depth,
                                               host_threads, C.byref(self._h)), "tc_pipe_create")
        self.failed_blocks = 0
        self.in_flight = 0
        if max_bytes:
            self.set_budget(max_bytes)

    def set_budget(self, max_bytes):
        """Every source is recoded at the finest step of the rate grid whose codestream is at most max_bytes long, the search
        started from the previous frame's answer (ojphgpu_tc_pipe_set_budget).  Switched on before the first acquire();
        afterwards the budget may change between frames -- the value at submit() is the frame's -- but not go to 0.
        Irreversible outputs only.  A frame no step fits raises OjphError (capi.E_BUDGET) from its collect()."""
        check(self._lib.ojphgpu_tc_pipe_set_budget(self._h, int(max_bytes)), "tc_pipe_set_budget")

    def rate_info(self):
        """of the frame collected last: dict(grid_index, qstep, bytes, bytes_finer, passes, first_guess), as
        codec.Transcoder.rate_info; after E_BUDGET passes and first_guess"""
        info = capi.RateInfo()
        check(self._lib.ojphgpu_tc_pipe_rate_info(self._h, C.byref(info)), "tc_pipe_rate_info")
        return {k: getattr(info, k) for k, _ in capi.RateInfo._fields_}

    def close(self):
        if self._h:
            self._lib.ojphgpu_tc_pipe_destroy(self._h)
            self._h = None

    __del__ = close

    def acquire(self, nbytes):
        """-> writable uint8 view of pinned memory for the next source, or None when every slot is in flight"""
        ptr = C.c_void_p()
        rc = self._lib.ojphgpu_tc_pipe_acquire(self._h, nbytes, C.byref(ptr))
        if rc == capi.E_AGAIN:
            return None
        check(rc, "tc_pipe_acquire")
        return _view(ptr.value, nbytes)

    def submit(self):
        check(self._lib.ojphgpu_tc_pipe_submit(self._h), "tc_pipe_submit")
        self.in_flight += 1

    def collect(self, copy=True):
        """the oldest frame's output codestream; copy=False returns a view of pinned memory valid until its slot is acquired
        again.  failed_blocks = the source's blocks that did not decode (zero blocks of a resilient pipe).  A frame that
        failed -- it does not parse, has another geometry (capi.E_INVALID), failed blocks in a pipe that is not resilient
        (capi.E_BLOCK), a budget no step fits (capi.E_BUDGET) -- raises OjphError from here, and the sequence goes on."""
        ptr, n, failed = C.c_void_p(), C.c_size_t(), C.c_uint32()
        if self.in_flight <= 0:              # nothing to collect: the counter stays where it is
            raise capi.OjphError(capi.E_INVALID, "tc_pipe_collect: nothing in flight")
        rc = self._lib.ojphgpu_tc_pipe_collect(self._h, C.byref(ptr), C.byref(n), C.byref(failed))
        self.in_flight -= 1                  # the oldest frame is taken whatever its outcome
        self.failed_blocks = int(failed.value)
        check(rc, "tc_pipe_collect")
        v = _view(ptr.value, n.value)
        return v.tobytes() if copy else v

    def stats(self):
        out = (C.c_double * 4)()
        check(self._lib.ojphgpu_tc_pipe_stats(self._h, out), "tc_pipe_stats")
        n = C.c_uint32()
        check(self._lib.ojphgpu_tc_pipe_fused_retries(self._h, C.byref(n)), "tc_pipe_fused_retries")
        return dict(frames=int(out[0]), host_parse_ms=out[1], host_tier2_ms=out[2], latency_ms=out[3], fused_retries=int(n.value))

    def transcode_sequence(self, codestreams, budgets=None):
        """codestreams: iterable of sources -> generator of output codestreams, in order, `depth` frames in flight.  budgets (a
        pipe with a byte budget): one int for every frame, or an iterable parallel to codestreams; a frame that fails raises
        from here as from collect() (the generator ends with it: drive acquire / submit / collect to go on past one)"""
        if budgets is not None and not hasattr(budgets, "__iter__"):
            self.set_budget(budgets)
            budgets = None
        budgets = iter(budgets) if budgets is not None else None
        for n, cs in enumerate(codestreams):
            if budgets is not None:                       # (before the first acquire() this is what switches the mode on)
                b = next(budgets, None)
                if b is None:
                    raise ValueError("transcode_sequence: budgets ended after %d values, codestreams go on" % n)
                self.set_budget(b)
            buf = self.acquire(len(cs))
            while buf is None:
                yield self.collect()
                buf = self.acquire(len(cs))
            buf[:] = np.frombuffer(cs, dtype=np.uint8)
            self.submit()
        while self.in_flight:
            yield self.collect()
