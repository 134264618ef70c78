"""The frame hand-over kernels of kernels_pixels.hip as stages: pixel-interleaved samples <-> planes (unpack_kernel / pack_kernel
through codec.unpack_pixels / pack_pixels) and bit strings <-> containers (unpack_bits_kernel / pack_bits_kernel through
codec.unpack_bits / pack_bits).  Everything is bit for bit against a numpy restatement -- transpose, byte swap and np.clip for
the pixels, pipeline.pack_bits / unpack_bits (pinned by tests/test_pack_bits.py) for the bit strings -- and every destination
lies between guards of tests/video_cases.py that must still hold the fill afterwards.

A thread of the pixel kernels takes 4 pixels and a workgroup 1024; a thread of the bit kernels 32 samples and a workgroup 8192:
the counts sit on both sides of each.  Every suite asserts its own coverage."""
import numpy as np
import pytest

from tests.video_cases import FILL, GUARD, guarded_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# ---- A. pixel-interleaved samples ----------------------------------------------------------------------------------------------
# (w, h): pixel counts 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027, 4097
SIZES = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (7, 1), (8, 1), (341, 3), (32, 32), (205, 5), (79, 13), (17, 241)]
COUNTS = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027, 4097]
COMPS = [1, 2, 3, 4, 5]
# (pixel bits, big endian, container bits)
FORMS = [(8, False, 8), (8, False, 16), (8, False, 32), (16, False, 16), (16, True, 16), (16, False, 32), (16, True, 32)]
TWO_FORMS = [(8, False, 32), (16, True, 16)]
FORM_SIZES = [(5, 1), (205, 5), (17, 241)]                  # 5, 1025 and 4097 pixels
DEPTHS = {8: (1, 5, 8), 16: (9, 12, 16)}
NP = {8: np.uint8, 16: np.uint16, 32: np.int32}
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def _template(nc):
    """the instantiation launch_unpack / launch_pack picks: NC = 1, 3, 4, or 0 (the generic path)"""
    return nc if nc in (1, 3, 4) else 0


def _pixel_cases():
    """(form, (w, h), components): every count and component number at two forms; every form at 5, 1025 and 4097 pixels with
    3 and 5 components -- and with 1 and 4, so that every form meets every template"""
    cases = [(f, s, c) for f in TWO_FORMS for s in SIZES for c in COMPS]
    cases += [(f, s, c) for f in FORMS for s in FORM_SIZES for c in (3, 5, 1, 4)]
    assert sorted({w * h for _, (w, h), _ in cases}) == COUNTS
    assert {(f, w * h, c) for f, (w, h), c in cases} >= {(f, n, c) for f in TWO_FORMS for n in COUNTS for c in COMPS}
    assert {(f, w * h, c) for f, (w, h), c in cases} >= {(f, n, c) for f in FORMS for n in (5, 1025, 4097) for c in (3, 5)}
    assert {(f, _template(c)) for f, _, c in cases} == {(f, t) for f in FORMS for t in (0, 1, 3, 4)}
    assert {c for _, _, c in cases if _template(c) == 0} == {2, 5}          # the generic path twice
    return cases


def _dev(a):
    """a numpy array's bytes on the device, as a uint8 tensor"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _tdtype(bits):
    return {8: torch.uint8, 16: torch.int16, 32: torch.int32}[bits]


def _placed(a, shift):
    """the array on the device as a contiguous tensor of its element size that starts on a 16-byte boundary (shift 0) or
    `shift` elements behind one"""
    item = a.dtype.itemsize
    raw = np.concatenate([np.zeros(16 + shift * item, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])
    t = torch.from_numpy(raw).cuda()[16 + shift * item:].view(_tdtype(8 * item)).reshape(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == (shift * item) % 16
    return t


class Guarded:
    """a destination of `n` elements of `bits` bits between guards, all of it holding the fill; shift: it starts that many
    elements behind a 16-byte boundary"""

    def __init__(self, n, bits, shift=0):
        self.front, self.nbytes = GUARD + shift * (bits // 8), n * (bits // 8)
        self.raw = torch.from_numpy(guarded_bytes(np.full(self.nbytes, FILL, np.uint8), front=self.front)).cuda()
        self.view = self.raw[self.front:self.front + self.nbytes].view(_tdtype(bits))
        assert self.view.data_ptr() % 16 == (shift * (bits // 8)) % 16 and self.raw.data_ptr() % 16 == 0

    def content(self, tag):
        """-> the destination's bytes; the guards must hold the fill"""
        got = self.raw.cpu().numpy()
        assert (got[:self.front] == FILL).all(), "%s: the guard in front of the destination was written" % (tag,)
        assert (got[self.front + self.nbytes:] == FILL).all(), "%s: the guard behind the destination was written" % (tag,)
        return got[self.front:self.front + self.nbytes]

    def untouched(self):
        return bool((self.raw.cpu().numpy() == FILL).all())


def _file_dtype(pb, be):
    return np.dtype(np.uint8) if pb == 8 else np.dtype(">u2" if be else "<u2")


def _run_unpack(form, size, nc, rng, shift):
    from openjph_amd import codec
    (pb, be, cb), (w, h) = form, size
    values = rng.integers(0, 1 << pb, (h, w, nc))
    values.reshape(-1)[:: max(values.size // 7, 1)] = (1 << pb) - 1
    file_bytes = values.astype(_file_dtype(pb, be))                        # the samples as the file holds them
    want = np.transpose(values, (2, 0, 1)).astype(NP[cb])
    dst = Guarded(nc * h * w, cb, shift)
    got = codec.unpack_pixels(_placed(file_bytes.view(NP[pb]), shift), big_endian=be, out=dst.view)
    tag = ("unpack", form, size, nc, shift)
    assert got.shape == (nc, h, w) and got.data_ptr() == dst.view.data_ptr()
    content = dst.content(tag)
    assert np.array_equal(content.view(NP[cb]).reshape(nc, h, w), want), tag


def _specials(depth, cb):
    """name -> value: 0, maxv, maxv + 1 (where the container holds it) and the container's maximum; in int32 containers also
    -1, INT_MIN and INT_MAX"""
    maxv = (1 << depth) - 1
    top = INT_MAX if cb == 32 else (1 << cb) - 1
    out = {"0": 0, "maxv": maxv, "top": top}
    if maxv + 1 <= top:
        out["maxv+1"] = maxv + 1
    if cb == 32:
        out.update({"-1": -1, "INT_MIN": INT_MIN, "INT_MAX": INT_MAX})
    return out


def _run_pack(form, size, nc, depth, rng, shift, seen):
    from openjph_amd import codec
    (pb, be, cb), (w, h) = form, size
    maxv = (1 << depth) - 1
    top = INT_MAX if cb == 32 else (1 << cb) - 1
    values = rng.integers(0, min(2 * maxv + 2, top + 1), (nc, h, w)).astype(np.int64)
    special = _specials(depth, cb)
    at = rng.permutation(values.size)[: max(values.size // 3, 1)]
    values.reshape(-1)[at] = rng.choice(list(special.values()), at.size)
    seen.setdefault((pb, cb), set()).update(k for k, v in special.items() if (values == v).any())
    want = np.ascontiguousarray(np.transpose(np.clip(values, 0, maxv), (1, 2, 0))).astype(_file_dtype(pb, be))
    dst = Guarded(nc * h * w, pb, shift)
    got = codec.pack_pixels(_placed(values.astype(NP[cb]), shift), depth, pixel_bits=pb, big_endian=be, out=dst.view)
    tag = ("pack", form, size, nc, depth, shift)
    assert got.shape == (h, w, nc) and got.data_ptr() == dst.view.data_ptr()
    content = dst.content(tag)
    assert np.array_equal(content, want.view(np.uint8).reshape(-1)), tag


def test_unpack_pixels_every_count_component_number_and_form():
    rng = np.random.default_rng(1)
    ran = set()
    for form, size, nc in _pixel_cases():
        _run_unpack(form, size, nc, rng, 0)
        ran.add((form, _template(nc)))
    assert ran == {(f, t) for f in FORMS for t in (0, 1, 3, 4)}


def test_pack_pixels_every_count_component_number_form_and_depth():
    rng = np.random.default_rng(2)
    ran, depths, seen = set(), {8: set(), 16: set()}, {}
    for i, (form, size, nc) in enumerate(_pixel_cases()):
        depth = DEPTHS[form[0]][i % 3]
        _run_pack(form, size, nc, depth, rng, 0, seen)
        ran.add((form, _template(nc)))
        depths[form[0]].add(depth)
    assert ran == {(f, t) for f in FORMS for t in (0, 1, 3, 4)}
    assert depths == {8: set(DEPTHS[8]), 16: set(DEPTHS[16])}
    for (pb, cb), names in seen.items():                     # what the clamp met
        assert {"0", "maxv", "maxv+1", "top"} <= names and (cb != 32 or {"-1", "INT_MIN", "INT_MAX"} <= names), (pb, cb, sorted(names))
    assert set(seen) == {(pb, cb) for pb, _, cb in FORMS}


def test_pixels_one_element_past_a_16_byte_boundary():
    """source and destination are contiguous views into larger tensors that start one element behind a 16-byte boundary:
    every form, every template, at 5, 1025 and 4097 pixels"""
    rng = np.random.default_rng(3)
    ran = set()
    for i, (form, size, nc) in enumerate((f, s, c) for f in FORMS for s in FORM_SIZES for c in (1, 3, 4, 5)):
        _run_unpack(form, size, nc, rng, 1)
        _run_pack(form, size, nc, DEPTHS[form[0]][i % 3], rng, 1, {})
        ran.add((form, _template(nc)))
    assert ran == {(f, t) for f in FORMS for t in (0, 1, 3, 4)}


def test_pixels_refusals_leave_the_destination_alone():
    from openjph_amd import capi, codec
    w, h, nc = 5, 3, 3
    refused = 0

    def invalid(call, dst):
        nonlocal refused
        with pytest.raises(capi.OjphError) as e:
            call()
        assert e.value.code == capi.E_INVALID and dst.untouched()
        refused += 1

    px8, px16 = _placed(np.zeros((h, w, nc), np.uint8), 0), _placed(np.zeros((h, w, nc), np.uint16), 0)
    pl8, pl32 = _placed(np.zeros((nc, h, w), np.uint8), 0), _placed(np.full((nc, h, w), 3, np.int32), 0)
    # 16-bit pixels and 8-bit containers
    dst = Guarded(nc * h * w, 8)
    invalid(lambda: codec.unpack_pixels(px16, out=dst.view), dst)
    dst = Guarded(nc * h * w, 16)
    invalid(lambda: codec.pack_pixels(pl8, 8, pixel_bits=16, out=dst.view), dst)
    # bit_depth > pixel_bits (and 0)
    for pb, depth in ((8, 9), (16, 17), (8, 0)):
        dst = Guarded(nc * h * w, pb)
        invalid(lambda: codec.pack_pixels(pl32, depth, pixel_bits=pb, out=dst.view), dst)
    # zero components, zero width, zero height: the C entries themselves, with pointers that are valid
    lib = capi.lib()
    for ww, hh, cc in ((w, h, 0), (0, h, nc), (w, 0, nc)):
        dst = Guarded(nc * h * w, 32)
        invalid(lambda: capi.check(lib.ojphgpu_unpack_pixels(None, px8.data_ptr(), dst.view.data_ptr(), ww, hh, cc, 8, 0, 32), "unpack_pixels"), dst)
        dst = Guarded(nc * h * w, 8)
        invalid(lambda: capi.check(lib.ojphgpu_pack_pixels(None, pl32.data_ptr(), dst.view.data_ptr(), ww, hh, cc, 32, 8, 0, 8), "pack_pixels"), dst)
    torch.cuda.synchronize()
    assert refused == 2 + 3 + 6
    # ... and the same calls with sizes that are valid run
    dst = Guarded(nc * h * w, 8)
    capi.check(lib.ojphgpu_pack_pixels(None, pl32.data_ptr(), dst.view.data_ptr(), w, h, nc, 32, 8, 0, 8), "pack_pixels")
    torch.cuda.synchronize()
    assert (dst.content("pack") == 3).all()


# ---- B. bit strings --------------------------------------------------------------------------------------------------------------
BIT_COUNTS = [1, 31, 32, 33, 63, 8191, 8192, 8193, 16401]
BIT_FORMS = [(bits, cb) for bits in (10, 12, 14) for cb in (16, 32)]


def test_unpack_bits_every_count_and_form():
    """the spare samples of the last group of 32 hold random bits; nothing is written behind sample n - 1"""
    from openjph_amd import codec
    from openjph_amd import pipeline as pl
    rng = np.random.default_rng(4)
    ran = set()
    for bits, cb in BIT_FORMS:
        for n in BIT_COUNTS:
            samples = rng.integers(0, 1 << bits, n)
            samples[:: max(n // 5, 1)] = (1 << bits) - 1
            string = np.unpackbits(pl.pack_bits(samples, bits), bitorder="little")
            assert string.size == (n + 31) // 32 * 32 * bits
            string[n * bits:] = rng.integers(0, 2, string.size - n * bits)
            packed = np.packbits(string, bitorder="little")
            want = pl.unpack_bits(packed, bits, n)
            assert np.array_equal(want, samples)
            dst = Guarded(n, cb)
            got = codec.unpack_bits(_placed(packed, 0), bits, n, out=dst.view)
            assert got.shape == (n,) and got.data_ptr() == dst.view.data_ptr()
            content = dst.content(("unpack_bits", bits, cb, n))
            assert np.array_equal(content.view(NP[cb]).astype(np.int64), want.astype(np.int64)), (bits, cb, n)
            ran.add((bits, cb, n))
    assert ran == {(b, c, n) for b, c in BIT_FORMS for n in BIT_COUNTS} and len(BIT_FORMS) == 6


def test_pack_bits_every_count_and_form_clamps():
    """the destination holds the fill beforehand; afterwards the padded groups are pipeline.pack_bits of the clamped samples,
    padding samples zero, and the guard behind them is intact"""
    from openjph_amd import codec
    from openjph_amd import pipeline as pl
    rng = np.random.default_rng(5)
    ran, seen = set(), {}
    for bits, cb in BIT_FORMS:
        maxv = (1 << bits) - 1
        special = [maxv, maxv + 1, 65535] + ([-1, -maxv - 1, INT_MIN, INT_MAX, 65536, 1 << bits << 16] if cb == 32 else [])
        for k, n in enumerate(BIT_COUNTS):
            v = rng.integers(0, 1 << bits, n).astype(np.int64)
            at = rng.permutation(n)[: max(n // 3, 1)]
            v[at] = rng.choice(special, at.size) if n > 1 else special[(k + bits + cb) % 3]
            seen.setdefault((bits, cb), set()).update(int(x) for x in np.unique(v[at]))
            want = pl.pack_bits(np.clip(v, 0, maxv), bits)
            nbytes = (n + 31) // 32 * 4 * bits
            assert want.size == nbytes
            dst = Guarded(nbytes, 8)
            got = codec.pack_bits(_placed(v.astype(NP[cb]), 0), bits, out=dst.view)
            assert got.shape == (nbytes,) and got.data_ptr() == dst.view.data_ptr()
            content = dst.content(("pack_bits", bits, cb, n))
            bad = np.nonzero(content != want)[0]
            assert bad.size == 0, "pack_bits %d/%d n %d: first difference at byte %d" % (bits, cb, n, bad[0])
            assert np.array_equal(pl.unpack_bits(content, bits, (n + 31) // 32 * 32)[n:], np.zeros((-n) % 32, np.uint32))
            ran.add((bits, cb, n))
    assert ran == {(b, c, n) for b, c in BIT_FORMS for n in BIT_COUNTS}
    for (bits, cb), vals in seen.items():                    # the clamp met what it must change: one past the range first of all
        assert {(1 << bits) - 1, 1 << bits, 65535} <= vals and (cb != 32 or {-1, INT_MIN, INT_MAX} <= vals), (bits, cb)


def test_bits_without_out_allocate_what_they_return():
    from openjph_amd import codec
    from openjph_amd import pipeline as pl
    v = np.random.default_rng(6).integers(0, 1 << 12, 33).astype(np.int32)
    packed = codec.pack_bits(_placed(v, 0), 12)
    assert packed.dtype == torch.uint8 and np.array_equal(packed.cpu().numpy(), pl.pack_bits(v, 12))
    back = codec.unpack_bits(packed, 12, 33, dtype=torch.int32)
    assert back.dtype == torch.int32 and np.array_equal(back.cpu().numpy(), v)


def test_bits_refusals_leave_the_destination_alone():
    from openjph_amd import capi, codec
    n = 40
    nbytes = 2 * 4 * 14                                      # two groups of the widest form
    packed = _placed(np.zeros(nbytes + 16, np.uint8), 0)
    s16, s32, s8 = (_placed(np.ones(n, t), 0) for t in (np.uint16, np.int32, np.uint8))
    refused = 0

    def invalid(call, dst):
        nonlocal refused
        with pytest.raises(capi.OjphError) as e:
            call()
        assert e.value.code == capi.E_INVALID and dst.untouched()
        refused += 1

    for cb, samples in ((16, s16), (32, s32)):
        dst = Guarded(n, cb)
        invalid(lambda: codec.unpack_bits(packed, 11, n, out=dst.view), dst)                       # bits 11
        invalid(lambda: codec.unpack_bits(packed, 12, 0, out=dst.view), dst)                       # n = 0
        invalid(lambda: codec.unpack_bits(packed[2:], 12, n, out=dst.view), dst)                   # 2-byte aligned bit string
        dst = Guarded(nbytes + 16, 8)
        invalid(lambda: codec.pack_bits(samples, 11, out=dst.view), dst)
        invalid(lambda: codec.pack_bits(samples[:0], 12, out=dst.view), dst)
        invalid(lambda: codec.pack_bits(samples, 12, out=dst.view[2:]), dst)
    dst = Guarded(n, 8)                                                                            # container 8
    invalid(lambda: codec.unpack_bits(packed, 12, n, out=dst.view), dst)
    dst = Guarded(nbytes, 8)
    invalid(lambda: codec.pack_bits(s8, 12, out=dst.view), dst)
    assert refused == 14
