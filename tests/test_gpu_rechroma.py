"""ojphgpu_frame_rechroma (kernels_chroma.hip; include/ojphgpu.h section 7f) against pipeline.rechroma_frame, bit for bit: tiny
frames of every size under every pairing of chroma cells and the three containers, planes on every residue of their 16 bytes,
int32 samples with negatives and the type's ends, a frame whose threads take several turns, sentinels around every
destination plane, and the host's refusals."""
import ctypes as C

import numpy as np
import pytest

from openjph_amd import capi, pipeline
from tests.chroma_cases import CELLS, DTYPES, PAIRS, random_planes

pytestmark = pytest.mark.gpu

SENTINEL = {8: 0xA5, 16: 0xA5C3, 32: -0x5A3C5A3D}


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def run_batch(cases, bits, residues=None):
    """cases = [(w, h, s, d, planes)]: every frame's planes laid into ONE source buffer and ONE destination buffer with gaps
    between them, the destination filled with a sentinel; one launch per frame; the whole destination buffer must then be the
    expected planes with the sentinel everywhere else.  residues = [(rs, rd)] per frame: its source planes start rs elements
    behind a 16-byte boundary, its destination planes rd; None: gaps of 1, 2, 3, ... elements, so that the planes wander over
    the residues"""
    from openjph_amd import codec
    dt, g = DTYPES[bits], 128 // bits
    jobs, sn, dn, k = [], 0, 0, 0
    for n, (w, h, s, d, planes) in enumerate(cases):
        want = [p.astype(dt) for p in pipeline.rechroma_frame(planes, s, d)]
        so, do = [], []
        for p, q in zip(planes, want):
            if residues:
                sn, dn = -(-sn // g) * g + g + residues[n][0], -(-dn // g) * g + g + residues[n][1]
            else:
                sn, dn, k = sn + 1 + k % g, dn + 1 + (k // 3) % g, k + 1
            so.append(sn); do.append(dn)
            sn += p.size; dn += q.size
        jobs.append((w, h, s, d, want, so, do))
        assert all(p.dtype == dt for p in planes)
    src, exp = np.zeros(sn + 1, dt), np.full(dn + 16, SENTINEL[bits], dt)
    for (w, h, s, d, want, so, do), case in zip(jobs, cases):
        for p, q, a, b in zip(case[4], want, so, do):
            src[a:a + p.size] = p.reshape(-1)
            exp[b:b + q.size] = q.reshape(-1)
    d_src, d_dst = to_dev(src), to_dev(np.full(dn + 16, SENTINEL[bits], dt))
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    for w, h, s, d, want, so, do in jobs:
        codec.frame_rechroma(d_src, d_dst, w, h, s, d, src_off=so, dst_off=do)
    got = d_dst.cpu().numpy().view(dt)
    if not np.array_equal(got, exp):                            # name the first frame that differs
        for n, (w, h, s, d, want, so, do) in enumerate(jobs):
            for c, (q, b) in enumerate(zip(want, do)):
                assert np.array_equal(got[b:b + q.size], q.reshape(-1)), (bits, w, h, s, d, "plane %d" % c, residues and residues[n])
        assert False, "a sentinel between the planes was overwritten (%d-bit)" % bits
    return jobs


@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("s,d", PAIRS, ids=["%d%d-%d%d" % (s + d) for s, d in PAIRS])
def test_every_tiny_size_bit_for_bit(s, d, bits):
    rng = np.random.default_rng(bits + 10 * CELLS.index(s) + 100 * CELLS.index(d))
    run_batch([(w, h, s, d, random_planes(rng, w, h, s, bits)) for w in range(1, 20) for h in range(1, 8)], bits)


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_planes_on_every_residue(bits):
    """source and destination planes at every pair of residues of their 16 bytes (a 16-bit destination two bytes off is among
    them), the pairings in turn; 37 x 5: more than one group to a row, an odd width"""
    g = 128 // bits
    rng = np.random.default_rng(bits)
    cases, residues = [], []
    for rs in range(g):
        for rd in range(g):
            s, d = PAIRS[(rs * g + rd) % len(PAIRS)]
            cases.append((37, 5, s, d, random_planes(rng, 37, 5, s, bits)))
            residues.append((rs, rd))
    jobs = run_batch(cases, bits, residues)
    for (w, h, s, d, want, so, do), (rs, rd) in zip(jobs, residues):
        assert all(a % g == rs for a in so) and all(b % g == rd for b in do)


def test_int32_extremes_stay_inside_their_inputs():
    """negative samples and INT32_MIN / INT32_MAX: the 64-bit sums, and the no-clamp property on what the device wrote"""
    from openjph_amd import codec
    rng = np.random.default_rng(32)
    for s, d in PAIRS:
        planes = random_planes(rng, 21, 11, s, 32)
        planes[1][:] = np.where(rng.integers(0, 2, planes[1].shape) == 1, 2 ** 31 - 1, -2 ** 31)     # nothing but the ends
        src = np.concatenate([p.reshape(-1) for p in planes])
        got = codec.frame_rechroma(to_dev(src), None, 21, 11, s, d).cpu().numpy()
        want = pipeline.rechroma_frame(planes, s, d)
        assert np.array_equal(got, np.concatenate([p.reshape(-1) for p in want]).astype(np.int32)), (s, d)
        assert min(int(p.min()) for p in planes) == -2 ** 31 and max(int(p.max()) for p in planes) == 2 ** 31 - 1
        n = 21 * 11
        assert got[n:].min() >= min(int(p.min()) for p in planes[1:]) and got[n:].max() <= max(int(p.max()) for p in planes[1:])


@pytest.mark.parametrize("bits,pairs", [(16, (((1, 1), (2, 2)), ((2, 2), (1, 1)), ((2, 1), (1, 2)), ((2, 1), (2, 2)), ((2, 1), (2, 1)))),
                                        (8, (((1, 2), (2, 1)),)), (32, (((2, 2), (2, 1)),))], ids=["16", "8", "32"])
def test_threads_take_several_turns(bits, pairs, monkeypatch):
    """2100 x 37 under OJPHGPU_CHROMA_WGS=2: one workgroup per plane, so every thread takes a second and a third item, in the
    copy loop and in the resampling loop"""
    monkeypatch.setenv("OJPHGPU_CHROMA_WGS", "2")
    rng = np.random.default_rng(2100 + bits)
    run_batch([(2100, 37, s, d, random_planes(rng, 2100, 37, s, bits)) for s, d in pairs], bits)


def test_host_refusals():
    import torch
    lib = capi.lib()
    w, h = 18, 6
    src = torch.zeros(3 * w * h + 8, dtype=torch.int16, device="cuda")
    dst = torch.zeros(3 * w * h + 8, dtype=torch.int16, device="cuda")
    ps, pd = src.data_ptr(), dst.data_ptr()

    def frame(sfx=2, sfy=1, dfx=2, dfy=2, ww=w, hh=h, so=(0, w * h, 2 * w * h), do=(0, w * h, 2 * w * h)):
        f = capi.ChromaFrame(ww, hh, sfx, sfy, dfx, dfy)
        f.src_off[:] = so
        f.dst_off[:] = do
        return f

    def call(a, b, bits, f):
        return lib.ojphgpu_frame_rechroma(None, C.c_void_p(a), C.c_void_p(b), bits, None if f is None else C.byref(f))
    assert call(ps, pd, 16, frame()) == capi.OK
    torch.cuda.synchronize()
    assert call(None, pd, 16, frame()) == capi.E_INVALID and call(ps, None, 16, frame()) == capi.E_INVALID and call(ps, pd, 16, None) == capi.E_INVALID
    for bad in (dict(sfx=3), dict(sfy=0), dict(dfx=4), dict(dfy=3), dict(ww=0), dict(hh=0)):
        assert call(ps, pd, 16, frame(**bad)) == capi.E_INVALID, bad
    for bits in (0, 12, 24, 64):
        assert call(ps, pd, bits, frame()) == capi.E_INVALID
    assert call(ps + 1, pd, 16, frame()) == capi.E_INVALID and call(ps, pd + 1, 16, frame()) == capi.E_INVALID      # off the container's alignment
    assert call(ps + 2, pd, 32, frame(ww=4, hh=2, so=(0, 8, 16), do=(0, 8, 16))) == capi.E_INVALID
    assert call(ps + 1, pd + 3, 8, frame()) == capi.OK                                                                 # bytes stand anywhere
    torch.cuda.synchronize()
    # a source plane over a destination plane: the same buffer; the destination's Cr plane reaching into the source's luma
    assert call(ps, ps, 16, frame()) == capi.E_INVALID
    tiny = dict(ww=4, hh=2, sfx=1, sfy=1, dfx=2, dfy=1, so=(0, 8, 16))                      # source planes [0, 8), [8, 16), [16, 24)
    assert call(ps, ps, 16, frame(do=(23, 40, 50), **tiny)) == capi.E_INVALID             # the destination's luma begins on the source's last sample
    assert call(ps, ps, 16, frame(do=(24, 40, 50), **tiny)) == capi.OK                    # one buffer, planes apart
    torch.cuda.synchronize()
    assert call(ps + 2 * (w * h // 2), ps, 16, frame(ww=4, hh=2, so=(0, 8, 16), do=(0, 8, w * h // 2 - 1))) == capi.E_INVALID
    assert torch.count_nonzero(dst[3 * w * h:]).item() == 0
