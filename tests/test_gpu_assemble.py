"""Codestream assembly and the pipes' copy kernel as stages (kernels_assemble.hip: assemble_codestream through codec.assemble,
copy_to_host_kernel through codec.copy_to_host).  In a codestream all placement jobs abut, so a lane that stores past its job's
end is overwritten -- or not -- by the neighbouring wavefront; here the jobs lie apart in a destination of fill, between
guards, and every byte is compared with the placement written in numpy (what t2_place_host does).

The table runs every residue of dst mod 16 with every residue of src mod 4 -- the head that aligns the destination, the four
source shifts of the 16-byte body -- at lengths around the head, one and several 16-byte pieces, one and several 1 KB steps of
a wavefront, and the `n < head` and `no whole piece` corners.  OJPHGPU_COPY_WGS, which sizes the grids of the copy and the gather
kernels and is read once per process, gets one child process per value."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.video_cases import FILL, GUARD, guarded_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 1023, 1024, 1025, 1040, 4101]
ABUTTING = 200
LAST = 37                                                    # the job that ends on the last byte of its source


def _jobs():
    """-> (jobs as (dst, src, n, blob) tuples, bytes of the destination, of the blob, of the data)"""
    jobs = []
    at = 0                                                   # end of the last job in the destination
    cur = [0, 0]                                             # ... in the data (0) and in the blob (1)

    def add(n, dres=None, sres=None, gap=0):
        nonlocal at
        d = at + gap
        if dres is not None:                                 # 1 to 40 bytes of fill in front, ending on the residue
            d = at + 1
            d += (dres - d) % 16
            if d + 16 - at <= 40 and (len(jobs) % 3) == 0:
                d += 16
            assert 1 <= d - at <= 40
        which = len(jobs) & 1                                # half from the blob, half from the data
        s = cur[which] + 1 + len(jobs) % 5
        if sres is not None:
            s += (sres - s) % 4
        jobs.append((d, s, n, which))
        at = d + n
        cur[which] = s + n
    for dres in range(16):
        for sres in range(4):
            for n in LENGTHS:
                add(n, dres, sres)
    add(1 + 6 % 40, 9, 2)                                    # the stretch starts apart from the table, on an odd residue
    for i in range(1, ABUTTING):                             # abutting jobs of 1 to 40 bytes, as a packet sequence has them
        add(1 + (i * 7 + 6) % 40)
    add(5, 3, 1)
    caps = [(c + 64 + 3) & ~3 for c in cur]
    d = at + 7
    jobs.append((d, caps[0] - LAST, LAST, 0))                # ends on the last byte of the data
    at = d + LAST
    return jobs, at + 9, caps[1], caps[0]


def _head(dst, n):
    return min((16 - dst % 16) % 16, n)


def test_assemble_table_covers_what_it_claims():
    jobs, total, nblob, ndata = _jobs()
    assert len(jobs) % 4 != 0, "the last workgroup must have idle wavefronts"
    assert nblob % 4 == 0 and ndata % 4 == 0
    table = jobs[:16 * 4 * len(LENGTHS)]
    assert {(d % 16, s % 4, n) for d, s, n, _ in table} == {(a, b, n) for a in range(16) for b in range(4) for n in LENGTHS}
    # the shift the body works with is that of the source behind the head
    assert {(d % 16, (s + _head(d, n)) % 4, n) for d, s, n, _ in table} == {(a, b, n) for a in range(16) for b in range(4) for n in LENGTHS}
    assert any(n < (16 - d % 16) % 16 for d, s, n, _ in table) and any(n >= 16 and (n - _head(d, n)) < 16 for d, s, n, _ in table)
    for w in (0, 1):
        assert abs(sum(1 for j in jobs if j[3] == w) - len(jobs) / 2) <= 1
    ends = [d + n for d, s, n, _ in jobs]
    gaps = [jobs[i + 1][0] - ends[i] for i in range(len(jobs) - 1)]
    assert all(0 <= g <= 40 for g in gaps)
    run = best = 0
    for i, g in enumerate(gaps):
        run = run + 1 if g == 0 and 1 <= jobs[i + 1][2] <= 40 else 0
        best = max(best, run)
    assert best == ABUTTING - 1                               # 200 jobs, 199 seams
    assert sum(1 for g in gaps if g == 0) == ABUTTING - 1     # every other job has fill in front of it
    assert jobs[-1][1] + jobs[-1][2] == ndata and jobs[-1][3] == 0
    assert all(s + n <= (nblob if b else ndata) for d, s, n, b in jobs) and ends[-1] < total


def _job_array(jobs):
    from openjph_amd import codec
    a = np.zeros(len(jobs), codec.t2_job_dtype)
    for i, (d, s, n, b) in enumerate(jobs):
        a[i] = (d, s, n, b)
    return a


def _guarded(nbytes):
    """-> (the whole tensor, the destination inside it): nbytes of fill between guards"""
    raw = torch.from_numpy(guarded_bytes(np.full(nbytes, FILL, np.uint8))).cuda()
    assert raw.data_ptr() % 16 == 0 and GUARD % 16 == 0
    return raw, raw[GUARD:GUARD + nbytes]


def test_assemble_places_every_job_and_nothing_else():
    from openjph_amd import codec
    jobs, total, nblob, ndata = _jobs()
    rng = np.random.default_rng(7)
    blob, data = rng.integers(0, 256, nblob, dtype=np.uint8), rng.integers(0, 256, ndata, dtype=np.uint8)
    want = np.full(total, FILL, np.uint8)
    for d, s, n, b in jobs:
        want[d:d + n] = (blob if b else data)[s:s + n]
    d_blob, d_data = torch.from_numpy(blob).cuda(), torch.from_numpy(data).cuda()
    assert d_blob.data_ptr() % 16 == 0 and d_data.data_ptr() % 16 == 0        # the residues of the table are those of the addresses
    raw, out = _guarded(total)
    assert codec.assemble(_job_array(jobs), d_blob, d_data, out) is out
    got = raw.cpu().numpy()
    assert (got[:GUARD] == FILL).all() and (got[GUARD + total:] == FILL).all(), "a guard of the destination was written"
    bad = np.nonzero(got[GUARD:GUARD + total] != want)[0]
    if bad.size:
        j = max(i for i, job in enumerate(jobs) if job[0] <= bad[0] or i == 0)
        assert False, "first difference at byte %d of %d, at or behind job %d %r" % (bad[0], total, j, jobs[j])
    assert np.array_equal(d_blob.cpu().numpy(), blob) and np.array_equal(d_data.cpu().numpy(), data)


def test_assemble_zero_jobs_launch_nothing():
    from openjph_amd import codec
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    raw, out = _guarded(512)
    codec.assemble(np.zeros(0, codec.t2_job_dtype), src, src, out)
    assert (raw.cpu().numpy() == FILL).all()


def test_assemble_wrapper_refuses_what_leaves_the_tensors():
    """on the host, before anything is launched"""
    from openjph_amd import codec
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    raw, out = _guarded(512)
    for job in ((0, 60, 5, 0), (0, 60, 5, 1), (0, 65, 0, 0), (510, 0, 3, 0), (513, 0, 0, 1), (1 << 63, 0, 1, 0), (0, 1 << 63, 1, 0), (0, 0, 0xFFFFFFFF, 1)):
        with pytest.raises(ValueError):
            codec.assemble(_job_array([job]), src, src, out)
    with pytest.raises(ValueError):
        codec.assemble(_job_array([(0, 0, 1, 0)]), src, src[:62], out)        # a source that is no whole number of dwords
    with pytest.raises(ValueError):
        codec.assemble(_job_array([(0, 0, 1, 0)]), src, src[1:61], out)       # ... or does not start on one
    with pytest.raises(ValueError):
        codec.assemble(_job_array([(0, 0, 1, 0)]), src, src.cpu(), out)
    assert (raw.cpu().numpy() == FILL).all()
    codec.assemble(_job_array([(509, 61, 3, 0), (0, 64, 0, 1), (512, 0, 0, 0)]), src, src, out)      # the last bytes of both: accepted
    assert (raw.cpu().numpy()[GUARD + 509:GUARD + 512] == 0).all() and (raw.cpu().numpy()[GUARD + 512:] == FILL).all()


# ---- the copy kernel -------------------------------------------------------------------------------------------------------------
STEP = 16384
COPY_BYTES = [0, 1, 15, 16, 17, 16368, STEP, 16405, 3 * STEP + 64007, 8 * STEP, 8 * STEP + 16, (1 << 20) + 13]


def check_copies():
    """every byte count, device memory to device memory: source, destination and the guards on both sides -> the number run"""
    from openjph_amd import codec
    rng = np.random.default_rng(8)
    for n in COPY_BYTES:
        src_np = rng.integers(0, 256, GUARD + n + GUARD, dtype=np.uint8)      # around the payload: bytes that are not the fill,
        src_np[:GUARD] |= 0x80                                               # so that one byte copied too many shows in the guard
        src_np[GUARD + n:] |= 0x80
        assert FILL < 0x80
        payload = src_np[GUARD:GUARD + n].copy()
        src = torch.from_numpy(src_np).cuda()
        raw, _ = _guarded(n)
        assert src.data_ptr() % 16 == 0
        codec.copy_to_host(raw[GUARD:], src[GUARD:], n)      # (n = 0: tensors that are not empty, a count that is)
        got = raw.cpu().numpy()
        assert (got[:GUARD] == FILL).all(), "%d bytes: the guard in front of the destination was written" % n
        assert (got[GUARD + n:] == FILL).all(), "%d bytes: the guard behind the destination was written" % n
        bad = np.nonzero(got[GUARD:GUARD + n] != payload)[0]
        assert bad.size == 0, "%d bytes: first difference at byte %d" % (n, bad[0])
        assert np.array_equal(src.cpu().numpy(), src_np), "%d bytes: the source was written" % n
    return len(COPY_BYTES)


def test_copy_every_byte_count():
    assert check_copies() == 12


def test_copy_refuses_misaligned_pointers_and_counts_beyond_the_tensors():
    from openjph_amd import capi, codec
    src = torch.arange(0, 256, dtype=torch.uint8, device="cuda")
    raw, dst = _guarded(256)
    for d, s, n in ((dst[1:], src, 32), (dst, src[8:], 32), (dst[4:], src[4:], 1), (dst[15:], src, 16)):
        with pytest.raises(capi.OjphError) as e:
            codec.copy_to_host(d, s, n)
        assert e.value.code == capi.E_INVALID
    for d, s, n in ((dst, src, 257), (dst[:16], src, 17), (dst, src[:16], 17), (dst, src, -1)):
        with pytest.raises(ValueError):
            codec.copy_to_host(d, s, n)
    assert (raw.cpu().numpy() == FILL).all()


def check_gather():
    """codec.gather_runs on the spans of tests/test_gpu_pipe_view.py: OJPHGPU_COPY_WGS sizes that kernel's grid too -> the
    number of runs"""
    from tests import test_gpu_pipe_view as pv
    src_np = np.random.default_rng(5).integers(0, 256, pv.SRC_CAP, dtype=np.uint8)
    d_src = torch.from_numpy(src_np).to("cuda:0")
    runs, staged = pv._layout(pv._gather_spans())
    pv._check_gather(src_np, d_src, runs, staged)
    return int(runs.size)


CHILD = r'''
import os, sys
sys.path.insert(0, %r)
from tests import test_gpu_assemble as t
print("COPY_WGS=%%s copies=%%d runs=%%d OK" %% (os.environ["OJPHGPU_COPY_WGS"], t.check_copies(), t.check_gather()))
'''


@pytest.mark.parametrize("wgs", [1, 3, 64])
def test_copy_and_gather_under_copy_wgs(wgs):
    """one fresh child process per value, under its own timeout; a child that fails, ends on a signal or at its timeout fails
    this test and is not started again"""
    from tests import test_gpu_pipe_view as pv
    env = dict(os.environ, OJPHGPU_COPY_WGS=str(wgs))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    line = "COPY_WGS=%d copies=%d runs=%d OK" % (wgs, len(COPY_BYTES), len(pv._gather_spans()))
    assert r.returncode == 0 and line.encode() in r.stdout, "OJPHGPU_COPY_WGS=%d:\n%s" % (wgs, r.stdout[-3000:].decode(errors="replace"))
