"""The fused block decoder (ht_dec_fused_kernel) under every launch geometry, through its stage entry
(openjph_amd.codec.ht_decode_fused): the launches of tests/fused_cases.py -- every per_wave, wavefronts short of it, idle
wavefronts, one to three step-1 workgroups, both un-stuffing schemes; every slice schedule; runs one after the other on one
scratch -- decoded into a buffer filled with a sentinel.  Verdicts and samples are the oracle's, bit for bit; refused and
uncoded blocks are zero; every word outside the block rectangles still holds the sentinel; no wait ran out.

The shape and the un-stuffing scheme come from knobs read once per process (OJPHGPU_FUSED_SHAPE, OJPHGPU_FUSED_RINGS): the tests
take whatever the environment sets, and test_under_setting starts the file again in a child process per setting."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fused_cases as fc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scratch(launches):
    from openjph_amd import codec
    quads = max(codec.ht_decode_layout(L.desc_array(codec.cb_desc_dtype))[0] for L in launches)
    return codec.FusedScratch(max(L.n for L in launches), quads)


def _run(L, scratch):
    """one launch; asserts everything the module's docstring states"""
    from openjph_amd import capi, codec
    s = fc.shape_of(L.n, L.cus)
    tag = "%s [per_wave %d n1 %d worker workgroups %d NR %d shape %d]" % (L.tag, s["per_wave"], s["n1"], s["wwgs"], s["nr"], s["shape"])
    coef = torch.from_numpy(L.before()).cuda()
    descs = L.desc_array(codec.cb_desc_dtype)
    if not s["able"]:                                        # more step-1 workgroups than compute units: refused, nothing runs
        with pytest.raises(capi.OjphError) as ei:
            codec.ht_decode_fused(descs, L.data, coef, scratch, L.rev, L.cus)
        assert ei.value.code == capi.E_INVALID
        assert np.array_equal(coef.cpu().numpy(), L.before()), tag
        return
    before = scratch.epoch
    status, retry, epoch = codec.ht_decode_fused(descs, L.data, coef, scratch, L.rev, L.cus)
    assert epoch == before + 1
    assert retry != epoch, "%s: a wait ran out on a launch that is wholly resident" % tag
    problems = L.problems(status, coef.cpu().numpy())
    assert not problems, "%s: %s" % (tag, " | ".join(problems))


@pytest.mark.parametrize("i", range(len(fc.GEOMETRY)), ids=["n%d-cus%d" % g for g in fc.GEOMETRY])
def test_geometry(i):
    L = fc.geometry_launches()[i]
    _run(L, _scratch([L]))


@pytest.mark.parametrize("max_qh", fc.SLICE_QH)
def test_slices(max_qh):
    L = fc.slice_launch(max_qh)
    _run(L, _scratch([L]))


def test_sequences_on_one_scratch():
    """nothing is cleared between the runs except the coefficient buffer: records, flags, tickets and status bytes of the
    run before are there, under another geometry"""
    runs = fc.sequences()
    scratch = _scratch(runs)
    for L in runs:
        _run(L, scratch)
    assert scratch.epoch == len(runs)


N_TESTS = len(fc.GEOMETRY) + len(fc.SLICE_QH) + 1


@pytest.mark.parametrize("name", [n for n in fc.SETTINGS if n != "default"])
def test_under_setting(name):
    """the tests above in ONE child process per setting, with a timeout; a child that fails, ends on a signal or at its
    timeout fails this test and is not started again"""
    env = {k: v for k, v in os.environ.items() if k not in ("OJPHGPU_FUSED_SHAPE", "OJPHGPU_FUSED_RINGS")}
    env.update(fc.SETTINGS[name])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu",
                        "-k", "test_geometry or test_slices or test_sequences", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and ("%d passed" % N_TESTS).encode() in r.stdout, "setting %s %s:\n%s" % (
        name, fc.SETTINGS[name], r.stdout[-3000:].decode(errors="replace"))
