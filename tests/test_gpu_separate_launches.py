"""The separate block-decoder launches -- ht_dec_step1_raw_kernel or prep + ht_dec_step1_kernel, then ht_dec_step2_kernel<TX, WD>
or ht_dec_step2_multi_kernel<TX, NB> -- through their stage entry (openjph_amd.codec.ht_decode_separate): the launches of
tests/separate_cases.py, each under every step-2 instantiation that may decode its class of blocks, reached by the truthful
`kinds` of its descriptors and by valid coarsenings of it alone; wavefronts of two and four blocks ordered by hand; runs one
after the other on one scratch.  Everything is decoded into a buffer filled with a sentinel.  Verdicts and samples are the
oracle's, bit for bit; refused and uncoded blocks are zero; every word outside the block rectangles still holds the sentinel.

What step 1 is (CH, raw or prep form) and how many blocks a wavefront of step 2 may take come from knobs read once per process
(OJPHGPU_S1_CH, OJPHGPU_DEC_PREP, OJPHGPU_DEC_DUAL): the tests take whatever the environment sets, and test_under_setting
starts the file again in a child process per setting.  tests/test_cpu_separate_cases.py shows without a GPU which kernels and
grids all of this reaches."""
import os
import subprocess
import sys

import pytest

from tests import separate_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(i, v) for i, (cls, _, _) in enumerate(sc.TABLE) for v in sc.variants_of(cls)]


def _scratch(launches):
    from openjph_amd import codec
    need = [codec.ht_decode_layout(L.desc_array(codec.cb_desc_dtype)) for L in launches]
    return codec.SeparateScratch(max(L.n for L in launches), max(q for q, _ in need), max(a for _, a in need))


def _run(L, variant, scratch):
    """one launch; asserts everything the module's docstring states"""
    from openjph_amd import codec
    descs = L.desc_array(codec.cb_desc_dtype)
    kinds = sc.VARIANTS[variant][0](codec.ht_decode_kinds(descs))
    s = sc.launches_of(L.n, kinds)
    tag = "%s as %s [kinds 0x%x: step 1 %s<%d> on %d workgroups, step 2 %s<%d, %d> on %d]" % (
        L.tag, variant, kinds, "prep +" if s["prep"] else "raw", s["ch"], s["wgs1"], "multi" if s["multi"] else "single", s["tx"],
        s["nb"] if s["multi"] else s["wd"], s["wgs2"])
    coef = torch.from_numpy(L.before()).cuda()
    status = codec.ht_decode_separate(descs, L.data, coef, scratch, kinds)
    got = coef.cpu().numpy()
    if (got != sc.expected(L)).any() or ((status != 0) != (L.status != 0)).any():
        problems = L.problems(status, got)
        assert not problems, "%s: %s" % (tag, " | ".join(problems))


@pytest.mark.parametrize("i,variant", RUNS, ids=["%s-%s-%s-%s" % (sc.TABLE[i][0], sc.TABLE[i][1], "rev" if sc.TABLE[i][2] else "irv", v) for i, v in RUNS])
def test_launch(i, variant):
    L = sc.launches()[i]
    _run(L, variant, _scratch([L]))


def test_sequences_on_one_scratch():
    """nothing is cleared between the runs except the coefficient buffer: the records, flat strings and status bytes of the run
    before are there, from other blocks at the same positions and under another kernel"""
    runs = sc.sequences()
    scratch = _scratch([L for L, _ in runs])
    for L, variant in runs:
        _run(L, variant, scratch)
    assert scratch.runs == len(runs)


N_TESTS = len(RUNS) + 1


@pytest.mark.parametrize("name", [n for n in sc.SETTINGS if n != "default"])
def test_under_setting(name):
    """the tests above in ONE child process per setting, with a timeout; a child that fails, ends on a signal or at its
    timeout fails this test and is not started again"""
    env = {k: v for k, v in os.environ.items() if k not in sc.KNOBS}
    env.update(sc.SETTINGS[name])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu",
                        "-k", "test_launch or test_sequences", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and ("%d passed" % N_TESTS).encode() in r.stdout, "setting %s %s:\n%s" % (
        name, sc.SETTINGS[name], r.stdout[-3000:].decode(errors="replace"))
