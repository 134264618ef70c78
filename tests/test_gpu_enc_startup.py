"""The narrow block encoder's entry and exit (ht_encode_kernel): a wavefront requests its first sample rows before the
workgroup's table copy and barrier, every wavefront of a workgroup -- also one with nothing to code -- reaches that barrier
and leaves behind it, and the claim of the output slot is issued before the coded bytes are tidied in LDS.  Launches through
the C ABI (ojphgpu_ht_encode: both wavelets' instantiations, the wide kernel and the 64-bit one run over every launch), the
coded bytes of every block against the oracle's, at the smallest inputs that reach each of those paths."""
import numpy as np
import pytest

from tests.synth import random_block

pytestmark = pytest.mark.gpu

OUT_STAGE = 5120          # bytes of coded output a wavefront stages in LDS (NOUT_CAP of kernels_ht_enc.hip)


def _block(rng, w, h, kmax, kind, dens, amp, tight=False):
    """one code-block: (w, h, kmax, kind, plane as 32-bit elements, pitch, the oracle's coded bytes).  kind: "rev" (5/3
    integers), "irv" (9/7 floats, quantised in the kernel), "s64" (64-bit sample path).  tight: rows follow each other
    without padding, so the block's last sample is the last element of its plane."""
    from oracle import oraclebind as ob
    from tests.test_gpu_wide import wide_block
    pitch = w if tight else (w + 63) & ~63
    if w == 0 or h == 0:
        return (w, h, kmax, kind, np.zeros(0, np.int32), pitch, 0.0, b"")
    delta = 0.0
    if kind == "rev":
        _, v = random_block(rng, w, h, pitch, kmax, dens, amp)
        plane = np.zeros((h, pitch), np.int32); plane[:, :w] = v[:, :w]
        q, mx = ob.quant_rev(np.ascontiguousarray(plane[:, :w]), kmax)
        want = ob.ht_encode(q, w, h, w, kmax - 1, 0) if mx >= (1 << (31 - kmax)) else b""
        words = plane.ravel()
    elif kind == "irv":
        step = 2.0 ** -6 * (1.0 + rng.random())          # a coefficient x is coded as the magnitude floor(|x| / step) <= amp
        delta = np.float32(step) / np.float32(1 << (31 - kmax))
        plane = np.zeros((h, pitch), np.float32)
        plane[:, :w] = ((rng.random((h, w)) - 0.5) * (rng.random((h, w)) < dens) * (1.96 * amp * step)).astype(np.float32)
        q, mx = ob.quant_irv(np.ascontiguousarray(plane[:, :w]), float(np.float32(1.0) / np.float32(delta)))
        want = ob.ht_encode(q, w, h, w, kmax - 1, 0) if mx >= (1 << (31 - kmax)) else b""
        words = plane.view(np.int32).ravel()
    else:
        sm, v = wide_block(rng, w, h, kmax, dens, min(kmax, 30))
        plane = np.zeros((h, pitch), np.int64); plane[:, :w] = v
        mx = int(np.bitwise_or.reduce((np.abs(v).astype(np.uint64) << np.uint64(63 - kmax)).ravel()))
        want = ob.ht_encode64(sm, w, h, w, kmax - 1, 0) if mx >= (1 << (63 - kmax)) else b""
        words = plane.view(np.int32).ravel()
    return (w, h, kmax, kind, words, pitch, float(delta), bytes(want))


def _launch(blocks, out_cap=None):
    """one ojphgpu_ht_encode launch over `blocks`; the coefficient tensor ends with the last block's last element"""
    import torch
    from openjph_amd import codec
    from openjph_amd.csrc_consts import block_scratch_bytes
    descs = np.zeros(len(blocks), codec.cb_desc_dtype)
    parts, off, soff = [], 0, 0
    for i, (w, h, kmax, kind, words, pitch, delta, _) in enumerate(blocks):
        if kind == "s64" and off & 1:                    # int64 samples: 8-byte aligned
            parts.append(np.zeros(1, np.int32)); off += 1
        d = descs[i]
        d["coef_off"], d["pitch"], d["w"], d["h"] = off, pitch, w, h
        d["K_max"], d["reversible"], d["delta"] = kmax, {"rev": 1, "irv": 0, "s64": 1 | 4}[kind], delta
        d["data_off"], d["scratch_cap"] = soff, block_scratch_bytes(w, h, kmax)
        parts.append(words); off += words.size; soff += int(d["scratch_cap"])
    coef = torch.from_numpy(np.concatenate(parts + [np.zeros(0, np.int32)]) if off else np.zeros(1, np.int32)).cuda()
    assert coef.numel() == max(off, 1)
    return codec.ht_encode(descs, coef, soff, soff if out_cap is None else out_cap)


def _check(blocks, res, out, upto=None):
    bad = []
    for i, b in enumerate(blocks[:upto]):
        o, n = int(res[i, 0]), int(res[i, 1])
        g = out[o:o + n].tobytes()
        if g != b[-1] or (n == 0 and o != 0):
            bad.append((i, b[:4], o, n, len(b[-1])))
    assert not bad, "HT encode mismatches (idx, (w, h, kmax, kind), offset, got_len, want_len): %s" % bad[:8]


SHAPES = [(64, 64), (32, 32), (64, 64), (17, 9), (64, 64), (8, 64), (64, 64), (64, 31), (64, 64)]


@pytest.mark.parametrize("tight", [False, True], ids=["padded", "tight"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 9])
def test_idle_wavefronts_in_the_last_workgroup(n, tight):
    """n blocks in workgroups of four wavefronts: the last workgroup has wavefronts whose index is beyond n.  `tight`: no
    element of the coefficient tensor lies behind the last block's last sample."""
    rng = np.random.default_rng(100 + n)
    blocks = [_block(rng, w, h, 11, "irv" if i & 1 else "rev", 0.5, 700, tight) for i, (w, h) in enumerate(SHAPES[:n])]
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)


def test_mixed_launch_every_instantiation_skips_blocks():
    """5/3 and 9/7 blocks, blocks of <= 32, <= 64 and 65..128 columns, a block of the 64-bit path and empty blocks in ONE
    launch, interleaved so that every workgroup of every kernel holds wavefronts that code and wavefronts that do not."""
    rng = np.random.default_rng(7)
    spec = [(64, 64, "rev"), (32, 32, "irv"), (128, 32, "rev"), (64, 64, "s64"),
            (0, 16, "rev"), (64, 64, "irv"), (16, 0, "irv"), (20, 20, "rev"),
            (100, 16, "irv"), (0, 0, "rev"), (64, 33, "irv"), (31, 64, "rev"),
            (16, 0, "rev"), (48, 48, "s64"), (0, 7, "irv"), (96, 8, "rev"), (64, 64, "irv")]
    blocks = [_block(rng, w, h, 20 if kind == "s64" else 10, kind, 0.6, 500) for (w, h, kind) in spec]
    assert sum(1 for b in blocks if len(b[-1]) > 0) == sum(1 for (w, h, _) in spec if w and h)
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)


@pytest.mark.parametrize("kind", ["rev", "irv"])
def test_small_and_ragged_blocks(kind):
    """1 x 1 up to 64 x 17: widths that are no multiple of four (eight dword loads per lane instead of two 16-byte ones),
    blocks of fewer rows than a step, odd heights whose last step lacks quad rows and the last sample row."""
    rng = np.random.default_rng(11)
    shapes = [(1, 1), (1, 64), (64, 1), (3, 5), (63, 63), (64, 17), (64, 13), (4, 3), (2, 2), (64, 9)]
    for tight in (False, True):
        blocks = [_block(rng, w, h, 9, kind, 1.0, 300, tight) for (w, h) in shapes]
        res, out, status = _launch(blocks)
        assert status == 0
        _check(blocks, res, out)


def test_block_without_a_significant_sample_claims_nothing():
    rng = np.random.default_rng(12)
    blocks = [_block(rng, 64, 64, 10, "irv", 0.5, 500), _block(rng, 64, 64, 10, "irv", 0.0, 1), _block(rng, 64, 64, 10, "irv", 0.5, 500),
              _block(rng, 32, 32, 10, "rev", 0.5, 500), _block(rng, 32, 32, 10, "rev", 0.0, 1), _block(rng, 32, 32, 10, "rev", 0.5, 500)]
    assert [len(b[-1]) > 0 for b in blocks] == [True, False, True, True, False, True]
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)
    assert tuple(res[1]) == (0, 0) and tuple(res[4]) == (0, 0)
    # nothing but the four coded blocks, each in a 4-byte aligned slot, was claimed
    assert len(out) == sum((len(b[-1]) + 3) & ~3 for b in blocks)


def test_stage_overflow_spills_and_is_claimed_with_a_spilled_part():
    """64 x 64 blocks of 16-bit noise at K_max 18: more MagSgn bytes than the 5 KB LDS stage holds, so the stage is flushed
    to the block's scratch slot while it is coded and the claim is made with a part of the block already in HBM."""
    rng = np.random.default_rng(13)
    blocks = [_block(rng, 64, 64, 18, "rev", 1.0, 65535), _block(rng, 64, 64, 18, "rev", 1.0, 65535), _block(rng, 64, 64, 17, "rev", 1.0, 65535)]
    assert all(len(b[-1]) > OUT_STAGE + 2048 for b in blocks)
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)


def test_output_too_small_for_the_last_block():
    """The last block -- by far the longest to code, so it claims last -- does not fit what the earlier ones left of the
    output: status set, its length 0, the earlier blocks' bytes as they should be."""
    rng = np.random.default_rng(14)
    blocks = [_block(rng, 8, 8, 9, "irv" if i & 1 else "rev", 1.0, 300) for i in range(4)] + [_block(rng, 64, 64, 12, "irv", 1.0, 4095)]
    assert all(len(b[-1]) > 0 for b in blocks)
    small = sum((len(b[-1]) + 3) & ~3 for b in blocks[:-1])
    res, out, status = _launch(blocks, out_cap=small + ((len(blocks[-1][-1]) + 3) & ~3) - 4)
    assert status != 0
    assert tuple(res[4]) == (0, 0)
    _check(blocks, res, out, upto=4)
