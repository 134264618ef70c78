"""The narrow block encoder's sample-row loads (ht_encode_kernel): blocks whose width is a multiple of four run an
instantiation of the step loop whose rows are ONE 16-byte load per lane, the others one with eight clamped dword loads; the
kernel can also be built with the rows of two steps in flight in two register sets and the loop unrolled by two
(-DENC_ROWS_AHEAD=2, not the shipped form: DESIGN 4.4).  What can go wrong is where the kinds of load, the sets and the steps
meet: step counts of both parities, a ragged last step at either position of a pair, steps that are skipped, rows that are
dword- but not 16-byte aligned, wavefronts of one workgroup in different instantiations, and leaving the loop with loads in
flight.  Coded bytes against the oracle's (oracle.oraclebind, pinned to the reference).

The C ABI's block launch (ojphgpu_ht_encode) does not know the widths of its blocks and always takes the 16-pairs-by-4-rows
layout (LOGP 4); the 8 x 8 layout of launches without a block wider than 32 columns (LOGP 3) and the 32 x 2 one of blocks of
65..128 columns (LOGP 5) are chosen by the encoder objects, so their cases are frames without a decomposition -- the frame
is its one sub-band and a frame no larger than a code-block is ONE block of exactly that shape -- whose codestream must be
the oracle pipeline's, byte for byte."""
import numpy as np
import pytest

from tests.test_gpu_enc_startup import OUT_STAGE, _block, _check, _launch

pytestmark = pytest.mark.gpu

KINDS = ["rev", "irv"]


# ---- step counts of both parities --------------------------------------------------------------------------------------

# 8 sample rows per step: 1, 1, 2, 2, 3, 3, 4, 5 and 8 steps; 9 / 17 / 25 / 33: a last step of one sample row, 1: a block of one
H64 = [1, 8, 9, 16, 17, 24, 25, 33, 64]
W64 = [64, 60, 4, 63, 61, 5, 1]                      # multiples of four (16-byte loads) and not (dword loads)


@pytest.mark.parametrize("kind", KINDS)
def test_step_counts_blocks_up_to_64_columns(kind):
    rng = np.random.default_rng(201)
    blocks = [_block(rng, w, h, 10, kind, 0.6, 500) for h in H64 for w in W64]
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)


def _frame_blocks(kind, block, shapes, seed):
    """every (w, h) of `shapes` as a frame of its own without a decomposition and with code-blocks of `block`: one block of
    w x h.  Half of the samples sit at mid-grey (zero coefficients), the others are noise."""
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    rng = np.random.default_rng(seed)
    bad = []
    for (w, h) in shapes:
        img = np.where(rng.random((1, h, w)) < 0.5, 2048, rng.integers(0, 4096, (1, h, w))).astype(np.int64)
        kw = dict(bit_depth=12, num_decomps=0, block=block, reversible=(kind == "rev"))
        if kind == "irv":
            kw["qstep"] = 0.002
        got = codec.encode(img, **kw)
        want = cp.encode(img, **kw)[0]
        assert len(want) > 150 + (w * h) // 8             # (a coded block, not an empty packet)
        if got != want:
            bad.append((w, h, len(got), len(want)))
    assert not bad, "codestream differs from the oracle's (w, h, got, want bytes): %s" % bad


@pytest.mark.parametrize("kind", KINDS)
def test_step_counts_blocks_up_to_32_columns(kind):
    """16 sample rows per step (8 pairs by 8 quad rows): 1, 2, 2, 3, 3 and 4 steps"""
    _frame_blocks(kind, (32, 64), [(w, h) for h in (16, 17, 32, 33, 48, 64) for w in (32, 28, 31)], 202)


@pytest.mark.parametrize("kind", KINDS)
def test_step_counts_blocks_of_65_to_128_columns(kind):
    """4 sample rows per step (32 pairs by 2 quad rows): 1, 2, 2, 3, 3 and 8 steps"""
    _frame_blocks(kind, (128, 32), [(w, h) for h in (4, 5, 8, 9, 12, 32) for w in (128, 100, 68, 127, 66)], 203)


# ---- neighbouring wavefronts in different instantiations ----------------------------------------------------------------

def test_both_kinds_of_load_interleaved_in_one_launch():
    """workgroups of four wavefronts: 16-byte, dword, 16-byte, dword ...; then the same with empty and 0 x n blocks between
    them, so that every workgroup also holds a wavefront that only meets the barrier"""
    rng = np.random.default_rng(204)
    spec = [(64, 64), (63, 64), (60, 33), (61, 33), (4, 9), (5, 9), (32, 17), (31, 17),
            (64, 24), (0, 16), (63, 24), (16, 0), (8, 64), (0, 0), (7, 64), (64, 25), (0, 3), (1, 25), (64, 64)]
    blocks = [_block(rng, w, h, 11, KINDS[i % 3 == 0], 0.6, 700) for i, (w, h) in enumerate(spec)]
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)
    assert all(tuple(res[i]) == (0, 0) for i, (w, h) in enumerate(spec) if w == 0 or h == 0)


# ---- 16-byte loads from rows that are only dword aligned ----------------------------------------------------------------

@pytest.mark.parametrize("lead", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_aligned_to_a_dword_only(kind, lead):
    """`lead` 1 x 1 blocks in front of blocks without row padding: every later block starts `lead` elements past a multiple of
    four, its rows (pitch = width) stay there or -- widths 60, 36, 4 -- move on; the last sample is the tensor's last element"""
    rng = np.random.default_rng(205 + lead)
    shapes = [(1, 1)] * lead + [(64, 64), (60, 17), (4, 9), (36, 33), (64, 16), (8, 64), (64, 25)]
    blocks = [_block(rng, w, h, 10, kind, 0.7, 500, tight=True) for (w, h) in shapes]
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)


# ---- steps without a significant sample, at even and odd steps ----------------------------------------------------------

def _banded_block(rng, kind, w, empty, kmax=10):
    """a w x 64 block whose 8-row bands (one step each) listed in `empty` hold no significant sample"""
    from oracle import oraclebind as ob
    h, pitch = 64, 64
    keep = np.ones((h, 1), bool)
    for b in empty:
        keep[8 * b:8 * b + 8] = False
    if kind == "rev":
        v = rng.integers(-500, 501, (h, w)) * (rng.random((h, w)) < 0.6) * keep
        plane = np.zeros((h, pitch), np.int32); plane[:, :w] = v
        q, mx = ob.quant_rev(np.ascontiguousarray(plane[:, :w]), kmax)
        words, delta = plane.ravel(), 0.0
    else:
        step = 2.0 ** -6 * 1.5
        delta = np.float32(step) / np.float32(1 << (31 - kmax))
        plane = np.zeros((h, pitch), np.float32)
        # (an empty band is not all zero: magnitudes below one step quantise to no significant sample)
        plane[:, :w] = np.where(keep, (rng.random((h, w)) - 0.5) * (rng.random((h, w)) < 0.6) * (1.96 * 500 * step),
                                (rng.random((h, w)) - 0.5) * step).astype(np.float32)
        q, mx = ob.quant_irv(np.ascontiguousarray(plane[:, :w]), float(np.float32(1.0) / np.float32(delta)))
        words = plane.view(np.int32).ravel()
    want = ob.ht_encode(q, w, h, w, kmax - 1, 0) if mx >= (1 << (31 - kmax)) else b""
    return (w, h, kmax, kind, words, pitch, float(delta), bytes(want))


EMPTY_BANDS = [(0, 1), (1,), (2, 3), (1, 3, 5, 7), (0, 2, 4, 6), (0, 1, 2, 3, 4, 5, 6), (7,), (6, 7)]


@pytest.mark.parametrize("kind", KINDS)
def test_skipped_steps_at_even_and_odd_positions(kind):
    """the "step without a significant sample below one without" skip at even and odd steps, directly before and after coded
    steps, and as the last step; 64 columns (16-byte loads) and 63 (dword loads); a block that is all such steps in between"""
    rng = np.random.default_rng(209)
    blocks = []
    for w in (64, 63):
        for empty in EMPTY_BANDS:
            blocks.append(_banded_block(rng, kind, w, empty))
        blocks.append(_banded_block(rng, kind, w, tuple(range(8))))
        blocks.append(_banded_block(rng, kind, w, ()))
    assert [len(b[-1]) > 0 for b in blocks] == ([True] * len(EMPTY_BANDS) + [False, True]) * 2
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)
    nothing = [i for i, b in enumerate(blocks) if not b[-1]]
    assert all(tuple(res[i]) == (0, 0) for i in nothing)
    assert len(out) == sum((len(b[-1]) + 3) & ~3 for b in blocks)


# ---- leaving the loop or the kernel with loads in flight ----------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_output_one_dword_too_small_for_the_last_block(kind):
    rng = np.random.default_rng(210)
    blocks = [_block(rng, w, h, 9, kind, 1.0, 300) for (w, h) in [(8, 8), (7, 9), (4, 17), (64, 8)]] + [_block(rng, 64, 64, 12, kind, 1.0, 4095)]
    assert all(len(b[-1]) > 0 for b in blocks)
    cap = sum((len(b[-1]) + 3) & ~3 for b in blocks) - 4
    res, out, status = _launch(blocks, out_cap=cap)
    assert status != 0
    assert tuple(res[4]) == (0, 0)
    _check(blocks, res, out, upto=4)


def test_stage_overflow_at_both_step_parities():
    """Noise deep enough to outgrow the 5 KB stage, which is then flushed to the scratch slot inside the step loop: 64 x 64
    (8 steps) of 16-bit noise at K_max 18, 64 x 33 (5 steps, the last one a single sample row) of 26-bit noise at K_max 26;
    63 columns for the dword loads"""
    rng = np.random.default_rng(211)
    blocks = [_block(rng, w, h, 18 if h == 64 else 26, "rev", 1.0, 65535 if h == 64 else (1 << 26) - 1)
              for (w, h) in [(64, 64), (64, 33), (63, 64), (63, 33), (64, 64)]]
    assert all(len(b[-1]) > OUT_STAGE + 1024 for b in blocks)
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)
