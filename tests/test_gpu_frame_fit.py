"""ojphgpu_frame_fit (openjph_amd/csrc/kernels_fit.hip) against pipeline.fit_frame, bit for bit: every run length around a
group of four, every place a run can start in its 16 bytes, a destination that sits differently in its 16 bytes than the
source (the sample-by-sample path), the three containers and the fit in place, both signs, shifts up and down, the values
at the clamp's ends and at the ends of int32 -- and a sentinel around every run."""
import numpy as np
import pytest

from openjph_amd.pipeline import fit_frame

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
COUNTS = (0, 1, 3, 4, 5, 7, 8, 1023)
# 48 components make 2048 // 48 = 42 workgroups each: 42 * 256 threads take one group of four per step and four steps per
# turn of the loop, so a run beyond 42 * 256 * 4 * 4 elements sends a thread round the loop twice
LONG = 42 * 256 * 16 + 4 * 256 * 5 + 3
SHIFTS = (-2, 0, 1, 2, 6)
GAP = 5                                                      # sentinel elements between runs
SENTINEL = {8: 0x5A, 16: 0x5A5A, 32: 0x5A5A5A5A}


def values(n, bo, shift, signed, rng):
    """n source samples for an output of bo bits: random ones over and past the range, then the clamp's ends and their
    neighbours (as the source sees them), ties of the rounding, and the ends of int32"""
    bs = bo + shift
    lo, hi = (-(1 << (bs - 1)), (1 << (bs - 1)) - 1) if signed else (0, (1 << bs) - 1)
    v = rng.integers(lo - (hi - lo) // 8 - 4, hi + (hi - lo) // 8 + 4, size=n, dtype=np.int64)
    special = [lo - 2, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 2, I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1, 0, -1, 1]
    if shift > 0:
        half, one = 1 << (shift - 1), 1 << shift
        special += [half - 1, half, half + 1, -half - 1, -half, -half + 1, one + half, -one - half, hi - half, hi - half + 1, lo - half - 1, lo - half]
    k = min(n, len(special))
    if k:
        v[rng.choice(n, size=k, replace=False)] = special[:k] if n < len(special) else special
    return np.clip(v, I32_MIN, I32_MAX).astype(np.int32)


def layout(counts, starts):
    """runs of these lengths, run i starting at an element congruent to starts[i] modulo 4, GAP sentinels at least between"""
    comps, at = [], GAP
    for n, s in zip(counts, starts):
        at += (s - at) % 4
        comps.append((at, n))
        at += n + GAP
    return comps, at + GAP


def run_case(bits, signed, counts, starts, dst_off=0, in_place=False, seed=1):
    import torch
    from openjph_amd import codec
    rng = np.random.default_rng(seed)
    bo = {8: 8, 16: 12, 32: 20}[bits]
    comps, total = layout(counts, starts)
    src = np.full(total, 0x5A5A5A5A, np.int32)
    fc, want = [], {}
    for i, (first, n) in enumerate(comps):
        shift = SHIFTS[i % len(SHIFTS)]
        sg = signed if signed is not None else bool(i & 1)
        src[first:first + n] = values(n, bo, shift, sg, rng)
        lo, hi = (-(1 << (bo - 1)), (1 << (bo - 1)) - 1) if sg else (0, (1 << bo) - 1)
        fc.append((first, n, shift, lo, hi))
        g = fit_frame([src[first:first + n]], [bo + shift], [bo], [sg])[0]
        want[i] = g.astype(np.int64) & ((1 << bits) - 1)       # the container's bits, whatever its sign
    d_src = torch.from_numpy(src).cuda()
    if in_place:
        d_out = d_src
    else:
        # dst_off elements into a buffer that starts on 16 bytes, as the source does: the run's phase in its 16 bytes differs
        buf = torch.from_numpy(np.full(total + dst_off + 16, SENTINEL[bits], {8: np.uint8, 16: np.uint16, 32: np.int32}[bits])).cuda()
        assert buf.data_ptr() % 16 == 0 and d_src.data_ptr() % 16 == 0
        d_out = buf[dst_off:dst_off + total]
    codec.frame_fit(d_src, fc, bits, out=d_out)
    got = d_out.cpu().numpy().astype(np.int64) & ((1 << bits) - 1)
    keep = np.ones(total, bool)
    for i, (first, n) in enumerate(comps):
        assert np.array_equal(got[first:first + n], want[i]), (bits, signed, i, fc[i])
        keep[first:first + n] = False
    assert (got[keep] == SENTINEL[bits]).all(), "written outside a run"
    if not in_place:
        assert np.array_equal(d_src.cpu().numpy(), src)         # the source is only read
        whole = buf.cpu().numpy().astype(np.int64) & ((1 << bits) - 1)
        assert (whole[:dst_off] == SENTINEL[bits]).all() and (whole[dst_off + total:] == SENTINEL[bits]).all()


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_every_count_at_every_start(bits, signed):
    counts = [n for n in COUNTS for _ in range(4)]
    starts = [s for _ in COUNTS for s in range(4)]
    run_case(bits, signed, counts, starts)


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_a_run_longer_than_one_turn_of_the_loop(bits):
    counts = [LONG] + [n for n in COUNTS for _ in range(4)] + [LONG + 1] * 15      # 48 components, signs alternating
    starts = [1] + [s for _ in COUNTS for s in range(4)] + [(3 * i) % 4 for i in range(15)]
    assert len(counts) == 48
    run_case(bits, None, counts, starts, seed=2)


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("bits", [8, 16])
def test_a_destination_two_bytes_off_goes_sample_by_sample(bits, signed):
    counts = [n for n in COUNTS for _ in range(4)] + [LONG // 16]
    starts = [s for _ in COUNTS for s in range(4)] + [2]
    run_case(bits, signed, counts, starts, dst_off=2 // (bits // 8), seed=3)


def test_a_32_bit_destination_one_element_off():
    counts = [n for n in COUNTS for _ in range(4)]
    starts = [s for _ in COUNTS for s in range(4)]
    run_case(32, None, counts, starts, dst_off=1, seed=4)


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
def test_in_place_at_32_bits(signed):
    counts = [n for n in COUNTS for _ in range(4)] + [LONG // 4]
    starts = [s for _ in COUNTS for s in range(4)] + [3]
    run_case(32, signed, counts, starts, in_place=True, seed=5)


def test_refusals():
    import ctypes as C
    import torch
    from openjph_amd import capi, codec
    src = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    d = codec.to_device(np.zeros(1, codec.fit_comp_dtype))
    f = capi.lib().ojphgpu_frame_fit
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert f(None, p(src), p(out), 12, p(d), 1) == capi.E_INVALID            # no such container
    assert f(None, p(src), p(src), 16, p(d), 1) == capi.E_INVALID            # in place only at 32 bits
    assert f(None, p(src), p(out, 2), 32, p(d), 1) == capi.E_INVALID         # a container off its natural alignment
    assert f(None, p(src), p(out, 1), 16, p(d), 1) == capi.E_INVALID
    assert f(None, None, p(out), 32, p(d), 1) == capi.E_INVALID
    assert f(None, p(src), p(out), 32, p(d), 0) == capi.OK                   # nothing to do
    # a component that is no fit (a shift beyond 31, an empty range) is left alone
    out.fill_(7)
    src.fill_(5)
    codec.frame_fit(src, [(0, 32, 40, 0, 255), (32, 32, 0, 9, 3)], 32, out=out)
    assert (out.cpu().numpy() == 7).all()
