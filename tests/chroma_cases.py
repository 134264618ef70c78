"""What the CPU and the GPU tests of the chroma stage share (tests/test_cpu_rechroma.py: the numpy rule and the plan judgement
without a device; tests/test_gpu_rechroma.py: the kernel; tests/test_gpu_rechroma_pipe.py: the pipes)."""
import numpy as np

from openjph_amd import pipeline

CELLS = ((1, 1), (2, 1), (2, 2), (1, 2))                # 4:4:4, 4:2:2, 4:2:0, 4:4:0
# every (source cell, destination cell): per direction same / halve / double -- the nine pairings of the two directions'
# modes, the unchanged direction at both of its factors
PAIRS = tuple((s, d) for s in CELLS for d in CELLS)
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.int32}
RGB_NAMES = ("bgra", "rgba", "argb", "r210", "r10k")
YCC_FORMATS = tuple(n for n in pipeline._VIDEO_TABLE if n not in RGB_NAMES)


def plane_shapes(w, h, cell):
    return [(h, w)] + [(-(-h // cell[1]), -(-w // cell[0]))] * 2


def random_planes(rng, w, h, cell, bits):
    """three planes of a w x h frame as `bits`-bit containers hold them: unsigned, or int32 with negatives and the type's ends"""
    out = []
    for shape in plane_shapes(w, h, cell):
        if bits == 32:
            a = rng.integers(-2 ** 31, 2 ** 31, shape)
            ends = rng.integers(0, 8, shape)
            a = np.where(ends == 0, -2 ** 31, np.where(ends == 1, 2 ** 31 - 1, a))
        else:
            a = rng.integers(0, 1 << bits, shape)
        out.append(a.astype(DTYPES[bits]))
    return out


def plane_loop(q, s, d, w, h):
    """rechroma_plane as a plain double loop over the outputs, taps written out"""
    def taps(i, n, fs, fd):
        if fs == fd:
            return [(i, 1)]
        if fd == 2 * fs:
            return [(max(2 * i - 1, 0), 1), (2 * i, 2), (min(2 * i + 1, n - 1), 1)]
        return [(i // 2, 2)] if i % 2 == 0 else [((i - 1) // 2, 1), (min((i + 1) // 2, n - 1), 1)]
    hs, ws = len(q), len(q[0])
    wo, ho = -(-w // d[0]), -(-h // d[1])
    k = {0: 0, 1: 2, -1: 1}[(d[0] == 2 * s[0]) - (s[0] == 2 * d[0])] + {0: 0, 1: 2, -1: 1}[(d[1] == 2 * s[1]) - (s[1] == 2 * d[1])]
    out = [[0] * wo for _ in range(ho)]
    for j in range(ho):
        for i in range(wo):
            acc = 0
            for y, wy in taps(j, hs, s[1], d[1]):
                for x, wx in taps(i, ws, s[0], d[0]):
                    acc += wy * wx * int(q[y][x])
            out[j][i] = (acc + (1 << (k - 1))) >> k if k else acc
    return out


def unpack_any(buf, fmt, w, h, depth):
    """pipeline.unpack_video* of the format's family"""
    f = {(2, 1): pipeline.unpack_video, (2, 2): pipeline.unpack_video420, (1, 1): pipeline.unpack_video444}[pipeline.video_cell(fmt)]
    return f(buf, fmt, w, h, depth)


def pack_any(planes, fmt, depth):
    f = {(2, 1): pipeline.pack_video, (2, 2): pipeline.pack_video420, (1, 1): pipeline.pack_video444}[pipeline.video_cell(fmt)]
    return f(planes, fmt, depth)


def layout_any(fmt, w, h):
    """-> (rows, row_bytes) of the buffer as a pipe's view shows it"""
    cell = pipeline.video_cell(fmt)
    if cell == (2, 2):
        row, _, total = pipeline.video420_layout(fmt, w, h)
    else:
        row, total = (pipeline.video_layout if cell == (2, 1) else pipeline.video444_layout)(fmt, w, h)
    return total // row, row
