"""What the GPU tests of the three video families share (tests/test_gpu_video.py: 4:2:2, test_gpu_video420.py, test_gpu_video444.py,
test_gpu_pipe_handover.py): arrays on their way to the device, surfaces with a pitch and guards around them, plans whose chroma
planes are a cell smaller than the luma plane, and frames through the plain codec objects."""
import numpy as np

GUARD = 256                 # bytes of the fill pattern in front of and behind every destination
FILL = 0x5A
C422, C420 = (2, 1), (2, 2)   # the chroma cells: a chroma sample covers that many luma samples (x, y)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def pitched(rows, pitch, rng=None):
    """[n, row_bytes] -> the bytes of a buffer of that pitch (None: tight) up to the end of its last row; the slack: FILL, or
    random bytes"""
    n, row = rows.shape
    if pitch is None:
        return rows.reshape(-1)
    out = np.full((n, pitch), FILL, np.uint8) if rng is None else rng.integers(0, 256, (n, pitch)).astype(np.uint8)
    out[:, :row] = rows
    return out.reshape(-1)[: pitch * (n - 1) + row]


def guarded_bytes(content, front=GUARD):
    """-> the bytes of a tensor that holds `content` between guards of FILL"""
    return np.concatenate([np.full(front, FILL, np.uint8), content, np.full(GUARD, FILL, np.uint8)])


def make_plan(w, h, depth, rev, cell=(1, 1), **kw):
    """a plan of three components (num_comps=: of that many) whose chroma planes are `cell` smaller than the luma plane
    (downsampling=: as given instead)"""
    from openjph_amd.plan import Plan, make_params
    kw.setdefault("downsampling", None if cell == (1, 1) else [(1, 1), cell, cell])
    return Plan(make_params(w, h, kw.pop("num_comps", 3), bit_depth=depth, reversible=rev, **kw))


def edged_planes(seed, w, h, depth, cell=(1, 1)):
    """blocks of 0 and 2^depth - 1: a lossy decode of them leaves the range"""
    rng = np.random.default_rng(seed)
    out = []
    for sx, sy in ((1, 1), cell, cell):
        ww, hh = -(-w // sx), -(-h // sy)
        a = np.where(rng.integers(0, 2, (hh // 2 + 1, ww // 3 + 1)) == 1, (1 << depth) - 1, 0)
        out.append(np.kron(a, np.ones((2, 3), int))[:hh, :ww].astype(np.int32))
    return out


def feed_planes(pipe, planes):
    buf = pipe.acquire()
    buf[...] = pipe.plan.pack_frame(planes).reshape(buf.shape)
    pipe.submit()


def decoded_planes(cs, **view):
    from openjph_amd import codec
    dec = codec.Decoder(cs, **view)
    return dec.plan.unpack_frame(dec.decode())
