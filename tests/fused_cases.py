"""Inputs and expectations for the fused block decoder's stage entry (ojphgpu_ht_decode_fused), shared by
tests/test_cpu_fused_cases.py (the net is sound) and tests/test_gpu_fused_geometry.py (the kernel under every geometry).

numpy + the oracle only.  A seeded POOL of code-blocks is coded once per process with the oracle's encoder; what a block
decodes to -- verdict and samples -- is the oracle's decoder's answer on the very bytes the GPU gets, damaged ones included.
A launch (Launch) is a list of pool entries laid out in one coefficient buffer with odd gaps, their bytes concatenated without
padding.  How a launch of n blocks on `cus` compute units is dealt out is asked of ojphgpu_ht_decode_fused_shape (shape_of),
never restated here."""
import numpy as np

SENTINEL = 0x5A5A5A5A
WIDTHS = (1, 2, 3, 5, 17, 31, 32, 33, 63, 64)
DELTA = 0.37 / (1 << 20)

# (n, cus) of the geometry launches.  Under the default shape (256 blocks per step-1 workgroup, 12-wavefront workgroups, two per
# CU) they give per_wave 1..8 -- (13, 1) 2, (26, 1) 3, (39, 1) 4, (51, 1) and (515, 6) 5, (61, 1) 6, (75, 1) 7, (99, 1), (123, 1)
# and (599, 3) 8, the last capped, on seven worker workgroups with n1 == cus == 3 -- each with wavefronts short of per_wave, a
# second step-1 workgroup with one live lane (257), n1 1, 2, 3 and a refusal (257, 1).  Under OJPHGPU_FUSED_SHAPE=0 (128 blocks
# per step-1 workgroup, 8 wavefronts, four per CU) the same table gives per_wave 1..6 -- all that shape can reach: an able launch
# has n <= 128 cus blocks on at least 24 cus worker wavefronts -- with (129, 5) as the one-live-lane case, n1 up to 5, and (599, 3)
# refused as well.  tests/test_cpu_fused_cases.py asserts all of this through the shape function.
GEOMETRY = ((1, 1), (7, 2), (64, 8), (65, 8), (256, 8), (257, 8), (13, 1), (26, 1), (39, 1), (51, 1), (61, 1), (75, 1), (99, 1),
            (123, 1), (129, 5), (259, 4), (515, 6), (599, 3), (257, 1))
SLICE_QH = tuple(range(1, 21)) + (23, 24, 25, 31, 32, 33, 64, 512)
SETTINGS = {"default": {}, "shape0": {"OJPHGPU_FUSED_SHAPE": "0"}, "rings1": {"OJPHGPU_FUSED_RINGS": "1"}}


def _ob():
    from oracle import oraclebind as ob
    return ob


def shape_of(n, cus):
    from openjph_amd import codec
    return codec.ht_decode_fused_shape(n, cus)


def slices_of(max_h):
    from openjph_amd import codec
    return codec.ht_decode_fused_slices(max_h)


class Entry:
    """one pool block: descriptor fields, the coded bytes as the GPU gets them, the oracle's verdict and samples"""

    def __init__(self, kind, w, h, kmax, mm, data, num_passes=1, len1=None, damaged=False):
        self.kind, self.w, self.h, self.kmax, self.mm, self.data, self.num_passes = kind, w, h, kmax, mm, bytes(data), num_passes
        self.len1 = len(self.data) if len1 is None else len1
        self.damaged = damaged
        self.coded = w > 0 and h > 0 and self.len1 > 0 and num_passes > 0
        self.ok, self.dec = True, None
        if self.coded:
            self.ok, dec = _ob().ht_decode(self.data, w, h, w, mm)
            self.dec = dec if self.ok else None
        self._exp = {}

    @property
    def scup(self):
        return (self.data[self.len1 - 1] << 4) + (self.data[self.len1 - 2] & 15) if self.len1 >= 2 else 0

    @property
    def passes_first_test(self):
        """what the reference tests before it touches the block (lengths, missing_msbs, Scup) lets this segment through"""
        return self.coded and self.len1 >= 2 and self.mm < 30 and 2 <= self.scup <= min(self.len1, 4079)

    @property
    def early_refused(self):
        return self.coded and not self.ok and not self.passes_first_test

    @property
    def late_refused(self):
        return self.coded and not self.ok and self.passes_first_test

    @property
    def magsgn(self):
        return self.data[:self.len1 - self.scup] if self.passes_first_test else b""

    def expect(self, rev):
        """int32 words [h, w] the coefficient buffer holds after the launch (float32 bit patterns when not rev)"""
        if rev not in self._exp:
            if self.dec is None:
                e = np.zeros((self.h, self.w), np.int32)
            elif rev:
                e = _ob().dequant_rev(self.dec, self.kmax)
            else:
                e = _ob().dequant_irv(self.dec, DELTA).view(np.int32)
            self._exp[rev] = np.ascontiguousarray(e)
        return self._exp[rev]


def _samples(rng, w, h, kmax, dens, amp):
    v = (rng.integers(-amp, amp + 1, size=(h, w)) * (rng.random((h, w)) < dens)).astype(np.int64)
    return (((v < 0).astype(np.uint64) << 31) | (np.abs(v).astype(np.uint64) << (31 - kmax))).astype(np.uint32), v


def _coded(rng, kind, w, h, kmax, dens, amp, mm=None, decl_k=None):
    sm, _ = _samples(rng, w, h, kmax, dens, amp)
    data = _ob().ht_encode(sm, w, h, w, kmax - 1, 0)
    return Entry(kind, w, h, kmax if decl_k is None else decl_k, kmax - 1 if mm is None else mm, data)


_POOL = {}


def pool(max_h=64):
    """the block pool for launches whose tallest block has max_h rows (geometry and sequence launches: 64)"""
    if max_h in _POOL:
        return _POOL[max_h]
    rng = np.random.default_rng(20240 + max_h)
    P = []
    hs = lambda: int(rng.integers(1, max_h + 1))
    # every K_max with missing_msbs = K_max - 1, every width, densities and amplitudes from sparse ones to full
    for kmax in range(1, 31):
        for j in range(5):
            w = WIDTHS[(kmax * 5 + j) % len(WIDTHS)]
            h = max_h if j == 0 else hs()
            dens = (0.002, 0.2, 1.0, 1.0, 0.2)[j]
            amp = (1, (1 << kmax) - 1, (1 << kmax) - 1, max(1, (1 << kmax) >> 1), 1)[j]
            P.append(_coded(rng, "plain", w, h, kmax, dens, amp))
    # density 0: coded although nothing is significant
    for j in range(6):
        P.append(_coded(rng, "plain", WIDTHS[j + 2], hs(), 5 + j, 0.0, 1))
    # the first block of a launch: a coded segment shorter than 34 bytes (bytewise tail loads at data_off 0)
    for j in range(8):
        e = _coded(rng, "tiny", 1 + j % 3, 1 + j % 4, 3 + j, 1.0, 3)
        assert 2 <= e.len1 < 34 and e.ok
        P.append(e)
    # full density, full amplitude: MagSgn strings that wrap the 1 KB ring many times; more of them until 0xFF stands just
    # before a 256-byte chunk boundary in 16 places
    big = 0
    while big < 36 or (boundary_ff(P) < 16 and big < 160):
        P.append(_coded(rng, "big", 64 if big % 4 else 63, max_h if big % 3 else max_h - 1, 30 - big % 7, 1.0, (1 << (30 - big % 7)) - 1))
        big += 1
    # missing_msbs 28..30 (30: refused before anything is read)
    for mm in (28, 29, 30):
        for j in range(4):
            kmax = min(mm + 1, 30)
            P.append(_coded(rng, "mm", WIDTHS[(3 * mm + j) % len(WIDTHS)], hs(), kmax, (0.2, 1.0)[j % 2], (1 << kmax) - 1, mm=mm, decl_k=mm + 1))
    # fewer missing_msbs declared than the block was coded with: exponents beyond missing_msbs + 2 appear somewhere down the
    # block, the oracle says where
    for j in range(24):
        kmax = int(rng.integers(6, 28))
        P.append(_coded(rng, "short-mm", WIDTHS[j % len(WIDTHS)], max(hs(), 8), kmax, (0.05, 0.6)[j % 2], (1 << kmax) - 1, mm=kmax - 1 - (1 + j % 3)))
    # not coded, and descriptors without samples
    some = _coded(rng, "plain", 17, 9, 9, 0.5, 100).data
    for j in range(6):
        P.append(Entry("uncoded", WIDTHS[j], hs(), 8, 7, b"", num_passes=1))
        P.append(Entry("uncoded", WIDTHS[9 - j], hs(), 8, 7, some, num_passes=0))
    for j in range(4):
        P.append(Entry("empty", 0 if j % 2 else 13, 11 if j % 2 else 0, 8, 7, some if j < 2 else b"", num_passes=1))
    # damaged segments, the oracle's verdict on each
    bases = [_coded(rng, "plain", 64, max_h, 11, 0.5, 700), _coded(rng, "plain", 33, max(max_h - 3, 1), 17, 1.0, 90000),
             _coded(rng, "plain", 17, max_h, 6, 0.3, 40), _coded(rng, "plain", 64, max(max_h // 2, 1), 24, 1.0, (1 << 24) - 1)]
    for j in range(24):                                      # truncated
        b = bases[j % 4]
        cut = (0, 1, 2, 3)[j] if j < 4 else int(rng.integers(2, b.len1))
        if cut:
            P.append(Entry("cut", b.w, b.h, b.kmax, b.mm, b.data[:cut], damaged=True))
    for j in range(48):                                      # random byte flips
        b = bases[j % 4]
        d = bytearray(b.data)
        for _ in range(int(rng.integers(1, 5))):
            d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
        P.append(Entry("flip", b.w, b.h, b.kmax, b.mm, d, damaged=True))
    for j in range(96):                                      # flips in the MEL / VLC tail, the two length bytes intact
        b = bases[j % 4]
        d = bytearray(b.data)
        for _ in range(int(rng.integers(1, 4))):
            d[len(d) - 3 - int(rng.integers(0, min(200, len(d) - 2)))] = int(rng.integers(0, 256))
        P.append(Entry("tail", b.w, b.h, b.kmax, b.mm, d, damaged=True))
    _POOL[max_h] = P
    return P


def boundary_ff(entries):
    """places where the last byte of a 256-byte chunk of an accepted block's MagSgn part is 0xFF"""
    return sum(1 for e in entries if e.coded and e.ok for k in range(255, len(e.magsgn), 256) if e.magsgn[k] == 0xFF)


class Launch:
    """entries laid out for one launch: descs (dicts for openjph_amd.codec.cb_desc_dtype), data, the expected buffer"""

    def __init__(self, tag, entries, cus, rev):
        self.tag, self.entries, self.cus, self.rev, self.n = tag, list(entries), cus, rev, len(entries)
        self.descs, datas, self.rects = [], [], []
        off, doff = 3, 0
        for i, e in enumerate(self.entries):
            pitch = e.w + (i * 7) % 5                       # odd gaps: a stray store meets a neighbour or the sentinel
            self.descs.append(dict(coef_off=off, pitch=max(pitch, 1), w=e.w, h=e.h, K_max=e.kmax, reversible=1 if rev else 0,
                                   missing_msbs=e.mm, num_passes=e.num_passes, delta=DELTA, len1=e.len1, len2=0, data_off=doff))
            self.rects.append((off, max(pitch, 1)))
            datas.append(np.frombuffer(e.data, np.uint8))
            off += max(pitch, 1) * e.h + (i % 3)
            doff += len(e.data)
        self.size = off + 64
        self.data = np.concatenate(datas) if datas else np.zeros(0, np.uint8)
        self.max_h = max([e.h for e in self.entries] + [1])
        self.status = np.array([0 if e.ok else 1 for e in self.entries], np.uint8)

    def desc_array(self, dtype):
        a = np.zeros(self.n, dtype)
        for d, src in zip(a, self.descs):
            for k, v in src.items():
                d[k] = v
        return a

    def before(self):
        return np.full(self.size, SENTINEL, np.int32)

    def expected(self):
        """the whole coefficient buffer after the launch: the oracle's words in every rectangle, zeros in refused and
        uncoded blocks, the sentinel everywhere else"""
        buf = self.before()
        for e, (off, pitch) in zip(self.entries, self.rects):
            if e.w and e.h:
                np.lib.stride_tricks.as_strided(buf[off:], (e.h, e.w), (pitch * 4, 4))[...] = e.expect(self.rev)
        return buf

    def problems(self, status, got):
        """what differs from the oracle, as text (empty: nothing)"""
        out = []
        bad = np.nonzero((np.asarray(status) != 0) != (self.status != 0))[0]
        if len(bad):
            out.append("verdicts differ at blocks %s (kinds %s): GPU %s, oracle %s" % (
                bad[:8].tolist(), [self.entries[i].kind for i in bad[:8]], np.asarray(status)[bad[:8]].tolist(), self.status[bad[:8]].tolist()))
        want = self.expected()
        if not np.array_equal(got, want):
            diff = np.nonzero(got != want)[0]
            starts = np.array([r[0] for r in self.rects])
            named = []
            for ix in diff[:400]:
                i = int(np.searchsorted(starts, ix, side="right")) - 1
                e = self.entries[max(i, 0)]
                off, pitch = self.rects[max(i, 0)]
                y, x = divmod(int(ix) - off, pitch)
                where = "block %d (%s %dx%d K %d mm %d ok %s) row %d col %d" % (i, e.kind, e.w, e.h, e.kmax, e.mm, e.ok, y, x) \
                    if i >= 0 and y < e.h and x < e.w else "outside the rectangles, behind block %d" % i
                if not named or named[-1][0] != i:
                    named.append((i, where + ": 0x%08x, expected 0x%08x" % (int(got[ix]) & 0xFFFFFFFF, int(want[ix]) & 0xFFFFFFFF)))
            left = int((got[diff] == np.int32(SENTINEL)).sum())
            out.append("%d words differ (%d of them still the sentinel), first: %s" % (len(diff), left, "; ".join(w for _, w in named[:6])))
        return out


def _pick(P, pred):
    return [e for e in P if pred(e)]


def _fill(tag, n, cus, rev, seed, start):
    """n pool entries: a short coded block first, two refused / uncoded / late-refused / full-amplitude ones where there is room,
    then the pool in turn from position `start` of a fixed order (every entry comes up in some launch), shuffled.  What a
    launch holds depends on its arguments alone, not on which launches were built before it."""
    P = pool(64)
    rng = np.random.default_rng(seed)
    tiny = _pick(P, lambda e: e.kind == "tiny")
    first = tiny[int(rng.integers(0, len(tiny)))]
    rest = []
    if n >= 12:
        for pred in (lambda e: e.early_refused, lambda e: not e.coded and e.w and e.h, lambda e: e.late_refused,
                     lambda e: e.kind == "big" and e.ok):
            c = _pick(P, pred)
            rest += [c[int(k)] for k in rng.choice(len(c), 2, replace=False)]
    order = np.random.default_rng(99).permutation(len(P))
    while len(rest) < n - 1:
        rest.append(P[int(order[start % len(P)])])
        start += 1
    rest = [rest[int(k)] for k in rng.permutation(len(rest))][:max(n - 1, 0)]
    return Launch(tag, [first] + rest, cus, rev)


_CACHE = {}


def geometry_launches():
    if "geo" not in _CACHE:
        out, start = [], 0
        for i, (n, cus) in enumerate(GEOMETRY):              # (each launch goes on in the pool where the one before stopped)
            out.append(_fill("n %d cus %d %s" % (n, cus, "rev" if i % 2 == 0 else "irv"), n, cus, i % 2 == 0, 1000 + i, start))
            start += n
        _CACHE["geo"] = out
    return _CACHE["geo"]


def _late_refused(rng, w, h):
    """a block with fewer missing_msbs declared than it was coded with that passes the first test and that the oracle refuses"""
    for _ in range(64):
        kmax = int(rng.integers(8, 29))
        e = _coded(rng, "short-mm", w, h, kmax, 1.0, (1 << kmax) - 1, mm=kmax - 1 - int(rng.integers(3, 6)))
        if e.late_refused:
            return e
    raise AssertionError("no late-refused block of %dx%d" % (w, h))


def slice_launch(max_qh):
    """one small launch whose tallest block has max_qh quad rows: that block, and for every slice [lo, hi) of the schedule
    a block that ends on the cut hi and one that ends inside the slice, odd and even heights -- all of them coded and accepted
    by the oracle, so that every one is decoded to its last row -- filled up to 15 with blocks of random heights; beside them
    two uncoded blocks, two the first test refuses (a one-byte segment, missing_msbs 30) and two refused late"""
    key = ("slice", max_qh)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(5000 + max_qh)
    max_h = 2 * max_qh - (max_qh % 2)
    bounds = slices_of(max_h)
    qhs = [max_qh]
    for lo, hi in bounds:
        qhs.append(hi)
        if hi - lo > 1:
            qhs.append(lo + 1 + int(rng.integers(0, hi - lo - 1)))
    while len(qhs) < 15:                                     # (two blocks to a wavefront on one compute unit)
        qhs.append(int(rng.integers(1, max_qh + 1)))

    def shape(j, qh):
        h = max_h if j == 0 else min(2 * qh - (j % 2), max_h)
        ws = [w for w in WIDTHS if w * h <= 4096]
        return (min(64, 4096 // h) if j == 0 else ws[int(rng.integers(0, len(ws)))]), h

    ents = []
    for j, qh in enumerate(qhs):
        w, h = shape(j, qh)
        kmax = int(rng.integers(2, 31))
        e = _coded(rng, "plain", w, h, kmax, (1.0, 0.3)[j % 2], max(1, ((1 << kmax) - 1) >> (j % 3)))
        assert e.ok
        ents.append(e)
    good = ents[0]
    for j in range(2):
        w, h = shape(1 + j, int(rng.integers(1, max_qh + 1)))
        ents.append(Entry("uncoded", w, h, 8, 7, b"" if j else good.data, num_passes=j))
        w, h = shape(1 + j, int(rng.integers(1, max_qh + 1)))
        ents.append(_late_refused(rng, max(w, 2), h))
    ents.append(Entry("cut", good.w, good.h, good.kmax, good.mm, good.data[:1], damaged=True))
    ents.append(Entry("mm", good.w, good.h, 31, 30, good.data))
    order = [0] + [int(k) + 1 for k in rng.permutation(len(ents) - 1)]
    ents = [ents[k] for k in order]
    L = Launch("max_qh %d" % max_qh, ents, 1 if len(ents) <= 128 else 2, max_qh % 2 == 1)
    L.bounds, L.qhs = bounds, qhs
    _CACHE[key] = L
    return L


def sequences():
    """launches made one after the other on ONE scratch: large then small, both transfers, and blocks that are coded in one
    run and uncoded or refused at the same position in the next (and the other way round)"""
    if "seq" in _CACHE:
        return _CACHE["seq"]
    P = pool(64)
    gone = _pick(P, lambda e: not e.coded and e.w and e.h) + _pick(P, lambda e: e.early_refused) + _pick(P, lambda e: e.late_refused)
    clean = _pick(P, lambda e: e.coded and e.ok and not e.damaged)
    a = _fill("seq 0: n 300 cus 8 rev", 300, 8, True, 7001, 11)
    swapped = []
    for i, e in enumerate(a.entries):
        if i and i % 3 == 0:
            e = gone[i % len(gone)] if (e.coded and e.ok) else clean[i % len(clean)]
        swapped.append(e)
    runs = [a, Launch("seq 1: the same positions, coded <-> not, irv, cus 3", swapped, 3, False),
            _fill("seq 2: n 40 cus 2 irv", 40, 2, False, 7002, 311),
            Launch("seq 3: run 0 again, cus 5", a.entries, 5, True),
            _fill("seq 4: n 7 cus 8 rev", 7, 8, True, 7003, 351),
            Launch("seq 5: run 1 again, rev, cus 4", swapped, 4, True)]
    _CACHE["seq"] = runs
    return runs
