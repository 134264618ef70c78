"""Inputs and expectations for the separate block-decoder launches as a stage (openjph_amd.codec.ht_decode_separate: prep,
step 1, then ht_dec_step2_kernel<TX, WD> or ht_dec_step2_multi_kernel<TX, NB>), shared by tests/test_cpu_separate_cases.py (the
net is sound) and tests/test_gpu_separate_launches.py (every instantiation under every launch).

numpy + the oracle only, on the pieces of tests/fused_cases.py (Entry, _coded, Launch, pool(64) -- used, not changed: the fused
launches stay input for input what they are).  Three width CLASSES of code-blocks, each a seeded pool built by the recipe of
fused_cases.pool; a launch is a list of entries of ONE class and ONE transfer, so that ojphgpu_ht_decode_kinds says of it
exactly what the class says, and the step-2 kernel it runs under is chosen by valid coarsenings of that value alone (VARIANTS),
never by an environment switch.  Which kernel and which grids that gives is asked of ojphgpu_ht_decode_launches (launches_of),
never restated here."""
import numpy as np

from tests import fused_cases as fc
from tests.fused_cases import Entry, Launch, _coded

# the widths of a class (wide: 65..128 columns, w * h <= 4096)
CLASSES = {"w16": (1, 2, 3, 5, 7, 8, 15, 16), "w32": (1, 2, 3, 5, 7, 8, 15, 16, 17, 31, 32), "wide": (65, 66, 100, 127, 128)}
FULL = {"w16": (16, 15), "w32": (32, 31)}                   # widths of the full-amplitude blocks of the narrow classes
CHUNK = {"w16": 64, "w32": 128}                              # bytes step2_multi un-stuffs per call and segment: 4 x 16, 4 x 32
FF_BLOCKS = 8                                                # accepted blocks with 0xFF on a chunk's last byte, per narrow class
FULL_CAP = 400                                               # ... within this many full-amplitude blocks, or the pool fails

# kinds a caller may pass in place of the truthful one K (include/ojphgpu.h: set bit 6 / 7, clear bit 8, set both of bits 2
# and 3, set bit 1) and the step-2 kernel each gives a launch of that class under the default environment:
# (multi, TX or None for the launch's own, WD, NB)
VARIANTS = {
    "truth": (lambda k: k, {"w16": (1, None, 1, 4), "w32": (1, None, 1, 2), "wide": (0, None, 0, 1)}),
    "two": (lambda k: k | 128, {"w16": (1, None, 1, 2)}),
    "one": (lambda k: k | 64 | 128, {"w16": (0, None, 1, 1), "w32": (0, None, 1, 1)}),
    "one-any-width": (lambda k: k | 2, {"w16": (0, None, 0, 1), "w32": (0, None, 0, 1)}),
    "one-any-transfer": (lambda k: k | 12, {"w16": (0, 0, 1, 1), "w32": (0, 0, 1, 1)}),
    "one-any-both": (lambda k: k | 12 | 2, {"w16": (0, 0, 0, 1), "w32": (0, 0, 0, 1), "wide": (0, 0, 0, 1)}),
    "no-bit-8": (lambda k: k & ~256, {}),                    # (the sequences use it: the same kernel as "one")
}
# the n of a class's launches, each built for both transfers.  With 4 wavefronts to a workgroup and 1, 2 or 4 blocks to a
# wavefront a workgroup holds B = 4, 8 or 16 blocks, and the step-2 grid is ceil(n / B):
#   B  4: 1 -> 1, 26 -> 7, 29 -> 8, 33 -> 9, 63 and 64 -> 16, 65 -> 17
#   B  8: 1 -> 1, 51 -> 7, 63 and 64 -> 8, 65 -> 9, 121 -> 16, 129 -> 17     (last wavefront of two: one block in 1, 51, 63, ...)
#   B 16: 1 -> 1, 98 -> 7, 121 -> 8, 129 -> 9, 256 -> 16, 257 -> 17          (last wavefront of four: 1, 2 (26, 98), 3 (51, 63))
# and step 1 (64 CH blocks per workgroup) sees 1, 63, 64, 65, 256 and 257.  tests/test_cpu_separate_cases.py asserts all of this
# through ojphgpu_ht_decode_launches.
N = {"w16": (1, 26, 29, 33, 51, 63, 64, 65, 98, 121, 129, 256, 257), "w32": (1, 26, 29, 33, 51, 63, 64, 65, 121, 129),
     "wide": (1, 26, 29, 33, 63, 64, 65)}
GRIDS = (1, 7, 8, 9, 16, 17)
STEP1_N = (1, 63, 64, 65, 256, 257)
# (class, n or "mixed", rev) of every launch of the GPU file, in the order of launches()
TABLE = tuple((c, n, rev) for c in ("w16", "w32", "wide") for n in N[c] for rev in (True, False)) + \
    tuple((c, "mixed", rev) for c in ("w16", "w32") for rev in (True, False))
SETTINGS = {"default": {}, "s1ch1": {"OJPHGPU_S1_CH": "1"}, "s1ch2": {"OJPHGPU_S1_CH": "2"}, "prep": {"OJPHGPU_DEC_PREP": "1"},
            "dual2": {"OJPHGPU_DEC_DUAL": "2"}}
KNOBS = ("OJPHGPU_S1_CH", "OJPHGPU_DEC_PREP", "OJPHGPU_DEC_DUAL")


def launches_of(n, kinds):
    from openjph_amd import codec
    return codec.ht_decode_launches(n, kinds)


def variants_of(cls):
    return [v for v, (_, by) in VARIANTS.items() if cls in by]


def truth_of(entries, rev):
    """the kinds of a launch as its class and transfer state them (what ojphgpu_ht_decode_kinds must say of its descriptors)"""
    k = 256 | (4 if rev else 8)
    for e in entries:
        k |= (2 if e.w > 64 else 1) | (64 if e.w > 32 else 0) | (128 if e.w > 16 else 0)
    return k


def ff_places(m, chunk):
    """places where the last byte of a `chunk`-byte piece of the MagSgn bytes m is 0xFF and more bytes follow: the next call
    of the un-stuffer starts behind an 0xFF that the call before saw"""
    return sum(1 for k in range(chunk - 1, len(m) - 1, chunk) if m[k] == 0xFF)


def chunk_ff(e, chunk):
    return ff_places(e.magsgn, chunk) if e.coded and e.ok else 0


def ff_blocks(entries, chunk):
    return sum(1 for e in entries if chunk_ff(e, chunk))


_POOL = {}


def pool(cls):
    """the block pool of a class, by the recipe of fused_cases.pool; the blocks of fused_cases.pool(64) that fit the class
    are part of it"""
    if cls in _POOL:
        return _POOL[cls]
    W = CLASSES[cls]
    rng = np.random.default_rng(31000 + len(W))
    top = lambda w: min(64, 4096 // w)
    hs = lambda w: int(rng.integers(1, top(w) + 1))
    P = []
    # every K_max with missing_msbs = K_max - 1, every width, densities and amplitudes from sparse ones to full
    for kmax in range(1, 31):
        for j in range(5):
            w = W[(kmax * 5 + j) % len(W)]
            h = top(w) if j == 0 else hs(w)
            dens = (0.002, 0.2, 1.0, 1.0, 0.2)[j]
            amp = (1, (1 << kmax) - 1, (1 << kmax) - 1, max(1, (1 << kmax) >> 1), 1)[j]
            P.append(_coded(rng, "plain", w, h, kmax, dens, amp))
    # heights 1 and 64 (the tallest of the width) and K_max 1 and 30 at full density, for the mixed wavefronts
    for j in range(4):
        w = W[-1 - j % 2]
        P.append(_coded(rng, "plain", w, 1, 9 + j, 1.0, 300))
        P.append(_coded(rng, "plain", w, top(w), 9 + j, 1.0, 300))
        P.append(_coded(rng, "plain", w, hs(w), 1, 1.0, 1))
        P.append(_coded(rng, "plain", w, hs(w), 30, 1.0, (1 << 30) - 1))
    if cls != "wide":
        for j in range(4):
            P.append(_coded(rng, "plain", 1, 1, 2 + j, 1.0, 3))
    # density 0: coded although nothing is significant
    for j in range(6):
        w = W[(j + 2) % len(W)]
        P.append(_coded(rng, "plain", w, hs(w), 5 + j, 0.0, 1))
    # the first block of a launch: a coded segment shorter than 34 bytes (bytewise tail loads at data_off 0)
    tiny = 0
    for j in range(400):
        if tiny == 8:
            break
        # (of a width that is the class's own: a launch of this one block is truthfully of its class)
        e = _coded(rng, "tiny", 1 + j % 3, 1 + j % 4, 3 + j % 8, 1.0, 3) if cls == "w16" else \
            _coded(rng, "tiny", W[-1 - j % 3], 1 + j % 3, 3 + j % 8, 0.04 if cls == "w32" else 0.02, 1)
        if 2 <= e.len1 < 34 and e.ok:
            P.append(e)
            tiny += 1
    assert tiny == 8, "class %s: %d segments under 34 bytes" % (cls, tiny)
    # full density, full amplitude, the widest blocks of a narrow class: more of them until 0xFF is the last byte of an
    # un-stuffing chunk in FF_BLOCKS accepted blocks of the class
    if cls in FULL:
        big = 0
        while big < 12 or ff_blocks(P, CHUNK[cls]) < FF_BLOCKS:
            if big >= FULL_CAP:
                raise AssertionError("class %s: %d blocks with 0xFF at the end of a %d-byte chunk after %d full-amplitude blocks" % (
                    cls, ff_blocks(P, CHUNK[cls]), CHUNK[cls], big))
            P.append(_coded(rng, "big", FULL[cls][1 if big % 4 == 0 else 0], 64 if big % 3 else 63, 30 - big % 7, 1.0, (1 << (30 - big % 7)) - 1))
            big += 1
    # missing_msbs 28..30 (30: refused before anything is read)
    for mm in (28, 29, 30):
        for j in range(4):
            kmax = min(mm + 1, 30)
            w = W[(3 * mm + j) % len(W)]
            P.append(_coded(rng, "mm", w, hs(w), kmax, (0.2, 1.0)[j % 2], (1 << kmax) - 1, mm=mm, decl_k=mm + 1))
    # fewer missing_msbs declared than the block was coded with: the oracle says where the block stops being decodable
    for j in range(24):
        kmax = int(rng.integers(6, 28))
        w = W[j % len(W)]
        P.append(_coded(rng, "short-mm", w, min(max(hs(w), 8), top(w)), kmax, (0.05, 0.6)[j % 2], (1 << kmax) - 1, mm=kmax - 1 - (1 + j % 3)))
    # not coded, and descriptors without samples
    some = _coded(rng, "plain", W[-1], 9, 9, 0.5, 100).data
    for j in range(6):
        w, v = W[j % len(W)], W[-1 - j % len(W)]
        P.append(Entry("uncoded", w, hs(w), 8, 7, b"", num_passes=1))
        P.append(Entry("uncoded", v, hs(v), 8, 7, some, num_passes=0))
    for j in range(4):
        P.append(Entry("empty", 0 if j % 2 else W[-2], 11 if j % 2 else 0, 8, 7, some if j < 2 else b"", num_passes=1))
    # damaged segments on bases of the class, the oracle's verdict on each
    a, b, c = W[-1], W[-2], W[len(W) // 2]
    bases = [_coded(rng, "plain", a, top(a), 11, 0.5, 700), _coded(rng, "plain", b, max(top(b) - 3, 1), 17, 1.0, 90000),
             _coded(rng, "plain", c, top(c), 6, 0.3, 40), _coded(rng, "plain", a, max(top(a) // 2, 1), 24, 1.0, (1 << 24) - 1)]
    for j in range(24):                                      # truncated
        s = bases[j % 4]
        cut = (0, 1, 2, 3)[j] if j < 4 else int(rng.integers(2, s.len1))
        if cut:
            P.append(Entry("cut", s.w, s.h, s.kmax, s.mm, s.data[:cut], damaged=True))
    for j in range(48):                                      # random byte flips
        s = bases[j % 4]
        d = bytearray(s.data)
        for _ in range(int(rng.integers(1, 5))):
            d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
        P.append(Entry("flip", s.w, s.h, s.kmax, s.mm, d, damaged=True))
    for j in range(96):                                      # flips in the MEL / VLC tail, the two length bytes intact
        s = bases[j % 4]
        d = bytearray(s.data)
        for _ in range(int(rng.integers(1, 4))):
            d[len(d) - 3 - int(rng.integers(0, min(200, len(d) - 2)))] = int(rng.integers(0, 256))
        P.append(Entry("tail", s.w, s.h, s.kmax, s.mm, d, damaged=True))
    # what fused_cases.pool(64) holds of these widths (the same objects: their expectations are shared)
    lo, hi = (65, 128) if cls == "wide" else (0, max(W))
    P += [e for e in fc.pool(64) if lo <= e.w <= hi and e.kind != "tiny"]
    assert all(e.w <= max(W) and e.w * e.h <= 4096 for e in P)
    _POOL[cls] = P
    return P


def _pick(P, pred):
    return [e for e in P if pred(e)]


def _launch(tag, cls, entries, rev):
    L = Launch(tag, entries, 0, rev)
    L.cls, L.truth = cls, truth_of(entries, rev)
    L._want = None
    return L


def expected(L):
    """Launch.expected, computed once per launch"""
    if L._want is None:
        L._want = L.expected()
        L._want.setflags(write=False)
    return L._want


def _fill(tag, cls, n, rev, seed, start):
    """n entries of the class's pool, as fused_cases._fill deals them: a short coded block first, two refused / uncoded /
    late-refused / full-amplitude ones where there is room, then the pool in turn from position `start` of a fixed order,
    shuffled.  What a launch holds depends on its arguments alone."""
    P = pool(cls)
    rng = np.random.default_rng(seed)
    tiny = _pick(P, lambda e: e.kind == "tiny")
    first = tiny[int(rng.integers(0, len(tiny)))]
    rest = []
    if n >= 12:
        for pred in (lambda e: e.early_refused, lambda e: not e.coded and e.w and e.h, lambda e: e.late_refused,
                     lambda e: e.ok and (e.kind == "big" or (cls == "wide" and len(e.magsgn) > 2048))):
            c = _pick(P, pred)
            rest += [c[int(k)] for k in rng.choice(len(c), 2, replace=False)]
    order = np.random.default_rng(77).permutation(len(P))
    taken = max(n - 1 - len(rest), 0)
    rest += [P[int(order[(start + j) % len(P)])] for j in range(taken)]
    rest = [rest[int(k)] for k in rng.permutation(len(rest))][:max(n - 1, 0)]
    L = _launch(tag, cls, [first] + rest, rev)
    L.taken = taken
    return L


def mixed_groups(cls):
    """the hand-ordered wavefronts: lists of four entries that one wavefront of four (and, as two pairs, two wavefronts of two)
    decodes together, with the name of what each is there for"""
    P = pool(cls)
    wmax = max(CLASSES[cls])
    wide_first = lambda c: sorted(c, key=lambda e: -e.w)     # (stable: the widest blocks of the class first)
    acc = wide_first(_pick(P, lambda e: e.coded and e.ok and not e.damaged and e.kind == "plain" and e.expect(True).any()))
    h1, h64 = [e for e in acc if e.h == 1], [e for e in acc if e.h == 64]
    k1, k30 = [e for e in acc if e.kmax == 1], [e for e in acc if e.kmax == 30 and e.mm == 29]
    early, late = wide_first(_pick(P, lambda e: e.early_refused)), wide_first(_pick(P, lambda e: e.late_refused))
    unc = wide_first(_pick(P, lambda e: not e.coded and e.w and e.h))
    big = _pick(P, lambda e: e.kind == "big" and e.ok)
    big30 = [e for e in big if e.kmax == 30]
    one = _pick(P, lambda e: e.coded and e.ok and e.w == 1 and e.h == 1 and e.kind == "plain")
    tiny = _pick(P, lambda e: e.kind == "tiny")
    ffb = _pick(P, lambda e: chunk_ff(e, CHUNK[cls]))
    assert min(len(x) for x in (h1, h64, k1, k30, early, late, unc, big, big30, one, tiny, ffb)) >= 2 and acc[0].w == wmax
    G = [("first", [tiny[0], h64[0], h1[0], h64[1]]),
         ("heights 1 and 64", [h1[0], h64[0], h64[1], h1[1]]),
         ("K_max 1 and 30", [k1[0], k30[0], k30[1], k1[1]]),
         ("early, late, uncoded, accepted", [early[0], late[0], unc[0], acc[0]]),
         ("accepted, uncoded, late, early", [acc[1], unc[1], late[1], early[1]]),
         ("four big", [big[0], big[1], big[2], big[3]]),
         ("K_max 30 full amplitude beside 1 x 1", [big30[0], one[0], one[1], big30[1]]),
         ("0xFF at a chunk end beside short blocks", [ffb[0], h1[1], tiny[1], ffb[1]]),
         ("nothing decodes", [early[2 % len(early)], unc[2 % len(unc)], early[3 % len(early)], unc[3 % len(unc)]]),
         ("all refused late", [late[j % len(late)] for j in range(2, 6)])]
    for pos in range(4):                                     # a refused block at every segment position, its neighbours accepted
        for r, name in ((early, "early"), (late, "late")):
            g = [acc[(2 + 3 * pos + j) % len(acc)] for j in range(4)]
            g[pos] = r[pos % len(r)]
            G.append(("%s-refused at position %d" % (name, pos), g))
    G.append(("a last wavefront of three", [late[0], h64[0], acc[2]]))
    return G


_CACHE = {}


def launches():
    """every launch of TABLE"""
    if "all" not in _CACHE:
        out, start = [], {c: 0 for c in CLASSES}
        for i, (cls, n, rev) in enumerate(TABLE):
            tag = "%s %s %s" % (cls, n, "rev" if rev else "irv")
            if n == "mixed":
                out.append(_launch(tag, cls, [e for _, g in mixed_groups(cls) for e in g], rev))
                out[-1].groups = mixed_groups(cls)
            else:
                out.append(_fill(tag, cls, n, rev, 2000 + i, start[cls]))
                start[cls] += out[-1].taken                  # (each launch goes on in the pool where the one before stopped)
        _CACHE["all"] = out
    return _CACHE["all"]


def sequences():
    """(launch, variant) runs made one after the other on ONE SeparateScratch: large then small, both transfers, four blocks
    to a wavefront, then one, then four again, a wide launch between narrow ones, and blocks that are coded in one run and
    uncoded or refused at the same position in the next (and the other way round), as fused_cases.sequences does it"""
    if "seq" in _CACHE:
        return _CACHE["seq"]
    P = pool("w16")
    gone = _pick(P, lambda e: not e.coded and e.w and e.h) + _pick(P, lambda e: e.early_refused) + _pick(P, lambda e: e.late_refused)
    clean = _pick(P, lambda e: e.coded and e.ok and not e.damaged)
    a = _fill("seq 0: w16 n 257 rev", "w16", 257, True, 9001, 5)
    swapped = []
    for i, e in enumerate(a.entries):
        if i and i % 3 == 0:
            e = gone[i % len(gone)] if (e.coded and e.ok) else clean[i % len(clean)]
        swapped.append(e)
    runs = [(a, "truth"),
            (_launch("seq 1: the same positions, coded <-> not, irv", "w16", swapped, False), "no-bit-8"),
            (_fill("seq 2: w32 n 40 irv", "w32", 40, False, 9002, 211), "truth"),
            (_launch("seq 3: run 0 again", "w16", a.entries, True), "truth"),
            (_fill("seq 4: wide n 7 rev", "wide", 7, True, 9003, 17), "truth"),
            (_launch("seq 5: run 1 again, rev", "w16", swapped, True), "two")]
    _CACHE["seq"] = runs
    return runs
