"""Host-side plan + Tier-2 wrappers over the C ABI (numpy views of the plan tables)."""
import ctypes as C
import numpy as np

from . import capi
from .capi import Params, BandInfo, BlockInfo, LevelInfo, CodedBlock, PaddedBlock, Run, check, PROG_ORDERS

band_dtype = np.dtype(BandInfo)
block_dtype = np.dtype(BlockInfo)
level_dtype = np.dtype(LevelInfo)
coded_dtype = np.dtype(CodedBlock)
padded_dtype = np.dtype(PaddedBlock)
run_dtype = np.dtype(Run)


def make_params(width, height, num_comps=1, bit_depth=8, is_signed=False, reversible=True,
                num_decomps=5, block=(64, 64), color_transform=False, tile=(0, 0),
                prog_order="RPCL", qstep=-1.0, precinct=(0, 0), tlm=False, precincts=None,
                downsampling=None, image_offset=(0, 0), tile_offset=(0, 0), tileparts="", bit_depths=None, signs=None,
                qfactor=0, coc=None, nlt=None, qfactors=None, atk=None, dfs=None, wavelet=0):
    """qfactors: {component: (ctype, qfactor)} with ctype "Y", "Cb" or "Cr" -- param_qcd::set_qfactor(comp_idx,
    ctype, qfactor) calls in the order of the dict (a QCC per named component).
    nlt: {component or "all": 0 or 3} -- param_nlt::set_nonlinear_transform calls in the order of the
    dict ("all" = the ALL_COMPS entry; 3 = binary complement <-> sign magnitude, 0 = none).
    coc: {component: dict(reversible=, num_decomps=, block=(w, h), precincts=[(w, h), ...])} -- COC
    marker segments in the order of the dict (param_cod's comp_idx setters); whatever a dict leaves
    out keeps the reference's COC defaults (9/7, 5 decompositions, 64x64, no precincts), NOT the COD's.
    Part 2 (the reference only READS these; this library also writes them, which is where the test codestreams come
    from): atk = {index 2..255: dict(steps=[(a, b, e), ...] for a reversible kernel or [A, ...] + K= for an irreversible
    one, synthesis order)} -- ATK marker segments; dfs = {index 0..15: [kind per decomposition level, 1 = the first one
    applied: 1 both directions, 2 horizontal, 3 vertical, 0 none]} -- DFS marker segments; wavelet = the ATK index the
    COD names (0: `reversible` decides); a coc entry may carry wavelet= and dfs= (a DFS index; the number of
    decompositions is then the COD's).
    width/height: the image SIZE (the reference's extent is offset + size); downsampling: list of
    (dx, dy) per component (param_siz::set_component), default 1,1; tileparts: "", "R", "C" or "RC"
    (codestream::set_tilepart_divisions); bit_depths / signs: per-component lists where they differ
    from bit_depth / is_signed; qfactor: 1..100 (param_qcd::set_qfactor), 0 = not set."""
    p = Params()
    p.width, p.height, p.num_comps = width, height, num_comps
    p.bit_depth, p.is_signed = bit_depth, int(is_signed)
    p.reversible, p.num_decomps = int(reversible), num_decomps
    p.block_w, p.block_h = block
    p.color_transform = int(color_transform)
    p.tile_w, p.tile_h = tile
    p.prog_order = PROG_ORDERS[prog_order] if isinstance(prog_order, str) else int(prog_order)
    p.qstep = float(qstep)
    p.precinct_w, p.precinct_h = precinct
    if precincts:                          # list of (w, h) from the lowest resolution up, last one repeated
        for i in range(num_decomps + 1):
            pw, ph = precincts[min(i, len(precincts) - 1)]
            p.precinct_exps[i] = (int(pw).bit_length() - 1) | ((int(ph).bit_length() - 1) << 4)
    p.tlm = int(tlm)
    p.reserved[1] = (1 if "R" in tileparts else 0) | (2 if "C" in tileparts else 0)
    p.reserved[2] = int(qfactor)
    for c, bd in enumerate(bit_depths or []):
        p.comp_depth[c] = int(bd)
    for c, sg in enumerate(signs or []):
        p.comp_sign[c] = 2 if sg else 1
    p.image_x0, p.image_y0 = image_offset
    p.tile_x0, p.tile_y0 = tile_offset
    p.wavelet = int(wavelet)
    for i, (idx, a) in enumerate((atk or {}).items()):
        k = p.atk[i]
        steps = a["steps"]
        k.index, k.num_steps = int(idx), len(steps)
        k.reversible = int(isinstance(steps[0], (tuple, list)))
        k.coeff_type = int(a.get("coeff_type", 1 if k.reversible else 2))
        k.K = float(a.get("K", 1.0))
        for j, st in enumerate(steps):
            if k.reversible:
                k.steps[j].a, k.steps[j].b, k.steps[j].e = [int(v) for v in st]
            else:
                k.steps[j].A = float(st)
    for i, (idx, kinds) in enumerate((dfs or {}).items()):
        f = p.dfs[i]
        f.used, f.index, f.num_levels = 1, int(idx), len(kinds)
        for j, kd in enumerate(kinds):
            f.types[j] = int(kd)
    for rank, (c, st) in enumerate((coc or {}).items()):
        if not 0 <= int(c) < 16:
            raise ValueError("per-component coding styles can be given for the first 16 components")
        k = p.coc[int(c)]
        k.rank = rank + 1
        k.reversible = int(bool(st.get("reversible", False)))
        k.num_decomps = int(st.get("num_decomps", 5))
        if st.get("dfs") is not None:
            k.reserved[0] |= 0x80 | (int(st["dfs"]) << 1)
        k.reserved[1] = int(st.get("wavelet", 0))
        bw, bh = st.get("block", (64, 64))
        k.log_block_w, k.log_block_h = int(bw).bit_length() - 1, int(bh).bit_length() - 1
        pl = st.get("precincts")
        if pl:
            k.has_precincts = 1
            for i in range(k.num_decomps + 1):
                pw, ph = pl[min(i, len(pl) - 1)]
                k.precinct_exps[i] = (int(pw).bit_length() - 1) | ((int(ph).bit_length() - 1) << 4)
    for rank, (c, (ctype, qf)) in enumerate((qfactors or {}).items()):
        if not 0 <= int(c) < 16:
            raise ValueError("per-component quality factors can be given for the first 16 components")
        p.qcc_qfactor[int(c)], p.qcc_ctype[int(c)], p.qcc_rank[int(c)] = int(qf), ("Y", "Cb", "Cr").index(ctype), rank + 1
    rank = 0
    for c, t in (nlt or {}).items():
        if int(t) not in (0, 3):
            raise ValueError("only the non-linearity types 0 and 3 exist in the reference")
        if c == "all":
            p.nlt_default = int(t) + 1
            continue
        if not 0 <= int(c) < 16:
            raise ValueError("NLT entries can be given for the first 16 components")
        if p.nlt_comp[int(c)] == 0:
            rank += 1
            p.nlt_rank[int(c)] = rank
        p.nlt_comp[int(c)] = int(t) + 1
    if downsampling:
        if len(downsampling) > 16:
            raise ValueError("sub-sampling factors can be given for the first 16 components")
        for c, (dx, dy) in enumerate(downsampling):
            p.comp_dx[c], p.comp_dy[c] = int(dx), int(dy)
    return p


class Plan:
    """Owns an ojphgpu_plan*. Tables are exposed as numpy structured arrays."""

    def __init__(self, params=None, handle=None, owned=True):
        self._lib = capi.lib()
        self._owned = owned                # False: the handle belongs to another object (a decoder pipe)
        if handle is None:
            h = C.c_void_p()
            check(self._lib.ojphgpu_plan_create(C.byref(params), C.byref(h)), "plan_create")
            handle = h
        self.handle = handle
        self.skip = (0, 0)
        self.region = None
        cnt = (C.c_uint64 * 8)()
        check(self._lib.ojphgpu_plan_counts(self.handle, cnt))
        (self.num_tiles, self.num_bands, self.num_blocks, self.num_levels, self.arena_elems,
         self.max_block_bytes, self.num_precincts, self.num_tcomps) = [int(v) for v in cnt]
        self.params = Params()
        check(self._lib.ojphgpu_plan_params(self.handle, C.byref(self.params)))
        ppt = C.c_uint32()
        check(self._lib.ojphgpu_plan_tile_parts(self.handle, C.byref(ppt)))
        self.parts_per_tile = int(ppt.value)
        self.bands = np.zeros(self.num_bands, band_dtype)
        self.blocks = np.zeros(self.num_blocks, block_dtype)
        self.levels = np.zeros(self.num_levels, level_dtype)
        if self.num_bands:
            check(self._lib.ojphgpu_plan_bands(self.handle, self.bands.ctypes.data, self.num_bands))
        if self.num_blocks:
            check(self._lib.ojphgpu_plan_blocks(self.handle, self.blocks.ctypes.data, self.num_blocks))
        if self.num_levels:
            check(self._lib.ojphgpu_plan_levels(self.handle, self.levels.ctypes.data, self.num_levels))

    def __del__(self):
        try:
            if self.handle and self._owned:
                self._lib.ojphgpu_plan_destroy(self.handle)
            self.handle = None
        except Exception:
            pass

    def set_comments(self, comments):
        """user COM segments of the main header: a list of str (Latin text, Rcom = 1) or bytes (Rcom = 0)"""
        n = len(comments)
        raw = [c.encode("latin-1") if isinstance(c, str) else bytes(c) for c in comments]
        data = (C.c_char_p * max(n, 1))(*raw)
        lens = (C.c_uint16 * max(n, 1))(*[len(b) for b in raw])
        rcom = (C.c_uint16 * max(n, 1))(*[1 if isinstance(c, str) else 0 for c in comments])
        check(self._lib.ojphgpu_plan_set_comments(self.handle, data, lens, rcom, n), "plan_set_comments")

    def restrict_resolution(self, skipped_res_for_data, skipped_res_for_recon=None):
        """codestream::restrict_input_resolution on a parsed plan (before a Decoder is created from it)"""
        if skipped_res_for_recon is None:
            skipped_res_for_recon = skipped_res_for_data
        check(self._lib.ojphgpu_plan_restrict_resolution(self.handle, int(skipped_res_for_data), int(skipped_res_for_recon)),
              "plan_restrict_resolution")
        self.skip = (int(skipped_res_for_data), int(skipped_res_for_recon))

    def restrict_region(self, x0, y0, w, h):
        """region decoding (ojphgpu_plan_restrict_region) on a parsed plan, after restrict_resolution if at all: a Decoder made
        from the plan decodes the rectangle (x0, y0, w, h) of the reference grid, relative to the image origin, and nothing
        else; comp_info / frame_shape then describe the region frame"""
        check(self._lib.ojphgpu_plan_restrict_region(self.handle, int(x0), int(y0), int(w), int(h)), "plan_restrict_region")
        self.region = (int(x0), int(y0), int(w), int(h))

    def region_blocks(self):
        """-> bool per block of the plan: decoded for the region (without a region: by a whole-frame decoder)"""
        out = np.zeros(self.num_blocks, np.uint8)
        if self.num_blocks:
            check(self._lib.ojphgpu_plan_region_blocks(self.handle, out.ctypes.data, self.num_blocks), "plan_region_blocks")
        return out.astype(bool)

    def upload_runs(self):
        """-> (runs, staged_len): what a view decoder of this parsed plan uploads (ojphgpu_plan_upload_runs) -- runs: run_dtype
        array (src = offset in the codestream, dst = place in the staged bytes, n), staged_len: the bytes staged"""
        n, staged = C.c_size_t(), C.c_uint64()
        check(self._lib.ojphgpu_plan_upload_runs(self.handle, None, 0, C.byref(n), C.byref(staged)), "plan_upload_runs")
        out = np.zeros(int(n.value), run_dtype)
        if n.value:
            check(self._lib.ojphgpu_plan_upload_runs(self.handle, out.ctypes.data, int(n.value), C.byref(n), C.byref(staged)), "plan_upload_runs")
        return out, int(staged.value)

    def comp_info(self, comp):
        """-> dict(x0, y0, w, h, frame_off, dx, dy) of component `comp` (see ojphgpu_plan_comp_info)"""
        out = (C.c_uint32 * 8)()
        check(self._lib.ojphgpu_plan_comp_info(self.handle, comp, out))
        v = [int(x) for x in out]
        return dict(x0=v[0], y0=v[1], w=v[2], h=v[3], frame_off=v[4] | (v[5] << 32), dx=v[6], dy=v[7])

    def comp_format(self, comp):
        """-> (bit depth, is_signed) of component `comp`"""
        bd, sg = C.c_uint32(), C.c_uint32()
        check(self._lib.ojphgpu_plan_comp_format(self.handle, comp, C.byref(bd), C.byref(sg)))
        return int(bd.value), bool(sg.value)

    def comp_style(self, comp):
        """coding style of component `comp` (its COC, else the COD): dict(num_decomps, reversible,
        log_block=(w, h), has_coc, recon_decomps = levels left after restrict_resolution, nlt3 = the type 3
        non-linearity applies, wide = the component takes the 64-bit sample path: int64 planes of two arena elements per
        sample)"""
        out = (C.c_uint32 * 8)()
        check(self._lib.ojphgpu_plan_comp_style(self.handle, comp, out))
        return dict(num_decomps=int(out[0]), reversible=bool(out[1]), log_block=(int(out[2]), int(out[3])),
                    has_coc=bool(out[4]), recon_decomps=int(out[5]), nlt3=bool(out[6]), wide=bool(out[7] & 1),
                    general=bool(out[7] & 2))

    def comp_lift(self, comp, level):
        """the wavelet of decomposition level `level` (1 = the first applied) of a component, for the general lifting
        form: dict(steps=[(a, b, e) | A, ...] in synthesis order, K, elem (0 int32, 1 int64, 2 float), horz, vert)"""
        k = capi.Lift()
        check(self._lib.ojphgpu_plan_comp_lift(self.handle, comp, level, C.byref(k)))
        rev = k.elem != 2
        steps = [(k.steps[i].a, k.steps[i].b, k.steps[i].e) if rev else float(k.steps[i].A) for i in range(k.num_steps)]
        return dict(steps=steps, K=float(k.K), elem=int(k.elem), horz=bool(k.horz), vert=bool(k.vert))

    @property
    def frame_elems(self):
        out = (C.c_uint32 * 8)()
        check(self._lib.ojphgpu_plan_comp_info(self.handle, int(self.params.num_comps), out))
        return int(out[4]) | (int(out[5]) << 32)

    @property
    def frame_shape(self):
        """[C,H,W] when every component has the same size, else the flat (frame_elems,)"""
        ci = [self.comp_info(c) for c in range(int(self.params.num_comps))]
        if all((c["w"], c["h"]) == (ci[0]["w"], ci[0]["h"]) for c in ci):
            return (len(ci), ci[0]["h"], ci[0]["w"])
        return (self.frame_elems,)

    def pack_frame(self, planes):
        """list of per-component 2-D arrays -> the frame layout every codec call takes"""
        if len(self.frame_shape) == 3:
            return np.ascontiguousarray(np.stack([np.asarray(q, dtype=np.int32) for q in planes]))
        out = np.empty(self.frame_elems, np.int32)
        for c, q in enumerate(planes):
            i = self.comp_info(c)
            assert tuple(np.shape(q)) == (i["h"], i["w"]), "component %d must be %dx%d" % (c, i["h"], i["w"])
            out[i["frame_off"]:i["frame_off"] + i["w"] * i["h"]] = np.asarray(q, dtype=np.int32).ravel()
        return out

    def unpack_frame(self, frame):
        """frame (numpy, either layout) -> list of per-component 2-D arrays"""
        flat = np.asarray(frame).reshape(-1)
        out = []
        for c in range(int(self.params.num_comps)):
            i = self.comp_info(c)
            out.append(flat[i["frame_off"]:i["frame_off"] + i["w"] * i["h"]].reshape(i["h"], i["w"]))
        return out

    def comp_plane(self, tile, comp):
        off, pitch, rect = C.c_uint64(), C.c_uint32(), (C.c_uint32 * 4)()
        check(self._lib.ojphgpu_plan_comp_plane(self.handle, tile, comp, C.byref(off), C.byref(pitch), rect))
        return int(off.value), int(pitch.value), tuple(int(v) for v in rect)

    def coded_blocks(self):
        out = np.zeros(self.num_blocks, coded_dtype)
        check(self._lib.ojphgpu_plan_coded_blocks(self.handle, out.ctypes.data, self.num_blocks))
        return out

    def padded_blocks(self):
        """ojphgpu_plan_padded_blocks: (block, got, offset, len1, len2, missing_msbs, num_passes) of the blocks a damaged
        codestream's packet headers promise more bytes for than their tile-part holds"""
        n = C.c_size_t()
        check(self._lib.ojphgpu_plan_padded_blocks(self.handle, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), padded_dtype)
        if n.value:
            check(self._lib.ojphgpu_plan_padded_blocks(self.handle, out.ctypes.data, int(n.value), C.byref(n)))
        return out

    @property
    def trunc_levels(self):
        """J, the number of levels of the truncation ladder (include/ojphgpu.h section 5f); OjphError E_INVALID for a plan the
        section refuses"""
        n = C.c_uint32()
        check(self._lib.ojphgpu_plan_trunc_levels(self.handle, C.byref(n)), "plan_trunc_levels")
        return int(n.value)

    def trunc_weights(self):
        """q_b, the weight of every band of the plan in quarter planes (int32 [num_bands])"""
        q = np.zeros(self.num_bands, np.int32)
        check(self._lib.ojphgpu_plan_trunc_weights(self.handle, q.ctypes.data), "plan_trunc_weights")
        return q

    def trunc_table(self, j):
        """t_b(j), the bit-planes every band of the plan drops at level j (uint8 [num_bands])"""
        t = np.zeros(self.num_bands, np.uint8)
        if not 0 <= int(j) < 2 ** 32:
            check(capi.E_INVALID, "plan_trunc_table")
        check(self._lib.ojphgpu_plan_trunc_table(self.handle, int(j), t.ctypes.data), "plan_trunc_table")
        return t

    def t2_write(self, block_data: np.ndarray, coded: np.ndarray) -> bytes:
        """block_data: uint8 array; coded: coded_dtype array (offset/len1/...) in plan order."""
        block_data = np.ascontiguousarray(block_data, dtype=np.uint8)
        coded = np.ascontiguousarray(coded, dtype=coded_dtype)
        need = C.c_size_t()
        cap = int(block_data.size + 64 * self.num_blocks + 4096 * (self.num_tiles + 1) + (1 << 16))
        out = np.empty(cap, np.uint8)
        rc = self._lib.ojphgpu_t2_write(self.handle, block_data.ctypes.data, coded.ctypes.data,
                                        out.ctypes.data, cap, C.byref(need))
        if rc == capi.E_OVERFLOW:
            cap = int(need.value)
            out = np.empty(cap, np.uint8)
            rc = self._lib.ojphgpu_t2_write(self.handle, block_data.ctypes.data, coded.ctypes.data,
                                            out.ctypes.data, cap, C.byref(need))
        check(rc, "t2_write")
        return out[:need.value].tobytes()


    def t2_write_tiles(self, block_data: np.ndarray, coded: np.ndarray, tile_first: int, tile_count: int):
        """Tile-parts of tiles [tile_first, tile_first+tile_count) -> (bytes, Psot per tile)."""
        block_data = np.ascontiguousarray(block_data, dtype=np.uint8)
        coded = np.ascontiguousarray(coded, dtype=coded_dtype)
        lens = np.zeros(max(tile_count, 1) * self.parts_per_tile, np.uint32)
        need = C.c_size_t()
        rc = self._lib.ojphgpu_t2_write_tiles(self.handle, block_data.ctypes.data, coded.ctypes.data, tile_first,
                                              tile_count, None, 0, C.byref(need), lens.ctypes.data)
        if rc not in (capi.OK, capi.E_OVERFLOW):
            check(rc, "t2_write_tiles")
        out = np.empty(max(int(need.value), 1), np.uint8)
        check(self._lib.ojphgpu_t2_write_tiles(self.handle, block_data.ctypes.data, coded.ctypes.data, tile_first,
                                               tile_count, out.ctypes.data, out.size, C.byref(need), lens.ctypes.data),
              "t2_write_tiles")
        return out[:need.value].tobytes(), lens[:tile_count * self.parts_per_tile].copy()

    def t2_main_header(self, tile_part_len=None) -> bytes:
        """SOC .. end of the main header; tile_part_len (Psot of every tile) feeds the TLM marker."""
        lens = None if tile_part_len is None else np.ascontiguousarray(tile_part_len, dtype=np.uint32)
        if lens is not None and lens.size != self.num_tiles * self.parts_per_tile:
            raise ValueError("tile_part_len must have one entry per tile-part")
        need = C.c_size_t()
        ptr = None if lens is None else lens.ctypes.data
        rc = self._lib.ojphgpu_t2_write_main_header(self.handle, ptr, None, 0, C.byref(need))
        if rc not in (capi.OK, capi.E_OVERFLOW):
            check(rc, "t2_write_main_header")
        out = np.empty(int(need.value), np.uint8)
        check(self._lib.ojphgpu_t2_write_main_header(self.handle, ptr, out.ctypes.data, out.size, C.byref(need)),
              "t2_write_main_header")
        return out[:need.value].tobytes()


def rate_grid_qstep(j):
    """base step j of the rate grid (ojphgpu_rate_grid_qstep): 0 = the coarsest (0.5) .. 240 = the finest (2^-16)"""
    q = C.c_float()
    check(capi.lib().ojphgpu_rate_grid_qstep(int(j), C.byref(q)), "rate_grid_qstep")
    return float(q.value)


def rate_search(plan: Plan, hist, max_bytes, size_fn, hint=None):
    """ojphgpu_rate_search, or with hint = a grid index ojphgpu_rate_search_hint (the first trial is `hint`, the second the
    neighbour its result points to; in a sequence: the previous frame's answer): hist uint32 [plan.num_bands, 80] (None: no
    model), size_fn(j) -> bytes of the codestream at grid index j.  -> dict(grid_index, qstep, bytes, bytes_finer, passes,
    first_guess); capi.OjphError with .code == capi.E_BUDGET (and .info = the dict) when not even index 0 fits."""
    info = capi.RateInfo()
    cb = capi.SIZE_FN(lambda user, j: int(size_fn(int(j))))
    h = None if hist is None else np.ascontiguousarray(hist, dtype=np.uint32)
    if h is not None and h.size != plan.num_bands * capi.STATS_BINS:
        raise ValueError("hist must hold 80 bins for every band of the plan")
    hp = None if h is None else h.ctypes.data
    if hint is None:
        rc = capi.lib().ojphgpu_rate_search(plan.handle, hp, int(max_bytes), cb, None, C.byref(info))
    elif not -2 ** 31 <= int(hint) < 2 ** 31:              # (no grid index, and c_int32 would wrap it into one)
        rc = capi.E_INVALID
    else:
        rc = capi.lib().ojphgpu_rate_search_hint(plan.handle, hp, int(max_bytes), int(hint), cb, None, C.byref(info))
    out = {k: getattr(info, k) for k, _ in capi.RateInfo._fields_}
    if rc != capi.OK:
        err = capi.OjphError(rc, "rate_search")
        err.info = out
        raise err
    return out


def trunc_synth_norm(depth, high):
    """L2 norm of the 1-D 5/3 synthesis basis vector of the low / high branch at decomposition depth `depth`: a unit impulse
    through the linear inverse lifting, in float64, in the middle of a line of 64 coefficients at that depth (beyond depth
    12: times sqrt(2) per further level, as the C code)"""
    if depth == 0:
        return 1.0
    dd = min(int(depth), 12)
    s, h = np.zeros(64), np.zeros(64)
    (h if high else s)[32] = 1.0
    for _ in range(dd):
        n = len(s)
        x = np.zeros(2 * n)
        x[0::2] = s - (np.concatenate([h[:1], h[:-1]]) + h) / 4.0
        x[1::2] = h + (x[0::2] + np.concatenate([x[2::2], x[-2:-1]])) / 2.0
        s, h = x, np.zeros(2 * n)
    return float(np.sqrt((s * s).sum()) * 2.0 ** (0.5 * (depth - dd)))


def trunc_table_np(bands, num_decomps, rct, j=None):
    """The ladder of include/ojphgpu.h section 5f restated in numpy from the band list alone: bands = plan.bands (fields comp,
    res, band, K_max), num_decomps = the decompositions of every component, rct = the reversible colour transform is on.
    -> (q int32 [bands], J, tie) with tie = the smallest distance of a 4 w_b from a rounding tie; with j also t_b(j) uint8
    as a fourth value."""
    comp, res, ori = (np.asarray(bands[k]).astype(np.int64) for k in ("comp", "res", "band"))
    top = np.maximum(np.asarray(bands["K_max"]).astype(np.int64), 1) - 1
    depth = np.where(res == 0, num_decomps, num_decomps - res + 1)
    norms = {(d, hi): trunc_synth_norm(d, hi) for d in set(depth.tolist()) for hi in (False, True)}
    gh = np.array([norms[(d, o in (1, 3))] for d, o in zip(depth.tolist(), ori.tolist())])
    gv = np.array([norms[(d, o in (2, 3))] for d, o in zip(depth.tolist(), ori.tolist())])
    gc = np.ones(len(comp))
    if rct:
        gc = np.where(comp == 0, np.sqrt(3.0), np.where(comp < 3, np.sqrt(11.0 / 16.0), 1.0))
    w = np.log2(gh * gv * gc)
    x = 4.0 * (w - w.min())
    q = np.floor(x + 0.5).astype(np.int64)
    tie = float(np.abs(x - np.floor(x) - 0.5).min())
    J = int((4 * top + q).max() - 3 + 1)
    out = (q.astype(np.int32), max(J, 1), tie)
    if j is not None:
        out += (np.clip((int(j) + 3 - q) // 4, 0, top).astype(np.uint8),)
    return out


def trunc_search(plan: Plan, hist, max_bytes, size_fn):
    """ojphgpu_trunc_search: hist uint32 [plan.num_bands, 80] of ojphgpu_band_stats_int (None: no model), size_fn(j) -> bytes
    of the codestream at level j.  -> dict(level, passes, first_guess, max_dropped, lossless, bytes, bytes_finer);
    capi.OjphError with .code == capi.E_BUDGET (and .info = the dict) when not even the last level fits."""
    info = capi.TruncInfo()
    cb = capi.SIZE_FN(lambda user, j: int(size_fn(int(j))))
    h = None if hist is None else np.ascontiguousarray(hist, dtype=np.uint32)
    if h is not None and h.size != plan.num_bands * capi.STATS_BINS:
        raise ValueError("hist must hold 80 bins for every band of the plan")
    rc = capi.lib().ojphgpu_trunc_search(plan.handle, None if h is None else h.ctypes.data, int(max_bytes), cb, None, C.byref(info))
    out = {k: int(getattr(info, k)) for k, _ in capi.TruncInfo._fields_ if k != "reserved"}
    if rc != capi.OK:
        err = capi.OjphError(rc, "trunc_search")
        err.info = out
        raise err
    return out


def near_lossless_search(plan: Plan, max_sse, max_pae, err_fn):
    """ojphgpu_near_lossless_search: max_sse / max_pae None = no bound; err_fn(level) -> (sse, pae) of the decode of the
    codestream at that level.  -> dict(level, passes, lossless, max_dropped, sse, pae, level_coarser, sse_coarser, pae_coarser,
    bytes = 0)"""
    info = capi.NearLosslessInfo()

    def trial(user, level, sse, pae):
        a, b = err_fn(int(level))
        sse[0], pae[0] = int(a), int(b)
        return 0

    t = 2 ** 64 - 1 if max_sse is None else int(max_sse)
    e = 2 ** 32 - 1 if max_pae is None else int(max_pae)
    check(capi.lib().ojphgpu_near_lossless_search(plan.handle, t, e, capi.ERR_FN(trial), None, C.byref(info)), "near_lossless_search")
    return {k: int(getattr(info, k)) for k, _ in capi.NearLosslessInfo._fields_ if k != "reserved"}


def quality_search(max_sse, sse_fn, hint=None):
    """ojphgpu_quality_search, or with hint = a grid index (-1: none) ojphgpu_quality_search_hint (the first trial is `hint`,
    then its neighbours on the side the result points to; in a sequence: the previous frame's answer): sse_fn(j) -> SSE of
    the frame at grid index j (a negative value: an error code).  -> dict(grid_index, qstep, sse, sse_coarser, pae, passes,
    bytes), with a hint also first_guess; capi.OjphError with .code == capi.E_QUALITY (and .info = the dict) when not even
    index 240 meets max_sse."""
    info = capi.QualityInfo()
    first = C.c_uint32()

    def fn(user, j, out):
        v = int(sse_fn(int(j)))
        if v < 0:
            return v
        out[0] = v
        return 0
    cb = capi.SSE_FN(fn)
    if not 0 <= int(max_sse) < 2 ** 64:
        raise ValueError("max_sse must fit 64 bits")
    if hint is None:
        rc = capi.lib().ojphgpu_quality_search(int(max_sse), cb, None, C.byref(info))
    elif not -2 ** 31 <= int(hint) < 2 ** 31:              # (no grid index, and c_int32 would wrap it into one)
        rc = capi.E_INVALID
    else:
        rc = capi.lib().ojphgpu_quality_search_hint(int(max_sse), int(hint), cb, None, C.byref(info), C.byref(first))
    out = {k: getattr(info, k) for k, _ in capi.QualityInfo._fields_}
    if hint is not None:
        out["first_guess"] = int(first.value)
    if rc != capi.OK:
        err = capi.OjphError(rc, "quality_search")
        err.info = out
        raise err
    return out


def capped_search(plan: Plan, max_sse, cap_bytes, sse_fn, size_fn, hist_fn=None, hint_q=-1, hint_b=-1):
    """ojphgpu_capped_search: a quality target under a byte cap over callbacks of the caller's -- sse_fn(j) -> SSE at grid
    index j, size_fn(j) -> bytes of its codestream (negative values: error codes), hist_fn() -> uint32 [plan.num_bands, 80]
    or None, called at most once and only when the cap binds.  -> dict of capi.CappedInfo's fields; capi.OjphError with
    .code (capi.E_BUDGET when not even index 0 fits) and .info = the dict otherwise."""
    info = capi.CappedInfo()
    keep = []

    def sse(user, j, out):
        v = int(sse_fn(int(j)))
        if v < 0:
            return v
        out[0] = v
        return 0

    def hist(user):
        h = None if hist_fn is None else hist_fn()
        if h is None:
            return None
        h = np.ascontiguousarray(h, dtype=np.uint32)
        if h.size != plan.num_bands * capi.STATS_BINS:
            raise ValueError("hist must hold 80 bins for every band of the plan")
        keep.append(h)
        return h.ctypes.data
    if not 0 <= int(max_sse) < 2 ** 64 or not 0 <= int(cap_bytes) < 2 ** 64:
        raise ValueError("max_sse and cap_bytes must fit 64 bits")
    if not all(-2 ** 31 <= int(h) < 2 ** 31 for h in (hint_q, hint_b)):
        rc = capi.E_INVALID
    else:
        rc = capi.lib().ojphgpu_capped_search(plan.handle, int(max_sse), int(cap_bytes), int(hint_q), int(hint_b), capi.SSE_FN(sse),
                                              capi.SIZE_FN(lambda user, j: int(size_fn(int(j)))), capi.HIST_FN(hist), None, C.byref(info))
    out = {k: getattr(info, k) for k, _ in capi.CappedInfo._fields_ if k != "reserved"}
    if rc != capi.OK:
        err = capi.OjphError(rc, "capped_search")
        err.info = out
        raise err
    return out


def psnr_to_sse(plan: Plan, db):
    """the max_sse of a PSNR over the whole frame: int(n peak^2 / 10^(dB / 10)) with n = the samples of all components and
    peak = 2^bit_depth - 1.  ValueError when the components differ in depth (a frame then has no one peak)."""
    nc = int(plan.params.num_comps)
    depths = {plan.comp_format(c)[0] for c in range(nc)}
    if len(depths) != 1:
        raise ValueError("psnr_to_sse: the components differ in bit depth (%s)" % sorted(depths))
    peak = (1 << depths.pop()) - 1
    n = sum(plan.comp_info(c)["w"] * plan.comp_info(c)["h"] for c in range(nc))
    return int(n * peak * peak / 10 ** (db / 10))


def rate_predict(plan: Plan, hist):
    """the model of ojphgpu_rate_search alone: predicted bytes at every grid index (float64 [241])"""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    out = np.zeros(capi.RATE_GRID, np.float64)
    check(capi.lib().ojphgpu_rate_predict(plan.handle, h.ctypes.data, out.ctypes.data_as(C.POINTER(C.c_double))), "rate_predict")
    return out


def transcode_params(src_plan: Plan, qstep=None, block=None, prog_order=None, precinct=None, precincts=None, tlm=None, tileparts=None):
    """The parameters of a transcode's output: those of the parsed `src_plan` with only what may change changed -- qstep (an
    irreversible output needs one, or a byte budget: a codestream does not carry its base step), block=(w, h),
    prog_order, precinct=(w, h) or precincts=[(w, h), ...] from the lowest resolution up, tlm, tileparts ("", "R", "C",
    "RC").  None keeps the source's."""
    p = Params.from_buffer_copy(src_plan.params)
    if qstep is not None:
        p.qstep = float(qstep)
    if block is not None:
        p.block_w, p.block_h = block
    if prog_order is not None:
        p.prog_order = PROG_ORDERS[prog_order] if isinstance(prog_order, str) else int(prog_order)
    if precinct is not None or precincts is not None:
        p.precinct_w, p.precinct_h = precinct if precinct is not None else (0, 0)
        for i in range(36):
            p.precinct_exps[i] = 0
        if precincts:
            for i in range(int(p.num_decomps) + 1):
                pw, ph = precincts[min(i, len(precincts) - 1)]
                p.precinct_exps[i] = (int(pw).bit_length() - 1) | ((int(ph).bit_length() - 1) << 4)
    if tlm is not None:
        p.tlm = int(bool(tlm))
    if tileparts is not None:
        p.reserved[1] = (1 if "R" in tileparts else 0) | (2 if "C" in tileparts else 0)
    return p


def transcode_plan(src_plan: Plan, params) -> Plan:
    """ojphgpu_plan_create_transcode: the plan of `params` (transcode_params) checked against the parsed source -- the same
    frame, components, wavelet and decompositions, every band at the same place in the arena.  OjphError E_INVALID
    otherwise."""
    h = C.c_void_p()
    check(capi.lib().ojphgpu_plan_create_transcode(src_plan.handle, C.byref(params), C.byref(h)), "plan_create_transcode")
    return Plan(handle=h)


# make_params keyword -> the fields of ojphgpu_params it fills ((name, index): one element of an array field)
_PARAM_FIELDS = {
    "bit_depth": ["bit_depth"], "bit_depths": ["comp_depth"], "is_signed": ["is_signed"], "signs": ["comp_sign"],
    "reversible": ["reversible"], "num_decomps": ["num_decomps"], "block": ["block_w", "block_h"],
    "color_transform": ["color_transform"], "tile": ["tile_w", "tile_h"], "prog_order": ["prog_order"], "qstep": ["qstep"],
    "precinct": ["precinct_w", "precinct_h"], "precincts": ["precinct_exps"], "tlm": ["tlm"], "tileparts": [("reserved", 1)],
    "qfactor": [("reserved", 2)], "image_offset": ["image_x0", "image_y0"], "tile_offset": ["tile_x0", "tile_y0"],
    "downsampling": ["comp_dx", "comp_dy"], "coc": ["coc"], "nlt": ["nlt_default", "nlt_comp", "nlt_rank"],
    "qfactors": ["qcc_qfactor", "qcc_ctype", "qcc_rank"], "atk": ["atk"], "dfs": ["dfs"], "wavelet": ["wavelet"],
}


def recode_params(src_plan: Plan, bit_depth=None, bit_depths=None, **kw):
    """The parameters of a recode's output (codec.Recoder; include/ojphgpu.h section 5e): those of the parsed `src_plan`
    -- under a view (restrict_resolution, restrict_region) the view's size on a grid of its own: image and tile offsets
    zero, one tile, the source's decompositions minus the skipped resolutions -- with every make_params keyword given
    overriding what it sets (reversible, qstep, num_decomps, tile, block, prog_order, ...).  bit_depth=N: every component
    N bits deep; bit_depths=[...]: per component.  What only a parser sets (vertically causal blocks, BDnlt) is dropped:
    the result is a writer's."""
    p = Params.from_buffer_copy(src_plan.params)
    p.reserved[0] = 0
    p.nlt_bd_default = 0
    for i in range(len(p.nlt_bd)):
        p.nlt_bd[i] = 0
    for i in range(len(p.nlt_reserved)):
        p.nlt_reserved[i] = 0
    skip = int(src_plan.skip[1])
    if skip or src_plan.region is not None:
        a0x, a0y = int(p.image_x0), int(p.image_y0)
        a1x, a1y = a0x + int(p.width), a0y + int(p.height)
        if src_plan.region is not None:
            x0, y0, w, h = src_plan.region
            a0x, a0y, a1x, a1y = a0x + x0, a0y + y0, a0x + x0 + w, a0y + y0 + h
        up = lambda v: -((-v) >> skip)                      # ceil(v / 2^skip)
        p.width, p.height = up(a1x) - up(a0x), up(a1y) - up(a0y)
        p.image_x0 = p.image_y0 = p.tile_x0 = p.tile_y0 = 0
        p.tile_w = p.tile_h = 0
        p.num_decomps = int(p.num_decomps) - skip
        for c in range(len(p.coc)):
            if p.coc[c].rank and not p.coc[c].reserved[0] & 0x80:
                p.coc[c].num_decomps = int(p.coc[c].num_decomps) - skip
    if bit_depth is not None:
        kw["bit_depth"] = int(bit_depth)
        kw.setdefault("bit_depths", [0] * 16)
    if bit_depths is not None:
        kw["bit_depths"] = [int(b) for b in bit_depths]
    unknown = set(kw) - set(_PARAM_FIELDS)
    if unknown:
        raise TypeError("recode_params: not a make_params keyword: %s" % ", ".join(sorted(unknown)))
    kw.setdefault("num_decomps", int(p.num_decomps))        # (make_params sizes the precinct list by it)
    o = make_params(int(p.width), int(p.height), int(p.num_comps), **kw)
    for k in kw:
        for f in _PARAM_FIELDS[k]:
            if isinstance(f, tuple):
                getattr(p, f[0])[f[1]] = getattr(o, f[0])[f[1]]
            else:
                setattr(p, f, getattr(o, f))
    return p


def parse_codestream(data: bytes, resilient=False, skip=None) -> Plan:
    """skip = (skipped_res_for_data, skipped_res_for_recon): restrict_input_resolution BEFORE the tile-parts are read, as the
    reference orders it (ojphgpu_t2_parse_restricted) -- on undamaged codestreams the same as Plan.restrict_resolution afterwards"""
    buf = np.frombuffer(data, dtype=np.uint8)
    h = C.c_void_p()
    if skip is None:
        check(capi.lib().ojphgpu_t2_parse(buf.ctypes.data, len(data), int(resilient), C.byref(h)), "t2_parse")
        return Plan(handle=h)
    check(capi.lib().ojphgpu_t2_parse_restricted(buf.ctypes.data, len(data), int(resilient), int(skip[0]), int(skip[1]), C.byref(h)), "t2_parse")
    pl = Plan(handle=h)
    pl.skip = (int(skip[0]), int(skip[1]))
    return pl
