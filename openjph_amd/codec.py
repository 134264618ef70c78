"""Python host-side wrapper of the GPU codec objects (C ABI sections 4 and 5).

PyTorch is used only as plumbing: device memory (torch tensors on ``cuda:N``) and streams.  All
arithmetic happens in the HIP kernels behind libojphgpu.so; there is no CPU fallback -- without the
library or without a GPU these calls raise.
"""
import ctypes as C
import numpy as np

from . import capi
from .capi import check, Params, DwtDesc, DwtRegion, CbDesc, CbResult, ConvertDesc
from .plan import Plan, make_params, parse_codestream

dwt_desc_dtype = np.dtype(DwtDesc)
dwt_region_dtype = np.dtype(DwtRegion)
cb_desc_dtype = np.dtype(CbDesc)
cb_result_dtype = np.dtype(CbResult)
convert_desc_dtype = np.dtype(ConvertDesc)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("openjph_amd: no GPU visible (torch.cuda.is_available() is False); "
                           "the HTJ2K hot path has no CPU fallback")
    return torch


def _stream_ptr(torch, device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def to_device(arr: np.ndarray, device=0):
    """numpy (any dtype / structured) -> uint8 torch tensor on the device holding the same bytes."""
    torch = _torch()
    raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
    if raw.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda:%d" % device)
    return torch.from_numpy(raw.copy()).to("cuda:%d" % device)


class Encoder:
    """Whole-frame encoder for one frame shape / parameter set (ojphgpu_encoder)."""

    def __init__(self, params: Params = None, device=0, plan: Plan = None, tiles=None, frames=1, max_bytes=0, max_sse=None, min_psnr=None,
                 budgets=None, cap_bytes=0, truncate_to=0, truncate_level=None, **kw):
        """tiles=(first, count) restricts the encoder to a run of tiles (multi-GPU sharding);
        frames=B makes it code a batch of B independent frames per run ([B,C,H,W] input);
        max_bytes=N codes every frame to a byte budget (set_budget);
        budgets=[N0, N1, ...] codes frame f of every batch to N_f bytes (set_budgets);
        max_sse=N / min_psnr=dB codes every frame to a quality target (set_quality);
        cap_bytes=N with one of those two: to the target, but never above N bytes (set_quality(..., cap_bytes=N));
        truncate_to=N codes every reversible frame under a byte cap (set_truncation), truncate_level=j at a fixed level of
        the truncation ladder (set_trunc_level)."""
        torch = _torch()
        if cap_bytes and max_sse is None and min_psnr is None:
            raise ValueError("cap_bytes needs a quality target (max_sse or min_psnr); a byte budget alone is max_bytes")
        self.device = device
        self.plan = plan if plan is not None else Plan(params if params is not None else make_params(**kw))
        self.tiles = (0, self.plan.num_tiles) if tiles is None else (int(tiles[0]), int(tiles[1]))
        self.frames = int(frames)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        with torch.cuda.device(device):
            if self.frames > 1:
                assert tiles is None, "a batch encoder codes whole frames"
                check(self._lib.ojphgpu_encoder_create_batch(self.plan.handle, device, _stream_ptr(torch, device),
                                                             self.frames, C.byref(self._h)), "encoder_create_batch")
            else:
                check(self._lib.ojphgpu_encoder_create_tiles(self.plan.handle, device, _stream_ptr(torch, device),
                                                             self.tiles[0], self.tiles[1], C.byref(self._h)),
                      "encoder_create")
        fs = self.plan.frame_shape          # [C,H,W], or flat (frame_elems,) when components differ in size
        self.shape = fs if self.frames == 1 else (self.frames,) + fs
        self.max_bytes = 0
        self.budgets = None
        self.max_sse = None
        self.cap_bytes = 0
        self._frame = None
        self.truncating = False
        if max_bytes:
            self.set_budget(max_bytes)
        if truncate_to:
            self.set_truncation(truncate_to)
        if truncate_level is not None:
            self.set_trunc_level(truncate_level)
        if budgets is not None:
            self.set_budgets(budgets)
        if max_sse is not None or min_psnr is not None:
            self.set_quality(max_sse=max_sse, min_psnr=min_psnr, cap_bytes=cap_bytes)

    def set_budget(self, max_bytes):
        """Every following frame is coded at the finest step of the rate grid (plan.rate_grid_qstep) whose codestream is at
        most max_bytes long; the plan's own qstep is then not used.  0 switches the budget off.  Irreversible whole-frame
        single-frame encoders without quality factors only; a budget nothing fits raises OjphError with code E_BUDGET from
        finish() / encode()."""
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_encoder_set_budget(self._h, int(max_bytes)), "encoder_set_budget")
        self.max_bytes = int(max_bytes)
        self.budgets = None

    def set_truncation(self, max_bytes):
        """Every following frame of a reversible encoder is coded under a byte cap (include/ojphgpu.h section 5f): lossless,
        byte for byte the plain encode, where that fits max_bytes; else at the first level of the truncation ladder
        (plan.trunc_table) whose codestream fits -- its sub-bands drop low bit-planes, any 5/3 decoder reads it.  0 switches
        the mode off.  A cap not even the last level fits raises OjphError with code E_BUDGET from finish() / encode()."""
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_encoder_set_truncation(self._h, int(max_bytes)), "encoder_set_truncation")
        self.truncating = int(max_bytes) > 0

    def set_trunc_level(self, j):
        """Every following frame is coded at level j of the truncation ladder (0: lossless): no search, no statistics.
        None or a negative j switches the mode off."""
        j = -1 if j is None else int(j)
        if not -2 ** 31 <= j < 2 ** 31:
            check(capi.E_INVALID, "encoder_set_trunc_level")
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_encoder_set_trunc_level(self._h, j), "encoder_set_trunc_level")
        self.truncating = j >= 0

    def trunc_info(self):
        """what the last finish() of a truncating encoder found: dict(level, passes = block-coder runs the search measured,
        first_guess, max_dropped = the most planes a band drops, lossless, bytes, bytes_finer = the length one level finer, 0
        at level 0); after E_BUDGET: passes and first_guess"""
        info = capi.TruncInfo()
        check(self._lib.ojphgpu_encoder_trunc_info(self._h, C.byref(info)), "encoder_trunc_info")
        return {k: int(getattr(info, k)) for k, _ in capi.TruncInfo._fields_ if k != "reserved"}

    def trunc_timing(self):
        """of the last finish() of a truncating encoder, ms: dict(search_ms = host clock of the coding inside it, stats_ms = the
        integer statistics kernel of the run before it (device events; 0 at a fixed level))"""
        t = (C.c_float * 2)()
        check(self._lib.ojphgpu_encoder_trunc_timing(self._h, t), "encoder_trunc_timing")
        return dict(search_ms=t[0], stats_ms=t[1])

    def set_budgets(self, budgets):
        """A batch encoder codes frame f of every following batch to budgets[f] bytes (len(budgets) == frames): each
        codestream is what a single-frame encoder with set_budget(budgets[f]) writes for that frame.  All zeros switches
        the budgets off; a zero among others is refused.  The frames are searched together, in rounds over shared launches
        (rate_rounds).  A frame nothing fits raises OjphError with code E_BUDGET from its own finish(f); the other frames
        are written.  set_budget(N) stays refused on a batch encoder: this is the call, also for equal budgets."""
        seq = [int(b) for b in budgets]
        arr = (C.c_uint64 * max(len(seq), 1))(*seq)
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_encoder_set_budgets(self._h, arr, len(seq)), "encoder_set_budgets")
        if self.frames == 1:
            self.max_bytes, self.budgets = seq[0], None
        else:
            self.max_bytes = seq[0] if any(seq) else 0
            self.budgets = seq if any(seq) else None

    def set_quality(self, max_sse=None, min_psnr=None, cap_bytes=0):
        """Every following frame is coded at the coarsest step of the rate grid found to meet the target: the squared error
        between the frame and the decode of its codestream, summed over all components, is at most max_sse (an integer; 0 is
        a target) -- or min_psnr in dB, turned into one by plan.psnr_to_sse.  Both None switches the target off.  Where
        set_budget applies, and components of at most 16 bits; not together with a budget.  A target that not even the
        finest step meets raises OjphError with code E_QUALITY from finish() / encode().  The frame handed to run_device
        is kept until finish() has returned: the search compares against it.

        cap_bytes=N > 0: under a byte cap -- the step of the target where its codestream is at most N bytes long (outcome
        MET), else the finest step that fits (outcome BY_BUDGET): the cap wins, E_QUALITY is never raised, and a cap below
        the coarsest step's codestream raises E_BUDGET.  capped_info() tells which; quality_info() and rate_info() are
        refused while a cap is set."""
        from .plan import psnr_to_sse
        if max_sse is not None and min_psnr is not None:
            raise ValueError("set_quality: max_sse or min_psnr, not both")
        cap = int(cap_bytes)
        if cap and max_sse is None and min_psnr is None:
            raise ValueError("set_quality: cap_bytes needs a quality target (max_sse or min_psnr)")
        if not 0 <= cap < 2 ** 64:
            raise ValueError("set_quality: cap_bytes must fit 64 bits")
        with _torch().cuda.device(self.device):
            if max_sse is None and min_psnr is None:
                check(self._lib.ojphgpu_encoder_clear_quality(self._h), "encoder_clear_quality")
                self.max_sse, self.cap_bytes = None, 0
                return
            t = int(max_sse) if max_sse is not None else psnr_to_sse(self.plan, float(min_psnr))
            if not 0 <= t < 2 ** 64:
                raise ValueError("set_quality: max_sse must fit 64 bits")
            if cap:
                check(self._lib.ojphgpu_encoder_set_quality_capped(self._h, t, cap), "encoder_set_quality_capped")
            else:
                check(self._lib.ojphgpu_encoder_set_quality(self._h, t), "encoder_set_quality")
        self.max_sse, self.cap_bytes = t, cap

    def capped_info(self):
        """what the last finish() under a byte cap found: dict(grid_index, qstep, outcome = capi.CAPPED_MET /
        CAPPED_BY_BUDGET, quality_index = the target's own step (241: no step of the grid meets it), quality_bytes = its
        codestream's length (0: never coded), bytes, bytes_finer, sse, sse_coarser, pae, quality_passes, rate_passes,
        first_guess_q, first_guess_b, comps = [(sse, pae) per component]); after E_BUDGET the passes and comps == []"""
        info = capi.CappedInfo()
        check(self._lib.ojphgpu_encoder_capped_info(self._h, C.byref(info)), "encoder_capped_info")
        out = {k: getattr(info, k) for k, _ in capi.CappedInfo._fields_ if k != "reserved"}
        out["comps"] = []
        for c in range(int(self.plan.params.num_comps)):
            sse, pae = C.c_uint64(), C.c_uint32()
            if self._lib.ojphgpu_encoder_quality_comp(self._h, c, C.byref(sse), C.byref(pae)) != capi.OK:
                break
            out["comps"].append((int(sse.value), int(pae.value)))
        return out

    def quality_info(self):
        """what the last finish() with a quality target found: dict(grid_index, qstep, sse, sse_coarser = the error one step
        coarser (0 at index 0), pae = the largest absolute difference, passes = trials made, bytes, comps = [(sse, pae) per
        component]); after E_QUALITY only passes is meaningful and comps is empty"""
        info = capi.QualityInfo()
        check(self._lib.ojphgpu_encoder_quality_info(self._h, C.byref(info)), "encoder_quality_info")
        out = {k: getattr(info, k) for k, _ in capi.QualityInfo._fields_}
        out["comps"] = []
        for c in range(int(self.plan.params.num_comps)):
            sse, pae = C.c_uint64(), C.c_uint32()
            if self._lib.ojphgpu_encoder_quality_comp(self._h, c, C.byref(sse), C.byref(pae)) != capi.OK:
                break
            out["comps"].append((int(sse.value), int(pae.value)))
        return out

    def quality_timing(self):
        """host clock of the last finish() with a quality target, ms: dict(search_ms = all trials, wait_ms = of that, waiting
        for the device, final_ms = coding the chosen step, its download and Tier-2)"""
        t = (C.c_float * 3)()
        check(self._lib.ojphgpu_encoder_quality_timing(self._h, t), "encoder_quality_timing")
        return dict(search_ms=t[0], wait_ms=t[1], final_ms=t[2])

    def rate_info(self, frame=None):
        """what the last budgeted finish() found: dict(grid_index, qstep, bytes, bytes_finer = the length one step finer
        (0 at the end of the grid), passes = block-coder runs made, first_guess = the model's first index).  A batch
        encoder: the list of these per frame (frame=f: that frame's alone), None for a frame nothing fitted; passes are
        the frame's own trials, as a single encoder would have made them."""
        info = capi.RateInfo()
        if self.frames == 1:
            check(self._lib.ojphgpu_encoder_rate_info(self._h, C.byref(info)), "encoder_rate_info")
            return {k: getattr(info, k) for k, _ in capi.RateInfo._fields_}
        out = []
        for f in (range(self.frames) if frame is None else [int(frame)]):
            rc = self._lib.ojphgpu_encoder_rate_info_frame(self._h, f, C.byref(info))
            if rc != capi.E_BUDGET:
                check(rc, "encoder_rate_info_frame")
            out.append(None if rc == capi.E_BUDGET else {k: getattr(info, k) for k, _ in capi.RateInfo._fields_})
        return out if frame is None else out[0]

    def rate_rounds(self):
        """block-coder runs the last budgeted finish() made: the rounds of a batch's search (every round codes all frames),
        the passes of a single frame's"""
        n = C.c_uint32()
        check(self._lib.ojphgpu_encoder_rate_rounds(self._h, C.byref(n)), "encoder_rate_rounds")
        return int(n.value)

    def rate_timing(self):
        """host clock of the last budgeted finish(), ms: dict(search_ms = all passes, wait_ms = of that, waiting for the device,
        final_ms = download + Tier-2 of the chosen step, stats_ms = the band statistics kernel (device events))"""
        t = (C.c_float * 4)()
        check(self._lib.ojphgpu_encoder_rate_timing(self._h, t), "encoder_rate_timing")
        return dict(search_ms=t[0], wait_ms=t[1], final_ms=t[2], stats_ms=t[3])

    def __del__(self):
        try:
            if self._h:
                self._lib.ojphgpu_encoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def run_device(self, d_image):
        """d_image: int32 torch tensor [C,H,W] (flat plan.frame_shape for sub-sampled components)
        resident on the device. Asynchronous.  In the order of the encoder's stream the frame has been consumed on return;
        the products are reached through this object's calls, which wait for them (a run with set_timing(False) may be
        released: include/ojphgpu.h, ojphgpu_encoder_run_device)."""
        torch = _torch()
        assert d_image.is_cuda and tuple(d_image.shape) == self.shape and d_image.is_contiguous()
        self._frame = d_image if self.max_sse is not None else None      # a quality target: finish() reads the frame again
        if d_image.dtype in (torch.int16, torch.uint16):     # 16-bit containers: int16 for signed components, else uint16
            check(self._lib.ojphgpu_encoder_run_device16(self._h, C.c_void_p(d_image.data_ptr())), "encoder_run_device16")
            return
        if d_image.dtype in (torch.int8, torch.uint8):       # 8-bit containers
            check(self._lib.ojphgpu_encoder_run_device8(self._h, C.c_void_p(d_image.data_ptr())), "encoder_run_device8")
            return
        assert d_image.dtype == torch.int32
        check(self._lib.ojphgpu_encoder_run_device(self._h, C.c_void_p(d_image.data_ptr())), "encoder_run_device")

    def set_timing(self, per_launch: bool):
        check(self._lib.ojphgpu_encoder_set_timing(self._h, int(per_launch)), "encoder_set_timing")

    def pending(self):
        """a released run of this encoder has not been waited for yet (by coded_bytes, finish*, timing, the next run)"""
        n = C.c_int()
        check(self._lib.ojphgpu_encoder_is_pending(self._h, C.byref(n)), "encoder_is_pending")
        return bool(n.value)

    def coded_bytes(self):
        n = C.c_uint64()
        check(self._lib.ojphgpu_encoder_coded_bytes(self._h, C.byref(n)), "encoder_coded_bytes")
        return int(n.value)

    def finish(self, frame=0) -> bytes:
        """codestream of frame `frame` of the last run"""
        if self.max_bytes:                 # (a budget far above what the frame can need: the second round below)
            budget = self.budgets[frame] if self.budgets and 0 <= frame < self.frames else self.max_bytes
            cap = min(budget, self.plan.frame_elems * 4 + 64 * self.plan.num_blocks + (1 << 20))
        elif self.max_sse is not None or self.truncating:     # (the blocks are coded inside finish: nothing to size the buffer by yet)
            cap = self.plan.frame_elems * 3 + 64 * self.plan.num_blocks + (1 << 20)
        else:
            cap = self.coded_bytes() // self.frames * 2 + 64 * self.plan.num_blocks + (1 << 20)
        out = np.empty(cap, np.uint8)
        n = C.c_size_t()
        rc = self._lib.ojphgpu_encoder_finish_frame(self._h, frame, out.ctypes.data, cap, C.byref(n))
        if rc == capi.E_OVERFLOW and n.value > cap:
            cap = int(n.value)
            out = np.empty(cap, np.uint8)
            rc = self._lib.ojphgpu_encoder_finish_frame(self._h, frame, out.ctypes.data, cap, C.byref(n))
        self._frame = None
        check(rc, "encoder_finish")
        return out[:n.value].tobytes()

    def finish_tiles(self):
        """-> (tile-part bytes of this encoder's tile range, Psot per tile)"""
        cap = self.plan.frame_elems * 3 + (1 << 20)
        lens = np.zeros(max(self.tiles[1], 1) * self.plan.parts_per_tile, np.uint32)
        n = C.c_size_t()
        out = np.empty(cap, np.uint8)
        rc = self._lib.ojphgpu_encoder_finish_tiles(self._h, out.ctypes.data, cap, C.byref(n), lens.ctypes.data)
        if rc == capi.E_OVERFLOW and n.value > cap:
            cap = int(n.value)
            out = np.empty(cap, np.uint8)
            rc = self._lib.ojphgpu_encoder_finish_tiles(self._h, out.ctypes.data, cap, C.byref(n), lens.ctypes.data)
        check(rc, "encoder_finish_tiles")
        return out[:n.value].tobytes(), lens[:self.tiles[1] * self.plan.parts_per_tile].copy()

    def finish_tiles_device(self):
        """-> (tile-part bytes of this encoder's tile range as a uint8 torch tensor ON THE DEVICE, Psot per tile-part):
        the bytes are assembled in HBM and never visit the host (input of shard.gather_bytes over RCCL)"""
        torch = _torch()
        cap = self.coded_bytes() + 64 * self.plan.num_blocks + 4096 * max(self.tiles[1], 1) + (1 << 16)
        lens = np.zeros(max(self.tiles[1], 1) * self.plan.parts_per_tile, np.uint32)
        n = C.c_size_t()
        out = torch.empty(cap, dtype=torch.uint8, device="cuda:%d" % self.device)
        rc = self._lib.ojphgpu_encoder_finish_tiles_device(self._h, C.c_void_p(out.data_ptr()), cap, C.byref(n), lens.ctypes.data)
        if rc == capi.E_OVERFLOW and n.value > cap:
            cap = int(n.value)
            out = torch.empty(cap, dtype=torch.uint8, device="cuda:%d" % self.device)
            rc = self._lib.ojphgpu_encoder_finish_tiles_device(self._h, C.c_void_p(out.data_ptr()), cap, C.byref(n), lens.ctypes.data)
        check(rc, "encoder_finish_tiles_device")
        return out[:n.value], lens[:self.tiles[1] * self.plan.parts_per_tile].copy()

    def encode(self, image):
        """image: numpy int32 [C,H,W] (host), a list of per-component 2-D arrays (sub-sampled
        components), or a torch int32 tensor on the device -> codestream bytes; for a batch encoder
        [B,C,H,W] -> list of B codestreams."""
        torch = _torch()
        if isinstance(image, (list, tuple)):
            image = self.plan.pack_frame(image)
        if isinstance(image, np.ndarray):
            if image.dtype in (np.int16, np.uint16):         # stays 16 bits wide on its way to and in HBM
                image = torch.from_numpy(np.ascontiguousarray(image).view(np.int16)).to("cuda:%d" % self.device)
            elif image.dtype in (np.int8, np.uint8):         # ... or 8
                image = torch.from_numpy(np.ascontiguousarray(image).view(np.int8)).to("cuda:%d" % self.device)
            else:
                image = torch.from_numpy(np.ascontiguousarray(image, dtype=np.int32)).to("cuda:%d" % self.device)
        self.run_device(image)
        if self.frames > 1:
            return [self.finish(f) for f in range(self.frames)]
        return self.finish()

    def timing(self):
        t = (C.c_float * 4)()
        check(self._lib.ojphgpu_encoder_timing(self._h, t), "encoder_timing")
        lv = (C.c_float * 40)(); n = C.c_uint32()
        check(self._lib.ojphgpu_encoder_level_timing(self._h, lv, 40, C.byref(n)), "encoder_level_timing")
        ht = (C.c_float * 4)(); nh = C.c_uint32(); ntop = C.c_uint32()
        check(self._lib.ojphgpu_encoder_ht_timing(self._h, ht, 4, C.byref(nh), C.byref(ntop)), "encoder_ht_timing")
        return dict(convert_ms=t[0], dwt_ms=t[1], ht_ms=t[2], total_ms=t[3], dwt_levels_ms=[lv[i] for i in range(n.value)],
                    ht_launches_ms=[ht[i] for i in range(nh.value)])

    def top_blocks(self):
        """number of block descriptors coded on the side stream (0 = no overlap)"""
        ht = (C.c_float * 4)(); nh = C.c_uint32(); ntop = C.c_uint32()
        check(self._lib.ojphgpu_encoder_ht_timing(self._h, ht, 4, C.byref(nh), C.byref(ntop)), "encoder_ht_timing")
        return int(ntop.value)


class Decoder:
    """Whole-frame decoder bound to one parsed codestream layout (ojphgpu_decoder)."""

    def __init__(self, codestream, device=0, resilient=False, tiles=None, skip_res=None, region=None):
        """codestream: bytes, or a list of codestreams of same-shaped frames (batch decoder, output
        [B,C,H,W]).  tiles=(first, count) restricts the decoder to a run of tiles (multi-GPU sharding).
        skip_res=n or (for_data, for_recon): reduced-resolution decoding (codestream::restrict_input_resolution).
        region=(x0, y0, w, h): decode that rectangle of the reference grid (relative to the image origin) only, applied after
        skip_res (Plan.restrict_region); the frame is the region's."""
        torch = _torch()
        self.device = device
        self.resilient = resilient
        streams = list(codestream) if isinstance(codestream, (list, tuple)) else [codestream]
        self.frames = len(streams)
        self.plans = [parse_codestream(cs, resilient) for cs in streams]
        if skip_res:
            a, b = (skip_res, skip_res) if isinstance(skip_res, int) else skip_res
            for pl in self.plans:
                pl.restrict_resolution(a, b)
        if region is not None:
            for pl in self.plans:
                pl.restrict_region(*region)
        self.plan = self.plans[0]
        self.tiles = (0, self.plan.num_tiles) if tiles is None else (int(tiles[0]), int(tiles[1]))
        self._lib = capi.lib()
        self._h = C.c_void_p()
        with torch.cuda.device(device):
            if self.frames > 1:
                assert tiles is None, "a batch decoder decodes whole frames"
                arr = (C.c_void_p * self.frames)(*[pl.handle.value if hasattr(pl.handle, "value") else pl.handle for pl in self.plans])
                check(self._lib.ojphgpu_decoder_create_batch(arr, self.frames, device, _stream_ptr(torch, device),
                                                             C.byref(self._h)), "decoder_create_batch")
            else:
                check(self._lib.ojphgpu_decoder_create_tiles(self.plan.handle, device, _stream_ptr(torch, device),
                                                             self.tiles[0], self.tiles[1], C.byref(self._h)),
                      "decoder_create")
        fs = self.plan.frame_shape
        self.shape = fs if self.frames == 1 else (self.frames,) + fs
        for f, cs in enumerate(streams):
            self.upload(cs, f)

    def __del__(self):
        try:
            if self._h:
                self._lib.ojphgpu_decoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def upload(self, codestream: bytes, frame=0):
        buf = np.frombuffer(codestream, dtype=np.uint8)
        check(self._lib.ojphgpu_decoder_upload_frame(self._h, frame, buf.ctypes.data, len(codestream)), "decoder_upload")
        _torch().cuda.synchronize(self.device)   # the host buffer may go away after this call

    def run_device(self, d_image=None, dtype=None):
        """dtype / d_image.dtype torch.int16 / uint16 or torch.int8 / uint8: samples in 16- / 8-bit containers.
        Asynchronous: the launches are enqueued on the decoder's stream.  The run is COLLECTED by failed_blocks() (decode()
        does it): that is where a block's verdict is read, and where a frame is decoded once more through the separate
        launches if the one-launch block decoder ran out of patience on a chip held by others (fused_retries() counts; it
        has not happened on an idle or a shared chip so far) -- a caller that reads d_image on the device without
        collecting the run takes that frame as it is."""
        torch = _torch()
        if d_image is None:
            alloc = torch.empty if self.tiles == (0, self.plan.num_tiles) else torch.zeros
            d_image = alloc(self.shape, dtype=dtype or torch.int32, device="cuda:%d" % self.device)
        if d_image.dtype in (torch.int16, torch.uint16):
            check(self._lib.ojphgpu_decoder_run_device16(self._h, C.c_void_p(d_image.data_ptr())), "decoder_run_device16")
        elif d_image.dtype in (torch.int8, torch.uint8):
            check(self._lib.ojphgpu_decoder_run_device8(self._h, C.c_void_p(d_image.data_ptr())), "decoder_run_device8")
        else:
            check(self._lib.ojphgpu_decoder_run_device(self._h, C.c_void_p(d_image.data_ptr())), "decoder_run_device")
        return d_image

    def set_timing(self, per_launch: bool):
        check(self._lib.ojphgpu_decoder_set_timing(self._h, int(per_launch)), "decoder_set_timing")

    def pending(self):
        """a released run of this decoder has not been settled yet (by failed_blocks, timing, set_timing, giveup_epoch, a run
        of the other schedule); include/ojphgpu.h, ojphgpu_decoder_run_device"""
        n = C.c_int()
        check(self._lib.ojphgpu_decoder_pending(self._h, C.byref(n)), "decoder_pending")
        return bool(n.value)

    def failed_blocks(self):
        n = C.c_uint32()
        check(self._lib.ojphgpu_decoder_failed_blocks(self._h, C.byref(n)), "decoder_failed_blocks")
        return int(n.value)

    def region_info(self):
        """-> dict(blocks decoded, blocks of the plan, codestream bytes uploaded per frame, tiles touched)"""
        out = (C.c_uint64 * 4)()
        check(self._lib.ojphgpu_decoder_region_info(self._h, out), "decoder_region_info")
        return dict(blocks=int(out[0]), plan_blocks=int(out[1]), upload_bytes=int(out[2]), tiles=int(out[3]))

    def fused_retries(self):
        """runs of this decoder that were repeated through the separate launches (see ojphgpu_decoder_failed_blocks)"""
        n = C.c_uint32()
        check(self._lib.ojphgpu_decoder_fused_retries(self._h, C.byref(n)), "decoder_fused_retries")
        return int(n.value)

    def giveup_epoch(self):
        """-> (last_giveup, current): the number of one-launch block-decoder runs enqueued so far, and the number of the newest
        one whose wait ran out (0: none); synchronises the stream.  Brackets a series of uncollected runs (bench.py)."""
        g, c = C.c_uint32(), C.c_uint32()
        check(self._lib.ojphgpu_decoder_giveup_epoch(self._h, C.byref(g), C.byref(c)), "decoder_giveup_epoch")
        return int(g.value), int(c.value)

    def decode(self) -> np.ndarray:
        img = self.run_device()
        failed = self.failed_blocks()
        if failed and not self.resilient:
            raise capi.OjphError(capi.E_BLOCK, "%d code-blocks" % failed)   # ojph_codeblock.cpp:214-224
        return img.cpu().numpy()

    def timing(self):
        t = (C.c_float * 4)()
        check(self._lib.ojphgpu_decoder_timing(self._h, t), "decoder_timing")
        lv = (C.c_float * 40)(); n = C.c_uint32()
        check(self._lib.ojphgpu_decoder_level_timing(self._h, lv, 40, C.byref(n)), "decoder_level_timing")
        ht = (C.c_float * 3)()
        check(self._lib.ojphgpu_decoder_ht_timing(self._h, ht), "decoder_ht_timing")
        return dict(ht_ms=t[0], dwt_ms=t[1], convert_ms=t[2], total_ms=t[3], dwt_levels_ms=[lv[i] for i in range(n.value)],
                    ht_prep_ms=ht[0], ht_step1_ms=ht[1], ht_step2_ms=ht[2])


class MultiEncoder:
    """One frame over several GPUs of this process (ojphgpu_multi_encoder: include/ojphgpu.h section 8): contiguous runs
    of tiles, one host thread + one encoder object per device, tile-parts copied from every GPU straight to their place
    in one pinned host buffer.  devices: list of device numbers (a number may repeat)."""

    def __init__(self, params=None, plan=None, devices=(0,)):
        torch = _torch()
        self.plan = plan if plan is not None else Plan(params)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(self._lib.ojphgpu_multi_encoder_create(self.plan.handle, devs, len(devices), C.byref(self._h)), "multi_encoder_create")
        self._out = torch.empty(max(self.plan.frame_elems * 4, 1 << 20) + (1 << 20), dtype=torch.uint8).pin_memory()
        n, per = C.c_uint32(), (C.c_uint32 * 64)()
        check(self._lib.ojphgpu_multi_encoder_workers(self._h, C.byref(n), per, 64), "multi_encoder_workers")
        self.tiles_per_worker = [int(per[i]) for i in range(n.value)]

    def __del__(self):
        try:
            if self._h:
                self._lib.ojphgpu_multi_encoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def encode(self, image, copy=True):
        """image: numpy array / pinned torch tensor in the frame layout, int32 or in 16- / 8-bit containers (the dtype says
        which: half / a quarter of the bytes over every device's link) -> the codestream (bytes; copy=False: a view of the
        encoder's pinned buffer, valid until the next call)"""
        torch = _torch()
        if hasattr(image, "data_ptr"):
            t = image
        else:
            a = np.ascontiguousarray(image)
            t = torch.from_numpy(a if a.dtype.itemsize in (1, 2) and a.dtype.kind in "iu" else a.astype(np.int32))
        bits = 8 * t.element_size()
        n = C.c_size_t()
        check(self._lib.ojphgpu_multi_encode_container(self._h, C.c_void_p(t.data_ptr()), bits, C.c_void_p(self._out.data_ptr()),
                                                       self._out.numel(), C.byref(n)), "multi_encode")
        v = self._out[:n.value].numpy()
        return v.tobytes() if copy else v


class MultiDecoder:
    """The decoding mirror of MultiEncoder (ojphgpu_multi_decoder)."""

    def __init__(self, codestream: bytes, devices=(0,), resilient=False, skip_res=None):
        torch = _torch()
        self._lib = capi.lib()
        self._h = C.c_void_p()
        self._cs = np.frombuffer(codestream, np.uint8)
        a, b = (0, 0) if not skip_res else ((skip_res, skip_res) if isinstance(skip_res, int) else skip_res)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(self._lib.ojphgpu_multi_decoder_create(self._cs.ctypes.data, len(codestream), int(resilient), a, b, devs, len(devices),
                                                     C.byref(self._h)), "multi_decoder_create")
        ph = C.c_void_p()
        check(self._lib.ojphgpu_multi_decoder_plan(self._h, C.byref(ph)), "multi_decoder_plan")
        self.plan = Plan(handle=ph, owned=False)
        self.resilient = resilient
        self._img = torch.zeros(self.plan.frame_shape, dtype=torch.int32).pin_memory()

    def __del__(self):
        try:
            if self._h:
                self._lib.ojphgpu_multi_decoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def decode(self, copy=True, dtype=None):
        """dtype np.int16 / np.uint16 / np.int8 / np.uint8: the samples come down in 16- / 8-bit containers"""
        torch = _torch()
        dt = np.dtype(dtype or np.int32)
        if dt.itemsize != 4:
            key = "_img%d" % dt.itemsize
            if not hasattr(self, key):
                setattr(self, key, torch.zeros(self.plan.frame_shape, dtype=torch.int16 if dt.itemsize == 2 else torch.int8).pin_memory())
            img = getattr(self, key)
        else:
            img = self._img
        failed = C.c_uint32()
        check(self._lib.ojphgpu_multi_decode_container(self._h, self._cs.ctypes.data, len(self._cs), C.c_void_p(img.data_ptr()),
                                                       8 * dt.itemsize, C.byref(failed)), "multi_decode")
        v = img.numpy().view(dt) if dt.itemsize != 4 else img.numpy()
        return v.copy() if copy else v


class Transcoder:
    """A codestream recoded to another packaging, quantisation step or byte budget without leaving the coefficient domain
    (ojphgpu_transcoder): the block decoder of the source and the block coder of the output on one arena, no transform and no
    samples in between.  At the source's own step, or one a whole number of octaves coarser, the result is byte for byte the
    direct encode of the original image with the output's parameters; a reversible source is carried over as it is."""

    def __init__(self, codestream: bytes, device=0, resilient=False, max_bytes=0, **kw):
        """codestream: the first source (parsed for the geometry; every later one must have the same).  kw: what changes, as
        plan.transcode_params takes it (qstep, block, prog_order, precinct, precincts, tlm, tileparts).  max_bytes=N: every
        source is recoded to a byte budget (set_budget); an irreversible output needs qstep or a budget."""
        from .plan import transcode_params, transcode_plan
        torch = _torch()
        self.device = device
        self.resilient = bool(resilient)
        self.src_plan = parse_codestream(codestream, resilient)
        self.params = transcode_params(self.src_plan, **kw)
        self.plan = transcode_plan(self.src_plan, self.params)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        with torch.cuda.device(device):
            check(self._lib.ojphgpu_transcoder_create(self.src_plan.handle, self.plan.handle, device, _stream_ptr(torch, device),
                                                      C.byref(self._h)), "transcoder_create")
        self.max_bytes = 0
        self.failed_blocks = 0
        self._cs_len = 0
        if max_bytes:
            self.set_budget(max_bytes)

    def __del__(self):
        try:
            if self._h:
                self._lib.ojphgpu_transcoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_budget(self, max_bytes):
        """Every following source is recoded at the finest step of the rate grid whose codestream is at most max_bytes long
        (Encoder.set_budget, with the transcode of the source in the place of the encode of a frame); 0 switches it off.
        Irreversible outputs only."""
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_transcoder_set_budget(self._h, int(max_bytes)), "transcoder_set_budget")
        self.max_bytes = int(max_bytes)

    def submit(self, codestream: bytes):
        """parses and uploads the source and enqueues its block decoder (with a budget: the band statistics behind it)"""
        buf = np.frombuffer(codestream, dtype=np.uint8)
        self._cs_len = len(codestream)
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_transcoder_submit(self._h, buf.ctypes.data, len(codestream), int(self.resilient)), "transcoder_submit")

    def finish(self) -> bytes:
        """the output codestream of the source submitted last; failed_blocks = the source's blocks that did not decode (zero
        blocks of a resilient transcoder; OjphError E_BLOCK otherwise)"""
        cap = (min(self.max_bytes, self._cs_len * 4) if self.max_bytes else self._cs_len * 2) + 64 * self.plan.num_blocks + (1 << 20)
        out = np.empty(cap, np.uint8)
        n, failed = C.c_size_t(), C.c_uint32()
        with _torch().cuda.device(self.device):
            rc = self._lib.ojphgpu_transcoder_finish(self._h, out.ctypes.data, cap, C.byref(n), C.byref(failed))
            if rc == capi.E_OVERFLOW and n.value > cap:
                cap = int(n.value)
                out = np.empty(cap, np.uint8)
                rc = self._lib.ojphgpu_transcoder_finish(self._h, out.ctypes.data, cap, C.byref(n), C.byref(failed))
        self.failed_blocks = int(failed.value)
        check(rc, "transcoder_finish")
        return out[:n.value].tobytes()

    def transcode(self, codestream: bytes) -> bytes:
        self.submit(codestream)
        return self.finish()

    def rate_info(self):
        """what the last budgeted finish() found, as Encoder.rate_info"""
        info = capi.RateInfo()
        check(self._lib.ojphgpu_transcoder_rate_info(self._h, C.byref(info)), "transcoder_rate_info")
        return {k: getattr(info, k) for k, _ in capi.RateInfo._fields_}

    def timing(self):
        """ms: dict(decode_ms = the block decoder, stats_ms = the band statistics (device events of the last submit), code_ms =
        search and coding, final_ms = download and Tier-2 (host clock of the last finish))"""
        t = (C.c_float * 4)()
        check(self._lib.ojphgpu_transcoder_timing(self._h, t), "transcoder_timing")
        return dict(decode_ms=t[0], stats_ms=t[1], code_ms=t[2], final_ms=t[3])


def transcode(codestream: bytes, device=0, resilient=False, max_bytes=0, **kw) -> bytes:
    """One-shot helper: codestream -> codestream; keyword args as plan.transcode_params, max_bytes=N: to a byte budget"""
    return Transcoder(codestream, device=device, resilient=resilient, max_bytes=max_bytes, **kw).transcode(codestream)


class _BorrowedEncoder(Encoder):
    """The encoder half of a Recoder (ojphgpu_recoder_encoder): the setters and infos of an Encoder over a handle that is
    the recoder's -- nothing is created, run, finished or destroyed through it."""

    def __init__(self, handle, plan, device):
        self.device, self.plan, self.frames = device, plan, 1
        self.tiles = (0, plan.num_tiles)
        self._lib = capi.lib()
        self._h = handle
        self.shape = plan.frame_shape
        self.max_bytes, self.budgets, self.max_sse, self.cap_bytes, self._frame = 0, None, None, 0, None

    def __del__(self):
        self._h = None

    def _refuse(self, *a, **k):
        raise RuntimeError("the encoder half of a Recoder runs and finishes through the Recoder")
    run_device = finish = finish_tiles = finish_tiles_device = encode = set_budgets = _refuse


class _DeviceMemory:
    """device memory somebody else owns, as torch.as_tensor takes it"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = dict(shape=(int(nbytes),), typestr="|u1", data=(int(ptr), False), version=2)


class Recoder:
    """A codestream recoded through the sample domain (ojphgpu_recoder; include/ojphgpu.h section 5e): what Transcoder
    refuses -- another wavelet, other decompositions or tiles, another bit depth, a source at a reduced resolution or
    through a window, and with resample= another chroma format.  One object owns a Decoder (under the view), one int32
    frame in HBM, the fit to the output's depth and range, and an Encoder with its three rate-control modes; the output is
    byte for byte what Encoder(out).encode(fit(Decoder(cs, view).run_device())) writes -- fit(resample(...)) with
    resample="cosited" (pipeline.resample_frame)."""

    def __init__(self, codestream: bytes, device=0, resilient=False, skip_res=None, region=None, max_bytes=0, max_sse=None, min_psnr=None,
                 cap_bytes=0, resample=None, **kw):
        """codestream: the first source (parsed for the geometry; every later one must have the same).  skip_res / region:
        the view, as Decoder takes them.  kw: what changes, as plan.recode_params takes it (bit_depth, bit_depths and every
        make_params keyword).  max_bytes / max_sse / min_psnr / cap_bytes: as Encoder takes them; a quality target is
        measured against the fitted frame.  resample="cosited": downsampling=[(dx, dy), ...] may then sub-sample a
        component by 2 more than the source does, per direction (4:4:4 -> 4:2:2 / 4:2:0: ojphgpu_recoder_create_resampled);
        without it such an output is refused as before."""
        from .plan import recode_params
        torch = _torch()
        if cap_bytes and max_sse is None and min_psnr is None:
            raise ValueError("cap_bytes needs a quality target (max_sse or min_psnr); a byte budget alone is max_bytes")
        self.device = device
        self.resilient = bool(resilient)
        self.src_plan = parse_codestream(codestream, resilient)
        if skip_res:
            a, b = (skip_res, skip_res) if isinstance(skip_res, int) else skip_res
            self.src_plan.restrict_resolution(a, b)
        if region is not None:
            self.src_plan.restrict_region(*region)
        self.params = recode_params(self.src_plan, **kw)
        self.plan = Plan(self.params)
        self._lib = capi.lib()
        self._h = C.c_void_p()
        if resample not in capi.RESAMPLE:
            raise ValueError("resample: None or one of %s" % ", ".join(sorted(k for k in capi.RESAMPLE if k)))
        self.resample = resample
        with torch.cuda.device(device):
            if capi.RESAMPLE[resample] == capi.RESAMPLE_NONE:
                check(self._lib.ojphgpu_recoder_create(self.src_plan.handle, self.plan.handle, device, _stream_ptr(torch, device),
                                                       C.byref(self._h)), "recoder_create")
            else:
                check(self._lib.ojphgpu_recoder_create_resampled(self.src_plan.handle, self.plan.handle, capi.RESAMPLE[resample], device,
                                                                 _stream_ptr(torch, device), C.byref(self._h)), "recoder_create_resampled")
        eh = C.c_void_p()
        check(self._lib.ojphgpu_recoder_encoder(self._h, C.byref(eh)), "recoder_encoder")
        self.encoder = _BorrowedEncoder(eh, self.plan, device)
        self.failed_blocks = 0
        if max_bytes:
            self.set_budget(max_bytes)
        if max_sse is not None or min_psnr is not None:
            self.set_quality(max_sse=max_sse, min_psnr=min_psnr, cap_bytes=cap_bytes)

    def __del__(self):
        try:
            if self._h:
                self.encoder._h = None
                self._lib.ojphgpu_recoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_budget(self, max_bytes):
        """Encoder.set_budget of the encoder half"""
        self.encoder.set_budget(max_bytes)

    def set_quality(self, max_sse=None, min_psnr=None, cap_bytes=0):
        """Encoder.set_quality of the encoder half; the target is measured against the fitted frame"""
        self.encoder.set_quality(max_sse=max_sse, min_psnr=min_psnr, cap_bytes=cap_bytes)

    def rate_info(self):
        return self.encoder.rate_info()

    def quality_info(self):
        return self.encoder.quality_info()

    def capped_info(self):
        return self.encoder.capped_info()

    def submit(self, codestream: bytes):
        """parses and uploads the source and enqueues its decode, the fit and the encoder's run"""
        buf = np.frombuffer(codestream, dtype=np.uint8)
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_recoder_submit(self._h, buf.ctypes.data, len(codestream), int(self.resilient)), "recoder_submit")

    def finish(self) -> bytes:
        """the output codestream of the source submitted last; failed_blocks = the source's blocks that did not decode (zero
        blocks of a resilient recoder; OjphError E_BLOCK otherwise)"""
        e = self.encoder
        cap = self.plan.frame_elems * 3 + 64 * self.plan.num_blocks + (1 << 20)
        if e.max_bytes:
            cap = min(e.max_bytes, self.plan.frame_elems * 4 + 64 * self.plan.num_blocks + (1 << 20))
        out = np.empty(cap, np.uint8)
        n, failed = C.c_size_t(), C.c_uint32()
        with _torch().cuda.device(self.device):
            rc = self._lib.ojphgpu_recoder_finish(self._h, out.ctypes.data, cap, C.byref(n), C.byref(failed))
            if rc == capi.E_OVERFLOW and n.value > cap:
                cap = int(n.value)
                out = np.empty(cap, np.uint8)
                rc = self._lib.ojphgpu_recoder_finish(self._h, out.ctypes.data, cap, C.byref(n), C.byref(failed))
        self.failed_blocks = int(failed.value)
        check(rc, "recoder_finish")
        return out[:n.value].tobytes()

    def recode(self, codestream: bytes) -> bytes:
        self.submit(codestream)
        return self.finish()

    def frame(self):
        """the fitted frame of the last submit, as the encoder half reads it: a torch tensor VIEW of the recoder's memory
        (the output plan's frame_shape -- flat where its components differ in size; int8 / int16 or uint8 / uint16 by the sign of component 0, or int32), valid until the next
        submit; read it after finish(), which is where a repeated decode lands"""
        torch = _torch()
        p, bits = C.c_void_p(), C.c_int()
        check(self._lib.ojphgpu_recoder_frame(self._h, C.byref(p), C.byref(bits)), "recoder_frame")
        signed = self.plan.comp_format(0)[1]
        dt = {8: torch.int8 if signed else torch.uint8, 16: torch.int16 if signed else torch.uint16, 32: torch.int32}[bits.value]
        raw = torch.as_tensor(_DeviceMemory(p.value, self.plan.frame_elems * (bits.value // 8)), device="cuda:%d" % self.device)
        return raw.view(dt).reshape(self.plan.frame_shape)

    def timing(self):
        """ms: dict(decode_ms, fit_ms, encode_ms = the three parts of the last submit (device events), finish_ms = the
        encoder half's finish, searches included (host clock))"""
        t = (C.c_float * 4)()
        with _torch().cuda.device(self.device):
            check(self._lib.ojphgpu_recoder_timing(self._h, t), "recoder_timing")
        return dict(decode_ms=t[0], fit_ms=t[1], encode_ms=t[2], finish_ms=t[3])


def recode(codestream: bytes, device=0, resilient=False, skip_res=None, region=None, max_bytes=0, max_sse=None, min_psnr=None, cap_bytes=0,
           resample=None, **kw) -> bytes:
    """One-shot helper: codestream -> codestream through the sample domain; arguments as Recoder takes them"""
    return Recoder(codestream, device=device, resilient=resilient, skip_res=skip_res, region=region, max_bytes=max_bytes, max_sse=max_sse,
                   min_psnr=min_psnr, cap_bytes=cap_bytes, resample=resample, **kw).recode(codestream)


def encode(image: np.ndarray, device=0, max_bytes=0, max_sse=None, min_psnr=None, cap_bytes=0, truncate_to=0, truncate_level=None, **kw) -> bytes:
    """One-shot helper: image int32 [C,H,W]; keyword args as in plan.make_params (minus sizes); max_bytes=N: coded to a byte
    budget (Encoder.set_budget); max_sse=N / min_psnr=dB: coded to a quality target (Encoder.set_quality), with cap_bytes=N
    under a byte cap; truncate_to=N: a reversible frame under a byte cap (Encoder.set_truncation), truncate_level=j: at a
    fixed level of the truncation ladder."""
    nc, h, w = image.shape
    return Encoder(make_params(w, h, nc, **kw), device=device, max_bytes=max_bytes, max_sse=max_sse, min_psnr=min_psnr, cap_bytes=cap_bytes,
                   truncate_to=truncate_to, truncate_level=truncate_level).encode(image)


def gather_runs(src, runs, staged_len, out=None):
    """the upload of a view as a stage (ojphgpu_gather_runs): src = uint8 tensor on the device (the codestream), runs =
    run_dtype array (Plan.upload_runs), -> uint8 tensor of staged_len bytes: the runs at their places, zeros elsewhere.
    out: a uint8 tensor of at least staged_len bytes to write into (bytes behind staged_len are left alone)"""
    from .plan import run_dtype
    torch = _torch()
    dev = src.device.index or 0
    runs = np.ascontiguousarray(runs, dtype=run_dtype)
    if out is None:
        out = torch.empty(max(int(staged_len), 16), dtype=torch.uint8, device=src.device)
    d_runs = to_device(runs, dev)
    with torch.cuda.device(dev):
        check(capi.lib().ojphgpu_gather_runs(_stream_ptr(torch, dev), C.c_void_p(src.data_ptr()), int(src.numel()), C.c_void_p(d_runs.data_ptr()),
                                             int(runs.size), C.c_void_p(out.data_ptr()), int(staged_len)), "gather_runs")
        torch.cuda.synchronize(dev)       # (d_runs may go away after this call)
    return out


def decode(codestream: bytes, device=0, resilient=False, skip_res=None, region=None) -> np.ndarray:
    return Decoder(codestream, device=device, resilient=resilient, skip_res=skip_res, region=region).decode()


# -------------------------------------------------------------------------------------------------
# stage-level entry points (used by the parity tests; same C ABI the codec objects call)
# -------------------------------------------------------------------------------------------------
def dwt(direction, reversible, descs: np.ndarray, arena, max_w, max_h):
    """descs: dwt_desc_dtype array (host); arena: torch int32/float32/uint32 tensor on the device."""
    torch = _torch()
    dev = arena.device.index
    d = to_device(descs, dev)
    f = capi.lib().ojphgpu_dwt_forward if direction == "forward" else capi.lib().ojphgpu_dwt_inverse
    check(f(_stream_ptr(torch, dev), int(reversible), C.c_void_p(d.data_ptr()), len(descs), max_w, max_h,
            C.c_void_p(arena.data_ptr())), "dwt_" + direction)
    torch.cuda.synchronize(dev)


def dwt_inverse_region(reversible, descs: np.ndarray, regions: np.ndarray, arena, image=None, container=32, colour=False):
    """region synthesis (ojphgpu_dwt_inverse_region_ex): descs dwt_desc_dtype, regions dwt_region_dtype (host, parallel);
    image None = lower levels into the arena, else a device tensor the top level writes into"""
    torch = _torch()
    dev = arena.device.index
    d, r = to_device(descs, dev), to_device(regions, dev)
    check(capi.lib().ojphgpu_dwt_inverse_region_ex(_stream_ptr(torch, dev), int(reversible), C.c_void_p(d.data_ptr()), C.c_void_p(r.data_ptr()),
                                                    len(descs), C.c_void_p(arena.data_ptr()),
                                                    None if image is None else C.c_void_p(image.data_ptr()), int(container), int(colour)),
          "dwt_inverse_region")
    torch.cuda.synchronize(dev)


def convert(direction, params: Params, descs: np.ndarray, image, arena, max_w, max_h, container=32):
    """ojphgpu_convert_forward_ex / _inverse_ex: descs convert_desc_dtype (host; n_tiles * params.num_comps of them, each with
    its own fmt), image a device tensor of `container`-bit samples, arena a device tensor of 32-bit elements"""
    torch = _torch()
    dev = arena.device.index
    d = to_device(descs, dev)
    n_tiles = len(descs) // max(int(params.num_comps), 1)
    f = capi.lib().ojphgpu_convert_forward_ex if direction == "forward" else capi.lib().ojphgpu_convert_inverse_ex
    check(f(_stream_ptr(torch, dev), C.byref(params), C.c_void_p(d.data_ptr()), n_tiles, max_w, max_h,
            C.c_void_p(image.data_ptr()), C.c_void_p(arena.data_ptr()), int(container)), "convert_" + direction)
    torch.cuda.synchronize(dev)


def dwt_image(direction, params: Params, descs: np.ndarray, image, arena, max_w, max_h, container=32, colour=False):
    """ojphgpu_dwt_forward_image_ex / _inverse_image_ex: one level with the sample conversion fused in; descs dwt_desc_dtype
    (host) with src_off / src_pitch inside `image` and reserved = the plane's bit depth | signed << 8"""
    torch = _torch()
    dev = arena.device.index
    d = to_device(descs, dev)
    f = capi.lib().ojphgpu_dwt_forward_image_ex if direction == "forward" else capi.lib().ojphgpu_dwt_inverse_image_ex
    check(f(_stream_ptr(torch, dev), C.byref(params), C.c_void_p(d.data_ptr()), len(descs), max_w, max_h,
            C.c_void_p(image.data_ptr()), C.c_void_p(arena.data_ptr()), int(container), int(bool(colour))), "dwt_image_" + direction)
    torch.cuda.synchronize(dev)


stats_desc_dtype = np.dtype(capi.StatsDesc)


def band_stats(descs: np.ndarray, arena, slots, integer=False):
    """ojphgpu_band_stats: descs stats_desc_dtype (host), arena a device tensor of 32-bit elements -> uint32 [slots, 80]
    half-octave histograms of the magnitudes of the planes' fp32 coefficients.  integer=True: ojphgpu_band_stats_int, the
    planes hold int32 coefficients and bin = the bit length of |v|."""
    torch = _torch()
    dev = arena.device.index
    d = to_device(descs, dev)
    hist = torch.zeros((int(slots), capi.STATS_BINS), dtype=torch.int32, device=arena.device)
    max_w = int(descs["w"].max()) if len(descs) else 0
    max_h = int(descs["h"].max()) if len(descs) else 0
    f = capi.lib().ojphgpu_band_stats_int if integer else capi.lib().ojphgpu_band_stats
    check(f(_stream_ptr(torch, dev), C.c_void_p(d.data_ptr()), len(descs), max_w, max_h,
            C.c_void_p(arena.data_ptr()), C.c_void_p(hist.data_ptr())), "band_stats_int" if integer else "band_stats")
    torch.cuda.synchronize(dev)
    return hist.cpu().numpy().view(np.uint32)


requant_desc_dtype = np.dtype(capi.RequantDesc)
error_comp_dtype = np.dtype(capi.ErrorComp)
frame_err_dtype = np.dtype(capi.FrameErr)


def band_requantise(descs: np.ndarray, src, dst):
    """ojphgpu_band_requantise: descs requant_desc_dtype (host); src, dst device tensors of 32-bit elements (the arenas).
    Writes the w x h samples of every descriptor's plane into dst, in place; src is only read."""
    torch = _torch()
    dev = src.device.index
    d = to_device(descs, dev)
    max_w = int(descs["w"].max()) if len(descs) else 0
    max_h = int(descs["h"].max()) if len(descs) else 0
    check(capi.lib().ojphgpu_band_requantise(_stream_ptr(torch, dev), C.c_void_p(d.data_ptr()), len(descs), max_w, max_h,
                                             C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())), "band_requantise")
    torch.cuda.synchronize(dev)


def frame_error(a, b, comps):
    """ojphgpu_frame_error / _ex: a, b device tensors holding two frames, of one integer dtype (8-, 16- or 32-bit containers) or
    b int32 against a narrower a; comps = [(first_elem, count, is_signed), ...] -> [(sse, pae), ...] per component, exact"""
    torch = _torch()
    assert a.is_cuda and b.is_cuda and a.is_contiguous() and b.is_contiguous()
    assert a.element_size() == b.element_size() or b.element_size() == 4
    dev = a.device.index
    cd = np.zeros(len(comps), error_comp_dtype)
    for i, (first, count, sg) in enumerate(comps):
        cd[i]["first_elem"], cd[i]["count"], cd[i]["is_signed"] = int(first), int(count), int(bool(sg))
    d = to_device(cd, dev)
    out = torch.zeros(max(len(comps), 1) * frame_err_dtype.itemsize, dtype=torch.uint8, device=a.device)
    check(capi.lib().ojphgpu_frame_error_ex(_stream_ptr(torch, dev), C.c_void_p(a.data_ptr()), 8 * a.element_size(), C.c_void_p(b.data_ptr()),
                                            8 * b.element_size(), C.c_void_p(d.data_ptr()), len(comps), C.c_void_p(out.data_ptr())), "frame_error")
    torch.cuda.synchronize(dev)
    r = out.cpu().numpy().view(frame_err_dtype)[:len(comps)]
    return [(int(x["sse"]), int(x["pae"])) for x in r]


fit_comp_dtype = np.dtype(capi.FitComp)


def frame_fit(src, comps, container_bits, out=None):
    """ojphgpu_frame_fit: src an int32 device tensor holding a frame, comps = [(first_elem, count, shift, lo, hi), ...] ->
    the fitted frame in container_bits (8 | 16 | 32)-bit containers, as a uint8 / uint16 / int32 device tensor of src's
    element count (a signed component's elements are int8 / int16 behind that view).  out: a device tensor of that size to
    write into -- elements outside the components' runs are left alone; src itself at 32 bits fits in place; None: zeros"""
    torch = _torch()
    assert src.is_cuda and src.is_contiguous() and src.dtype == torch.int32
    dev = src.device.index
    cd = np.zeros(len(comps), fit_comp_dtype)
    for i, (first, count, shift, lo, hi) in enumerate(comps):
        cd[i]["first_elem"], cd[i]["count"], cd[i]["shift"], cd[i]["lo"], cd[i]["hi"] = int(first), int(count), int(shift), int(lo), int(hi)
    d = to_device(cd, dev)
    if out is None:
        out = torch.zeros(src.numel(), dtype={8: torch.uint8, 16: torch.uint16, 32: torch.int32}[int(container_bits)], device=src.device)
    assert out.is_cuda and out.element_size() * 8 == int(container_bits)
    with torch.cuda.device(dev):
        check(capi.lib().ojphgpu_frame_fit(_stream_ptr(torch, dev), C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), int(container_bits),
                                           C.c_void_p(d.data_ptr()), len(comps)), "frame_fit")
        torch.cuda.synchronize(dev)
    return out


resample_comp_dtype = np.dtype(capi.ResampleComp)


def resample_table(src_plan, out_plan, resample="cosited"):
    """ojphgpu_recoder_resample_table: the plans judged as Recoder(resample=...) judges them, without a device -> the
    components of ojphgpu_frame_resample as a resample_comp_dtype array (OjphError E_INVALID where creation would refuse)"""
    nc = int(out_plan.params.num_comps)
    tab = np.zeros(max(nc, 1), resample_comp_dtype)
    n = C.c_uint32()
    check(capi.lib().ojphgpu_recoder_resample_table(src_plan.handle, out_plan.handle, capi.RESAMPLE[resample], tab.ctypes.data, len(tab),
                                                    C.byref(n)), "recoder_resample_table")
    return tab[:n.value]


def frame_resample(src, comps, container_bits, out=None):
    """ojphgpu_frame_resample: src an int32 device tensor holding a frame, comps = a resample_comp_dtype array or [dict(src_first,
    dst_first, src_w, src_h, dst_w, dst_h, fx, fy, px, py, shift, lo, hi), ...] -> the resampled and fitted frame in
    container_bits (8 | 16 | 32)-bit containers, as a uint8 / uint16 / int32 device tensor (a signed component's elements are
    int8 / int16 behind that view).  out: a device tensor to write into -- elements outside the components' outputs are left
    alone; None: zeros up to the last output element"""
    torch = _torch()
    assert src.is_cuda and src.is_contiguous() and src.dtype == torch.int32
    dev = src.device.index
    if isinstance(comps, np.ndarray):
        cd = np.ascontiguousarray(comps, resample_comp_dtype)
    else:
        cd = np.zeros(len(comps), resample_comp_dtype)
        for i, c in enumerate(comps):
            for k, v in c.items():
                cd[i][k] = int(v)
    d = to_device(cd, dev)
    if out is None:
        size = max([int(c["dst_first"]) + int(c["dst_w"]) * int(c["dst_h"]) for c in cd] + [1])
        out = torch.zeros(size, dtype={8: torch.uint8, 16: torch.uint16, 32: torch.int32}[int(container_bits)], device=src.device)
    assert out.is_cuda and out.element_size() * 8 == int(container_bits)
    with torch.cuda.device(dev):
        check(capi.lib().ojphgpu_frame_resample(_stream_ptr(torch, dev), C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), int(container_bits),
                                                C.c_void_p(d.data_ptr()), len(cd)), "frame_resample")
        torch.cuda.synchronize(dev)
    return out


def colour_table(standard, direction, rgb_depth, ycc_depth, rgb_range="full", ycc_range="narrow"):
    """ojphgpu_colour_table_make (host only): -> pipeline.ColourTable, entry for entry what pipeline.colour_table states"""
    from .pipeline import ColourTable
    t = capi.ColourTable()
    try:
        args = (capi.COLOUR_STANDARD[standard], capi.COLOUR_DIRECTION[direction], int(rgb_depth), int(ycc_depth), capi.COLOUR_RANGE[rgb_range],
                capi.COLOUR_RANGE[ycc_range])
    except KeyError as e:
        raise ValueError("colour_table: %s" % e)
    check(capi.lib().ojphgpu_colour_table_make(*args, C.byref(t)), "colour_table_make")
    return ColourTable(tuple(tuple(int(x) for x in r) for r in t.m), tuple(int(x) for x in t.off), tuple(int(x) for x in t.lo),
                       tuple(int(x) for x in t.hi), int(t.k))


def _colour_stage(name, src, dst_count, table, width, height, fx, fy, rgb_first, ycc_first, dtype, out):
    torch = _torch()
    w, h, fx, fy = int(width), int(height), int(fx), int(fy)
    assert src.is_cuda and src.is_contiguous() and src.element_size() in (1, 2, 4)
    dev = src.device.index or 0
    cw, ch = -(-w // max(fx, 1)), -(-h // max(fy, 1))
    t = capi.ColourTable()
    for c in range(3):
        for i in range(3):
            t.m[c][i] = int(table.m[c][i])
        t.off[c], t.lo[c], t.hi[c] = int(table.off[c]), int(table.lo[c]), int(table.hi[c])
    t.k = int(table.k)
    f = capi.ColourFrame(w, h, fx, fy)
    f.rgb_first[:] = [0, w * h, 2 * w * h] if rgb_first is None else [int(x) for x in rgb_first]
    f.ycc_first[:] = [0, w * h, w * h + cw * ch] if ycc_first is None else [int(x) for x in ycc_first]
    if out is None:
        assert rgb_first is None and ycc_first is None, "%s: planes placed by hand need out=" % name
        out = torch.zeros(dst_count(w, h, cw, ch), dtype=dtype if dtype is not None else src.dtype, device=src.device)
    assert out.is_cuda and out.is_contiguous() and out.element_size() in (1, 2, 4)
    with torch.cuda.device(dev):
        check(getattr(capi.lib(), "ojphgpu_frame_" + name)(_stream_ptr(torch, dev), C.c_void_p(src.data_ptr()), src.element_size() * 8,
                                                           C.c_void_p(out.data_ptr()), out.element_size() * 8, C.byref(f), C.byref(t)), name)
        torch.cuda.synchronize(dev)
    return out


def rgb_to_ycc(d_rgb, table, width, height, fx=1, fy=1, dtype=None, out=None, rgb_first=None, ycc_first=None):
    """ojphgpu_frame_rgb_to_ycc: d_rgb a device tensor of unsigned 8-, 16- or 32-bit containers (whatever the dtype's sign)
    holding the planes R, G, B [H, W], tightly packed one after the other or each from its element of rgb_first; table: a
    pipeline.ColourTable; fx, fy: the chroma cell (1 | 2 each) -> Y [H, W], Cb, Cr [ch, cw] as ONE flat tensor in `dtype`
    (default: d_rgb's), or in `out` (its dtype is the container; only the planes' samples are written), each plane from its
    element of ycc_first (default: one after the other).  pipeline.rgb_to_ycc states the arithmetic."""
    return _colour_stage("rgb_to_ycc", d_rgb, lambda w, h, cw, ch: w * h + 2 * cw * ch, table, width, height, fx, fy, rgb_first, ycc_first, dtype, out)


def ycc_to_rgb(d_ycc, table, width, height, fx=1, fy=1, dtype=None, out=None, rgb_first=None, ycc_first=None):
    """ojphgpu_frame_ycc_to_rgb, the mirror: Y [H, W], Cb, Cr [ch, cw] in d_ycc -> R, G, B [H, W].  pipeline.ycc_to_rgb states
    the arithmetic."""
    return _colour_stage("ycc_to_rgb", d_ycc, lambda w, h, cw, ch: 3 * w * h, table, width, height, fx, fy, rgb_first, ycc_first, dtype, out)


def frame_rechroma(src, dst, width, height, src_cell, dst_cell, src_off=None, dst_off=None):
    """ojphgpu_frame_rechroma: src a device tensor of 8-, 16- (unsigned, whatever the dtype's sign) or 32-bit (int32) containers
    holding Y [H, W] and Cb, Cr of src_cell = (sub_x, sub_y), tightly packed one after the other or each from its element of
    src_off -> the frame with chroma planes of dst_cell in dst, a device tensor of the same container (None: zeros of the
    planes' size; only the planes' samples are written), each plane from its element of dst_off.  pipeline.rechroma_frame
    states the arithmetic.  -> dst"""
    torch = _torch()
    w, h = int(width), int(height)
    assert src.is_cuda and src.element_size() in (1, 2, 4)
    dev = src.device.index or 0
    f = capi.ChromaFrame(w, h, int(src_cell[0]), int(src_cell[1]), int(dst_cell[0]), int(dst_cell[1]))
    sc = -(-w // max(f.sfx, 1)) * -(-h // max(f.sfy, 1))
    dc = -(-w // max(f.dfx, 1)) * -(-h // max(f.dfy, 1))
    f.src_off[:] = [0, w * h, w * h + sc] if src_off is None else [int(x) for x in src_off]
    f.dst_off[:] = [0, w * h, w * h + dc] if dst_off is None else [int(x) for x in dst_off]
    if dst is None:
        assert dst_off is None, "frame_rechroma: planes placed by hand need dst="
        dst = torch.zeros(w * h + 2 * dc, dtype=src.dtype, device=src.device)
    assert dst.is_cuda and dst.element_size() == src.element_size()
    with torch.cuda.device(dev):
        check(capi.lib().ojphgpu_frame_rechroma(_stream_ptr(torch, dev), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.element_size() * 8,
                                                C.byref(f)), "frame_rechroma")
        torch.cuda.synchronize(dev)
    return dst


def dwt_general_image(direction, steps, elem, params: Params, descs: np.ndarray, image, arena, max_w, max_h, K=1.0, container=32):
    """ojphgpu_dwt_forward_general_image / _inverse_general_image: the general lifting kernels' top level with the conversion
    fused in (steps as for dwt_general; elem 0 = int32, 2 = float); descs as for dwt_image"""
    torch = _torch()
    dev = arena.device.index
    d = to_device(descs, dev)
    k = _lift(steps, elem, K, True, True)
    f = capi.lib().ojphgpu_dwt_forward_general_image if direction == "forward" else capi.lib().ojphgpu_dwt_inverse_general_image
    check(f(_stream_ptr(torch, dev), C.byref(k), C.byref(params), C.c_void_p(d.data_ptr()), len(descs), max_w, max_h,
            C.c_void_p(image.data_ptr()), C.c_void_p(arena.data_ptr()), int(container)), "dwt_general_image_" + direction)
    torch.cuda.synchronize(dev)


class _LiftStep(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("e", C.c_int32), ("A", C.c_float)]


class _Lift(C.Structure):
    _fields_ = [("num_steps", C.c_uint32), ("elem", C.c_uint32), ("horz", C.c_uint32), ("vert", C.c_uint32), ("K", C.c_float),
                ("steps", _LiftStep * 16)]


def _lift(steps, elem, K, horz, vert):
    k = _Lift()
    k.num_steps, k.elem, k.horz, k.vert, k.K = len(steps), int(elem), int(bool(horz)), int(bool(vert)), float(K)
    for i, st in enumerate(steps):
        if isinstance(st, (tuple, list)):
            k.steps[i].a, k.steps[i].b, k.steps[i].e = st
        else:
            k.steps[i].A = float(st)
    return k


def dwt_general(direction, steps, elem, descs: np.ndarray, arena, max_w, max_h, K=1.0, horz=True, vert=True):
    """ojphgpu_dwt_forward_general / _inverse_general: steps in synthesis order -- (a, b, e) tuples for a reversible
    kernel, floats for an irreversible one; elem 0 = int32, 1 = int64, 2 = float planes in `arena`."""
    torch = _torch()
    dev = arena.device.index
    d = to_device(descs, dev)
    k = _lift(steps, elem, K, horz, vert)
    f = capi.lib().ojphgpu_dwt_forward_general if direction == "forward" else capi.lib().ojphgpu_dwt_inverse_general
    check(f(_stream_ptr(torch, dev), C.byref(k), C.c_void_p(d.data_ptr()), len(descs), max_w, max_h, C.c_void_p(arena.data_ptr())),
          "dwt_general_" + direction)
    torch.cuda.synchronize(dev)


def ht_encode_kinds(descs: np.ndarray):
    """what the blocks of `descs` are, as the truthful `widths` of ojphgpu_ht_encode_ex (host only; include/ojphgpu.h)"""
    descs = np.ascontiguousarray(descs)
    k = C.c_int()
    check(capi.lib().ojphgpu_ht_encode_kinds(descs.ctypes.data if len(descs) else None, len(descs), C.byref(k)), "ht_encode_kinds")
    return int(k.value)


def ht_encode_launches(n, widths):
    """the launches of ojphgpu_ht_encode_ex over n blocks under `widths`, in issue order (host only, no HIP call): a list of
    dicts of wide (1: ht_encode_wide_kernel<S64 = flag>, 0: ht_encode_kernel<REV = flag, logp>), flag, logp, wgs, per_wg"""
    L = capi.lib()
    cnt = C.c_uint32()
    L.ojphgpu_ht_encode_launches(int(n), int(widths), None, 0, C.byref(cnt))
    out = (C.c_uint32 * (5 * max(cnt.value, 1)))()
    check(L.ojphgpu_ht_encode_launches(int(n), int(widths), out, cnt.value, C.byref(cnt)), "ht_encode_launches")
    return [dict(zip(("wide", "flag", "logp", "wgs", "per_wg"), (int(v) for v in out[5 * i:5 * i + 5]))) for i in range(cnt.value)]


class EncodeStage:
    """ojphgpu_ht_encode_ex as the encoder objects use it: one descriptor array, one scratch, one compacted output with
    `regions` ((nreg, 2) uint32 rows of first byte, bytes; None = the single cursor over out_cap) and the cursor words, all
    made once; launch() codes a range of the descriptors into them.  Out and scratch start filled with SENTINEL, results
    with 0xFFFFFFFF words (a block no launched kernel owns keeps them).  scratch_caps_as_given=False: the slots (data_off,
    scratch_cap) are laid out here, roomy enough for any content, instead of taken from `descs`."""
    SENTINEL = 0xA5

    def __init__(self, descs: np.ndarray, coef, scratch_bytes, out_cap, regions=None, scratch_caps_as_given=True):
        torch = _torch()
        self.torch, self.dev, self.coef = torch, coef.device.index, coef
        descs = np.ascontiguousarray(descs.copy())
        if not scratch_caps_as_given:
            from .csrc_consts import block_scratch_bytes
            off = 0
            for d in descs:
                d["data_off"], d["scratch_cap"] = off, block_scratch_bytes(int(d["w"]), int(d["h"]), 30)
                off += int(d["scratch_cap"])
            scratch_bytes = off
        self.descs, self.n, self.out_cap = descs, len(descs), int(out_cap)
        self.d = to_device(descs, self.dev) if len(descs) else torch.zeros(64, dtype=torch.uint8, device=coef.device)
        self.scratch = torch.full((max(int(scratch_bytes), 16),), self.SENTINEL, dtype=torch.uint8, device=coef.device)
        self.out = torch.full((max(int(out_cap), 16),), self.SENTINEL, dtype=torch.uint8, device=coef.device)
        self.results = torch.full((len(descs) * 2 + 2,), -1, dtype=torch.int32, device=coef.device)
        reg = np.zeros((0, 2), np.uint32) if regions is None else np.ascontiguousarray(np.asarray(regions, np.uint32).reshape(-1, 2))
        self.nreg = len(reg)
        self.regions = to_device(reg, self.dev) if self.nreg else None
        self.counters = torch.zeros(32 * max(self.nreg, 1) + 32, dtype=torch.int32, device=coef.device)

    def launch(self, lo=0, n=None, widths=None, first=None):
        """codes descriptors [lo, lo + n) under `widths` (None: what ht_encode_kinds says of that range); `first` (None: lo) is
        the index of descriptor lo among all blocks and only chooses regions"""
        n = self.n - lo if n is None else int(n)
        if lo < 0 or n < 0 or lo + n > self.n:
            raise ValueError("the range is not inside the descriptor array")
        if widths is None:
            widths = ht_encode_kinds(self.descs[lo:lo + n])
        ptr = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        with self.torch.cuda.device(self.dev):
            check(capi.lib().ojphgpu_ht_encode_ex(_stream_ptr(self.torch, self.dev), ptr(self.d, lo * self.descs.dtype.itemsize), n,
                                                  ptr(self.coef), ptr(self.scratch), ptr(self.out), self.out_cap, ptr(self.results, 8 * lo),
                                                  ptr(self.counters), ptr(self.counters, 4), int(widths),
                                                  ptr(self.regions) if self.nreg else None, self.nreg, int(lo if first is None else first)),
                  "ht_encode_ex")

    def read(self):
        """(results (n, 2) uint32, the whole out buffer, status, the whole scratch buffer, cursor word per region (one for none))"""
        self.torch.cuda.synchronize(self.dev)
        res = self.results.cpu().numpy()[:self.n * 2].view(np.uint32).reshape(-1, 2).copy()
        cnt = self.counters.cpu().numpy().view(np.uint32)
        return res, self.out.cpu().numpy()[:self.out_cap].copy(), int(cnt[1]), self.scratch.cpu().numpy().copy(), cnt[0:32 * max(self.nreg, 1):32].copy()


_ENC_KW = dict(widths=None, regions=None, first=0, scratch_caps_as_given=True)


def ht_encode(descs: np.ndarray, coef, scratch_bytes, out_cap, **kw):
    """Returns (results array, out bytes tensor (host numpy), status).

    With any of the keyword arguments widths=None, regions=None, first=0, scratch_caps_as_given=True: one launch of
    ojphgpu_ht_encode_ex through an EncodeStage (which see), returning its read(): (results, the whole out buffer, status,
    the whole scratch buffer, the regions' cursor words), untouched bytes of out and scratch holding EncodeStage.SENTINEL."""
    if kw:
        if set(kw) - set(_ENC_KW):
            raise TypeError("ht_encode: unknown keyword argument(s) %s" % sorted(set(kw) - set(_ENC_KW)))
        a = dict(_ENC_KW, **kw)
        st = EncodeStage(descs, coef, scratch_bytes, out_cap, a["regions"], a["scratch_caps_as_given"])
        st.launch(0, len(descs), a["widths"], a["first"])
        return st.read()
    torch = _torch()
    dev = coef.device.index
    d = to_device(descs, dev)
    scratch = torch.zeros(max(int(scratch_bytes), 16), dtype=torch.uint8, device=coef.device)
    out = torch.zeros(max(int(out_cap), 16), dtype=torch.uint8, device=coef.device)
    results = torch.zeros(len(descs) * 2 + 2, dtype=torch.int32, device=coef.device)
    counters = torch.zeros(4, dtype=torch.int32, device=coef.device)
    check(capi.lib().ojphgpu_ht_encode(_stream_ptr(torch, dev), C.c_void_p(d.data_ptr()), len(descs),
                                       C.c_void_p(coef.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                       C.c_void_p(out.data_ptr()), int(out_cap), C.c_void_p(results.data_ptr()),
                                       C.c_void_p(counters.data_ptr()), C.c_void_p(counters.data_ptr() + 4)),
          "ht_encode")
    torch.cuda.synchronize(dev)
    res = results.cpu().numpy()[:len(descs) * 2].view(np.uint32).reshape(-1, 2)
    cnt = counters.cpu().numpy().view(np.uint32)
    return res, out.cpu().numpy()[:int(cnt[0])], int(cnt[1])


def ht_decode(descs: np.ndarray, data: np.ndarray, coef):
    torch = _torch()
    dev = coef.device.index
    L = capi.lib()
    descs = np.ascontiguousarray(descs.copy())
    q, a = C.c_uint64(), C.c_uint64()             # per-quad record / aux offsets (see include/ojphgpu.h)
    check(L.ojphgpu_ht_decode_layout(descs.ctypes.data, len(descs), C.byref(q), C.byref(a)), "ht_decode_layout")
    qoff, aoff = int(q.value), int(a.value)
    d = to_device(descs, dev)
    dd = to_device(np.concatenate([np.asarray(data, np.uint8), np.zeros(64, np.uint8)]), dev)
    status = torch.zeros(len(descs) + 16, dtype=torch.uint8, device=coef.device)
    quads = torch.zeros(qoff + 16, dtype=torch.int32, device=coef.device)
    aux = torch.zeros(aoff + 16, dtype=torch.int32, device=coef.device)
    check(L.ojphgpu_ht_decode(_stream_ptr(torch, dev), C.c_void_p(d.data_ptr()), len(descs),
                              C.c_void_p(dd.data_ptr()), C.c_void_p(coef.data_ptr()),
                              C.c_void_p(quads.data_ptr()), C.c_void_p(aux.data_ptr()),
                              C.c_void_p(status.data_ptr())),
          "ht_decode")
    torch.cuda.synchronize(dev)
    return status.cpu().numpy()[:len(descs)]


def ht_decode_kinds(descs: np.ndarray):
    """what the blocks of `descs` are, as the `kinds` of ojphgpu_ht_decode_step2_kinds (host only; include/ojphgpu.h)"""
    descs = np.ascontiguousarray(descs)
    k = C.c_int()
    check(capi.lib().ojphgpu_ht_decode_kinds(descs.ctypes.data if len(descs) else None, len(descs), C.byref(k)), "ht_decode_kinds")
    return int(k.value)


def ht_decode_launches(n, kinds=0):
    """what the separate launches over n blocks of `kinds` are under this process's OJPHGPU_S1_CH / OJPHGPU_DEC_PREP /
    OJPHGPU_DEC_DUAL (host only): dict of prep, ch, wgs1 (step 1: form, CH, workgroups), multi, tx, wd, nb, wgs2, per_wg
    (step 2: multi or single kernel, its TX, WD, NB, workgroups, blocks per workgroup)"""
    out = (C.c_uint32 * 9)()
    check(capi.lib().ojphgpu_ht_decode_launches(int(n), int(kinds), out), "ht_decode_launches")
    return dict(zip(("prep", "ch", "wgs1", "multi", "tx", "wd", "nb", "wgs2", "per_wg"), (int(v) for v in out)))


class SeparateScratch:
    """The scratch of the separate launches (prep, step 1, step 2) for up to max_blocks blocks, quad_elems record words and
    aux_elems words of flat strings: allocated and zeroed once, here, never again -- a run finds what the runs before left."""

    def __init__(self, max_blocks, quad_elems, aux_elems, device=0):
        torch = _torch()
        dev = torch.device("cuda", device)
        self.max_blocks, self.quad_elems, self.aux_elems, self.device, self.runs = int(max_blocks), int(quad_elems), int(aux_elems), device, 0
        self.quads = torch.zeros(self.quad_elems + 16, dtype=torch.int32, device=dev)
        self.aux = torch.zeros(self.aux_elems + 16, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.max_blocks + 16, dtype=torch.uint8, device=dev)


def ht_decode_separate(descs: np.ndarray, data: np.ndarray, coef, scratch: SeparateScratch, kinds=None):
    """prep, step 1 and step 2 of `descs` (cleanup passes only: no refinement launch, no 64-bit path) on a scratch that
    earlier runs have used, step 2 with `kinds` (None: what ht_decode_kinds says of these blocks; a caller may pass a valid
    coarsening of that, include/ojphgpu.h); returns status[:n]"""
    torch = _torch()
    dev = coef.device.index
    L = capi.lib()
    n = len(descs)
    descs = np.ascontiguousarray(descs.copy())
    q, a = C.c_uint64(), C.c_uint64()
    check(L.ojphgpu_ht_decode_layout(descs.ctypes.data, n, C.byref(q), C.byref(a)), "ht_decode_layout")
    if n > scratch.max_blocks or int(q.value) > scratch.quad_elems or int(a.value) > scratch.aux_elems or dev != scratch.device:
        raise ValueError("the SeparateScratch is too small for this launch or on another device")
    if kinds is None:
        kinds = ht_decode_kinds(descs)
    d = to_device(descs, dev)
    dd = to_device(np.concatenate([np.asarray(data, np.uint8), np.zeros(64, np.uint8)]), dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        s = _stream_ptr(torch, dev)
        check(L.ojphgpu_ht_decode_prep(s, ptr(d), n, ptr(dd), ptr(scratch.aux)), "ht_decode_prep")
        check(L.ojphgpu_ht_decode_step1(s, ptr(d), n, ptr(dd), ptr(scratch.aux), ptr(scratch.quads), ptr(scratch.status)), "ht_decode_step1")
        check(L.ojphgpu_ht_decode_step2_kinds(s, ptr(d), n, ptr(dd), ptr(scratch.quads), ptr(coef), ptr(scratch.status), int(kinds)),
              "ht_decode_step2_kinds")
    scratch.runs += 1
    torch.cuda.synchronize(dev)
    return scratch.status.cpu().numpy()[:n].copy()


def ht_decode_fused_shape(n, cus=0):
    """how the fused launch deals n blocks out on `cus` compute units under this process's OJPHGPU_FUSED_SHAPE / _RINGS
    (host only): dict of shape, ch, wgw, n1, per_wave, wwgs, nr, able (n1 <= cus), want (per_wave before the cap of 8)"""
    out = (C.c_uint32 * 9)()
    check(capi.lib().ojphgpu_ht_decode_fused_shape(int(n), int(cus), out), "ht_decode_fused_shape")
    return dict(zip(("shape", "ch", "wgw", "n1", "per_wave", "wwgs", "nr", "able", "want"), (int(v) for v in out)))


def ht_decode_fused_slices(max_h):
    """the fused launch's slices of quad rows for a tallest block of max_h rows (host only): [(lo, hi), ...]"""
    L = capi.lib()
    cnt = C.c_uint32()
    L.ojphgpu_ht_decode_fused_slices(int(max_h), None, 0, C.byref(cnt))
    out = (C.c_uint32 * (2 * max(cnt.value, 1)))()
    check(L.ojphgpu_ht_decode_fused_slices(int(max_h), out, cnt.value, C.byref(cnt)), "ht_decode_fused_slices")
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(cnt.value)]


def ht_decode_layout(descs: np.ndarray):
    """(quad_elems, aux_elems) ojphgpu_ht_decode_layout asks for these descriptors (a copy is laid out, not `descs`)"""
    descs = np.ascontiguousarray(descs.copy())
    q, a = C.c_uint64(), C.c_uint64()
    check(capi.lib().ojphgpu_ht_decode_layout(descs.ctypes.data, len(descs), C.byref(q), C.byref(a)), "ht_decode_layout")
    return int(q.value), int(a.value)


class FusedScratch:
    """The scratch of ojphgpu_ht_decode_fused for launches of up to max_blocks blocks and quad_elems record words: records,
    the state (zeroed once, here) and the status bytes with the RETRY word behind them; counts the epoch of the runs."""

    def __init__(self, max_blocks, quad_elems, device=0):
        torch = _torch()
        dev = torch.device("cuda", device)
        self.max_blocks, self.quad_elems, self.device, self.epoch = int(max_blocks), int(quad_elems), device, 0
        self.quads = torch.zeros(self.quad_elems + 16, dtype=torch.int32, device=dev)
        self.state = torch.zeros(int(capi.lib().ojphgpu_ht_decode_fused_state_words(self.max_blocks)), dtype=torch.int32, device=dev)
        self.status = torch.zeros(((self.max_blocks + 3) & ~3) + 4, dtype=torch.uint8, device=dev)


def ht_decode_fused(descs: np.ndarray, data: np.ndarray, coef, scratch: FusedScratch, reversible, cus=0):
    """step 1 + step 2 of `descs` in the one fused launch, dealt out for `cus` compute units (0: the device's), on a scratch
    that earlier runs have used; returns (status[:n], the RETRY word, the run's epoch).  Raises OjphError(E_INVALID) where
    the launch is unable to run (more step-1 workgroups than `cus`)."""
    torch = _torch()
    dev = coef.device.index
    L = capi.lib()
    n = len(descs)
    descs = np.ascontiguousarray(descs.copy())
    q, a = C.c_uint64(), C.c_uint64()
    check(L.ojphgpu_ht_decode_layout(descs.ctypes.data, n, C.byref(q), C.byref(a)), "ht_decode_layout")
    if n > scratch.max_blocks or int(q.value) > scratch.quad_elems or dev != scratch.device:
        raise ValueError("the FusedScratch is too small for this launch or on another device")
    max_h = int(descs["h"].max()) if n else 0
    d = to_device(descs, dev)
    dd = to_device(np.concatenate([np.asarray(data, np.uint8), np.zeros(64, np.uint8)]), dev)
    epoch = scratch.epoch + 1
    with torch.cuda.device(dev):
        check(L.ojphgpu_ht_decode_fused(_stream_ptr(torch, dev), C.c_void_p(d.data_ptr()), n, C.c_void_p(dd.data_ptr()),
                                        C.c_void_p(coef.data_ptr()), C.c_void_p(scratch.quads.data_ptr()),
                                        C.c_void_p(scratch.state.data_ptr()), C.c_void_p(scratch.status.data_ptr()), epoch,
                                        max(max_h, 1), 1 if reversible else 0, int(cus)), "ht_decode_fused")
    scratch.epoch = epoch
    torch.cuda.synchronize(dev)
    st = scratch.status.cpu().numpy()
    r = (n + 3) & ~3
    return st[:n].copy(), int(st[r:r + 4].view(np.uint32)[0]), epoch


def unpack_pixels(pixels, num_comps=None, big_endian=False, dtype=None, out=None):
    """pixel-interleaved samples on the device ([H,W,C] uint8 / uint16 tensor -- for big-endian 16-bit data the tensor
    holds the file's bytes as they are) -> planes [C,H,W] in `dtype` (uint8 / int16 / uint16 / int32; default: as the
    input), or in `out` (contiguous, at least C * H * W elements, of which the first C * H * W are written; its dtype is the
    container).  ojphgpu_unpack_pixels: what the reference's image readers do sample by sample on the host."""
    torch = _torch()
    assert pixels.is_cuda and pixels.is_contiguous() and pixels.dim() == 3
    h, w, c = pixels.shape
    bits = pixels.element_size() * 8
    assert bits in (8, 16)
    if out is None:
        out = torch.empty((c, h, w), dtype=dtype if dtype is not None else (torch.uint8 if bits == 8 else torch.int16), device=pixels.device)
    assert out.is_cuda and out.is_contiguous() and out.device == pixels.device and out.numel() >= c * h * w
    check(capi.lib().ojphgpu_unpack_pixels(_stream_ptr(torch, pixels.device.index or 0), C.c_void_p(pixels.data_ptr()),
                                           C.c_void_p(out.data_ptr()), w, h, c, bits, int(bool(big_endian)), out.element_size() * 8),
          "unpack_pixels")
    return out.reshape(-1)[:c * h * w].reshape(c, h, w)


def _bits_bytes(n, bits):
    """the bytes of a bit string of n samples: whole groups of 32 samples"""
    return (int(n) + 31) // 32 * 4 * int(bits)


def unpack_bits(d_packed, bits, n, dtype=None, out=None):
    """a bit string on the device (pipeline.pack_bits' layout: n samples of `bits` = 10 | 12 | 14 bits, padded to whole groups
    of 32 samples; a contiguous tensor whose first byte is 4-byte aligned) -> the n samples in `dtype` (int16 / uint16 /
    int32; default int16), or in `out` (contiguous, at least n elements, of which the first n are written; its dtype is the
    container).  ojphgpu_unpack_bits."""
    torch = _torch()
    n, bits = int(n), int(bits)
    assert d_packed.is_cuda and d_packed.is_contiguous()
    if out is None:
        out = torch.empty(max(n, 1), dtype=dtype if dtype is not None else torch.int16, device=d_packed.device)
    assert out.is_cuda and out.is_contiguous() and out.device == d_packed.device and out.numel() >= n
    if bits in (10, 12, 14):                              # (any other width: the library refuses it)
        assert d_packed.numel() * d_packed.element_size() >= _bits_bytes(n, bits), "unpack_bits: the bit string is shorter than its groups"
    check(capi.lib().ojphgpu_unpack_bits(_stream_ptr(torch, d_packed.device.index or 0), C.c_void_p(d_packed.data_ptr()),
                                         C.c_void_p(out.data_ptr()), n, bits, out.element_size() * 8), "unpack_bits")
    return out.reshape(-1)[:n]


def pack_bits(d_samples, bits, out=None):
    """the way back: samples on the device (a contiguous int16 / uint16 / int32 tensor, flattened) -> the bit string as a uint8
    tensor of whole groups of 32 samples, every sample clamped to [0, 2^bits - 1], the padding samples of the last group zero;
    `out`: a contiguous uint8 tensor of at least that many bytes, 4-byte aligned (bytes behind the groups are left alone).
    ojphgpu_pack_bits."""
    torch = _torch()
    bits = int(bits)
    assert d_samples.is_cuda and d_samples.is_contiguous()
    n = d_samples.numel()
    nbytes = _bits_bytes(n, bits)
    if out is None:
        out = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=d_samples.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.device == d_samples.device
    if bits in (10, 12, 14):
        assert out.numel() >= nbytes, "pack_bits: the destination is shorter than the groups"
    check(capi.lib().ojphgpu_pack_bits(_stream_ptr(torch, d_samples.device.index or 0), C.c_void_p(d_samples.data_ptr()),
                                       C.c_void_p(out.data_ptr()), n, d_samples.element_size() * 8, bits), "pack_bits")
    return out.reshape(-1)[:nbytes]


t2_job_dtype = np.dtype(capi.T2Job)


def assemble(jobs, blob, data, out):
    """codestream assembly as a stage (ojphgpu_assemble): jobs = t2_job_dtype array (host) -- job i copies n bytes from blob
    (blob != 0) or data (blob == 0) at src to out at dst; blob, data, out: contiguous uint8 tensors on one device, blob and data
    of a multiple of 4 bytes (the kernel reads the aligned dwords around a job's ends).  Every job is checked against the
    tensors here, on the host: one that leaves them raises ValueError and nothing is launched.  Returns out."""
    torch = _torch()
    jobs = np.ascontiguousarray(jobs, dtype=t2_job_dtype)
    for name, t in (("blob", blob), ("data", data), ("out", out)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.device == out.device):
            raise ValueError("assemble: %s is not a contiguous uint8 tensor on the destination's device" % name)
    for name, t in (("blob", blob), ("data", data)):
        if t.numel() == 0 or t.numel() % 4 or t.data_ptr() % 4:
            raise ValueError("assemble: %s is not a whole number of aligned dwords" % name)
    if (jobs["src"] >= 1 << 62).any() or (jobs["dst"] >= 1 << 62).any():
        raise ValueError("assemble: a job's offset is beyond any tensor")
    n, src, dst = (jobs[k].astype(np.int64) for k in ("n", "src", "dst"))
    if (src + n > np.where(jobs["blob"] != 0, blob.numel(), data.numel())).any():
        raise ValueError("assemble: a job reads beyond its source")
    if (dst + n > out.numel()).any():
        raise ValueError("assemble: a job writes beyond the destination")
    dev = out.device.index or 0
    d_jobs = to_device(jobs, dev)
    with torch.cuda.device(dev):
        check(capi.lib().ojphgpu_assemble(_stream_ptr(torch, dev), C.c_void_p(d_jobs.data_ptr()), int(jobs.size), C.c_void_p(blob.data_ptr()),
                                          C.c_void_p(data.data_ptr()), C.c_void_p(out.data_ptr())), "assemble")
        torch.cuda.synchronize(dev)       # (d_jobs may go away after this call)
    return out


def copy_to_host(dst, src, nbytes):
    """the pipes' copy kernel as a stage (ojphgpu_copy_to_host): nbytes bytes from src to dst, contiguous tensors on one device
    whose first bytes are 16-byte aligned (otherwise the library refuses: E_INVALID).  A byte count beyond either tensor raises
    ValueError and nothing is launched.  Returns dst."""
    torch = _torch()
    nbytes = int(nbytes)
    for name, t in (("dst", dst), ("src", src)):
        if not (t.is_cuda and t.is_contiguous() and t.device == dst.device):
            raise ValueError("copy_to_host: %s is not a contiguous tensor on the destination's device" % name)
        if nbytes < 0 or nbytes > t.numel() * t.element_size():
            raise ValueError("copy_to_host: %d bytes are more than %s holds" % (nbytes, name))
    dev = dst.device.index or 0
    with torch.cuda.device(dev):
        check(capi.lib().ojphgpu_copy_to_host(_stream_ptr(torch, dev), C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes), "copy_to_host")
        torch.cuda.synchronize(dev)
    return dst


def _video_args(family, fmt, width, height, bit_depth):
    """a video stage's format name (of its family), depth and frame -> (code, depth, w, h, row_bytes, chroma_offset, frame_bytes)"""
    from .pipeline import _format, _layout
    w, h = int(width), int(height)
    return _format(family, fmt, bit_depth) + (w, h) + _layout(family, fmt, w, h)


def _video_dtype(torch, fmt):
    """an unpack stage's container when none is asked for: uint8 for the formats whose depth column ends at 8 bits"""
    from .pipeline import _VIDEO_TABLE
    return torch.uint8 if _VIDEO_TABLE[fmt][4] == 8 else torch.int16


def unpack_video(d_buf, fmt, width, height, bit_depth=None, dtype=None, out=None):
    """a 4:2:2 video buffer on the device (uint8 tensor of the format's frame_bytes, 16-byte aligned; fmt = "uyvy" | "yuy2" |
    "v210" | "y210" | "y212" | "y216", pipeline.pack_video's layout) -> the frame's planes as ONE flat tensor, Y [H,W] then Cb
    and Cr [H,ceil(W/2)], in `dtype` (uint8 -- the 8-bit formats only -- / int16 / uint16 / int32; default: uint8 for the
    8-bit formats, else int16), or in `out` (contiguous, at least that many elements; its dtype is the container).
    ojphgpu_unpack_video."""
    torch = _torch()
    code, b, w, h, row, _, total = _video_args(422, fmt, width, height, bit_depth)
    n = w * h + 2 * ((w + 1) // 2) * h
    assert d_buf.is_cuda and d_buf.is_contiguous() and d_buf.numel() * d_buf.element_size() >= total
    if out is None:
        out = torch.empty(n, dtype=dtype if dtype is not None else _video_dtype(torch, fmt), device=d_buf.device)
    assert out.is_cuda and out.is_contiguous() and out.numel() >= n
    check(capi.lib().ojphgpu_unpack_video(_stream_ptr(torch, d_buf.device.index or 0), code, C.c_void_p(d_buf.data_ptr()),
                                          C.c_void_p(out.data_ptr()), w, h, b, out.element_size() * 8), "unpack_video")
    return out.reshape(-1)[:n]


def pack_video(d_planes, fmt, width, height, bit_depth=None, out=None):
    """the way back: the planes as one flat tensor (the frame layout above; uint8 / int16 / uint16 / int32) -> uint8
    [H, row_bytes], clamped to [0, 2^bit_depth - 1], every padding position zero; `out`: a contiguous uint8 tensor of at
    least frame_bytes, 16-byte aligned.  ojphgpu_pack_video."""
    torch = _torch()
    code, b, w, h, row, _, total = _video_args(422, fmt, width, height, bit_depth)
    assert d_planes.is_cuda and d_planes.is_contiguous() and d_planes.numel() >= w * h + 2 * ((w + 1) // 2) * h
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=d_planes.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= total
    check(capi.lib().ojphgpu_pack_video(_stream_ptr(torch, d_planes.device.index or 0), code, C.c_void_p(d_planes.data_ptr()),
                                        C.c_void_p(out.data_ptr()), w, h, d_planes.element_size() * 8, b), "pack_video")
    return out.reshape(-1)[:total].reshape(h, row)


def _video420_args(torch, what, buf, fmt, width, height, bit_depth, luma_pitch, chroma, chroma_pitch):
    """the surface of the two 4:2:0 stages -> (code, depth, w, h, row_bytes, luma pointer, luma pitch, chroma pointer, chroma
    pitch).  The defaults are the tight layout inside `buf`; chroma=: a second tensor that holds the chroma plane"""
    code, b, w, h, row, _, _ = _video_args(420, fmt, width, height, bit_depth)
    ch = (h + 1) // 2
    lp = row if luma_pitch is None else int(luma_pitch)
    cp = (lp if chroma is None else row) if chroma_pitch is None else int(chroma_pitch)
    assert buf.is_cuda and buf.is_contiguous(), what
    if lp >= row and cp >= row:                           # (a pitch below row_bytes: the library refuses it)
        nbytes = lambda t: t.numel() * t.element_size()
        if chroma is None:
            assert nbytes(buf) >= lp * h + cp * (ch - 1) + row, what
        else:
            assert chroma.is_cuda and chroma.is_contiguous() and chroma.device == buf.device, what
            assert nbytes(buf) >= lp * (h - 1) + row and nbytes(chroma) >= cp * (ch - 1) + row, what
    cptr = buf.data_ptr() + lp * h if chroma is None else chroma.data_ptr()
    return code, b, w, h, row, buf.data_ptr(), lp, cptr, cp


def unpack_video420(d_buf, fmt, width, height, bit_depth=None, dtype=None, out=None, luma_pitch=None, chroma=None, chroma_pitch=None):
    """a 4:2:0 video buffer on the device (fmt = "nv12" | "nv21" | "p0xx" | "p010" | "p012" | "p016"; uint8 tensor) -> the
    frame's planes as ONE flat tensor, Y [H,W] then Cb and Cr [ceil(H/2),ceil(W/2)], in `dtype` (uint8 -- nv12 / nv21 only -- /
    int16 / uint16 / int32; default: uint8 for nv12 / nv21, else int16), or in `out` (contiguous, at least that many elements;
    its dtype is the container).  The defaults are pipeline.pack_video420's tight layout inside d_buf; luma_pitch: the bytes
    from one luma row to the next, the chroma plane then following the last luma row at luma_pitch * H; chroma=: a second
    tensor that holds the chroma plane (a surface whose planes are separate), chroma_pitch: its rows' distance.  Pointers and
    pitches are multiples of 2 (p0xx: 4) bytes and need no other alignment.  ojphgpu_unpack_video420."""
    torch = _torch()
    code, b, w, h, row, lptr, lp, cptr, cp = _video420_args(torch, "unpack_video420", d_buf, fmt, width, height, bit_depth, luma_pitch, chroma, chroma_pitch)
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    if out is None:
        out = torch.empty(n, dtype=dtype if dtype is not None else _video_dtype(torch, fmt), device=d_buf.device)
    assert out.is_cuda and out.is_contiguous() and out.numel() >= n
    check(capi.lib().ojphgpu_unpack_video420(_stream_ptr(torch, d_buf.device.index or 0), code, C.c_void_p(lptr), lp, C.c_void_p(cptr), cp,
                                             C.c_void_p(out.data_ptr()), w, h, b, out.element_size() * 8), "unpack_video420")
    return out.reshape(-1)[:n]


def pack_video420(d_planes, fmt, width, height, bit_depth=None, out=None, luma_pitch=None, chroma=None, chroma_pitch=None):
    """the way back: the planes as one flat tensor (the frame layout above; uint8 / int16 / uint16 / int32) -> the video buffer,
    clamped to [0, 2^bit_depth - 1], every padding position zero.  Without `out`: a new uint8 [H + ch, row_bytes] in the tight
    layout.  `out` (uint8, contiguous), luma_pitch, chroma= and chroma_pitch describe the surface as for unpack_video420; only
    [0, row_bytes) of every row of the two planes is written.  Returns out (the tight layout: reshaped to [H + ch, row_bytes]).
    ojphgpu_pack_video420."""
    torch = _torch()
    from .pipeline import video420_layout
    w, h = int(width), int(height)
    assert d_planes.is_cuda and d_planes.is_contiguous() and d_planes.numel() >= w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    tight = luma_pitch is None and chroma is None and chroma_pitch is None
    if out is None:
        assert tight, "pack_video420: a pitched surface is the caller's (out=)"
        out = torch.empty(video420_layout(fmt, w, h)[2], dtype=torch.uint8, device=d_planes.device)
    code, b, w, h, row, lptr, lp, cptr, cp = _video420_args(torch, "pack_video420", out, fmt, w, h, bit_depth, luma_pitch, chroma, chroma_pitch)
    check(capi.lib().ojphgpu_pack_video420(_stream_ptr(torch, d_planes.device.index or 0), code, C.c_void_p(d_planes.data_ptr()), C.c_void_p(lptr), lp,
                                           C.c_void_p(cptr), cp, w, h, d_planes.element_size() * 8, b), "pack_video420")
    rows = h + (h + 1) // 2
    return out.reshape(-1)[:row * rows].reshape(rows, row) if tight else out


def _video444_args(what, buf, fmt, width, height, bit_depth, pitch):
    """the surface of the two 4:4:4 stages -> (code, depth, w, h, row_bytes, pitch); the default is the tight layout"""
    code, b, w, h, row, _, _ = _video_args(444, fmt, width, height, bit_depth)
    p = row if pitch is None else int(pitch)
    assert buf.is_cuda and buf.is_contiguous(), what
    if p >= row:                                          # (a pitch below row_bytes: the library refuses it)
        assert buf.numel() * buf.element_size() >= p * (h - 1) + row, what
    return code, b, w, h, row, p


def unpack_video444(d_buf, fmt, width, height, bit_depth=None, dtype=None, out=None, pitch=None):
    """a 4:4:4 packed video buffer on the device (fmt = "v410" | "y410" | "r210" | "r10k" | "y4xx" | "y412" | "y416" | "ayuv" |
    "bgra" | "rgba" | "argb"; uint8 tensor) -> the frame's three planes [H,W] as ONE flat tensor in `dtype` (uint8 -- the byte
    formats only -- / int16 / uint16 / int32; default: uint8 for the byte formats, else int16), or in `out` (contiguous, at
    least that many elements; its dtype is the container).  The default is pipeline.pack_video444's tight layout; pitch: the
    bytes from one row to the next of a surface that is used in place.  The pointer and the pitch are multiples of the
    pixel's size (4 bytes, y4xx: 8) and need no other alignment.  ojphgpu_unpack_video444."""
    torch = _torch()
    code, b, w, h, row, p = _video444_args("unpack_video444", d_buf, fmt, width, height, bit_depth, pitch)
    n = 3 * w * h
    if out is None:
        out = torch.empty(n, dtype=dtype if dtype is not None else _video_dtype(torch, fmt), device=d_buf.device)
    assert out.is_cuda and out.is_contiguous() and out.numel() >= n
    check(capi.lib().ojphgpu_unpack_video444(_stream_ptr(torch, d_buf.device.index or 0), code, C.c_void_p(d_buf.data_ptr()), p,
                                             C.c_void_p(out.data_ptr()), w, h, b, out.element_size() * 8), "unpack_video444")
    return out.reshape(-1)[:n]


def pack_video444(d_planes, fmt, width, height, bit_depth=None, out=None, pitch=None):
    """the way back: the three planes as one flat tensor (uint8 / int16 / uint16 / int32) -> the packed buffer, clamped to [0,
    2^bit_depth - 1], padding zero, alpha opaque.  Without `out`: a new uint8 [H, row_bytes] in the tight layout.  `out`
    (uint8, contiguous) and pitch describe the surface as for unpack_video444; only [0, row_bytes) of every row is written.
    Returns out (the tight layout: reshaped to [H, row_bytes]).  ojphgpu_pack_video444."""
    torch = _torch()
    from .pipeline import video444_layout
    w, h = int(width), int(height)
    assert d_planes.is_cuda and d_planes.is_contiguous() and d_planes.numel() >= 3 * w * h
    if out is None:
        assert pitch is None, "pack_video444: a pitched surface is the caller's (out=)"
        out = torch.empty(video444_layout(fmt, w, h)[1], dtype=torch.uint8, device=d_planes.device)
    code, b, w, h, row, p = _video444_args("pack_video444", out, fmt, w, h, bit_depth, pitch)
    check(capi.lib().ojphgpu_pack_video444(_stream_ptr(torch, d_planes.device.index or 0), code, C.c_void_p(d_planes.data_ptr()), C.c_void_p(out.data_ptr()), p,
                                           w, h, d_planes.element_size() * 8, b), "pack_video444")
    return out.reshape(-1)[:row * h].reshape(h, row) if pitch is None else out


def pack_pixels(planes, bit_depth, pixel_bits=None, big_endian=False, out=None):
    """planes [C,H,W] on the device -> pixel-interleaved [H,W,C] (uint8 for pixel_bits 8, else int16 holding the bytes
    of uint16 samples, byte-swapped when big_endian), clamped to [0, 2^bit_depth - 1] as the reference's writers do.
    `out`: a contiguous tensor of pixel_bits-bit elements, at least H * W * C of them, of which the first H * W * C are
    written."""
    torch = _torch()
    assert planes.is_cuda and planes.is_contiguous() and planes.dim() == 3
    c, h, w = planes.shape
    pb = int(pixel_bits) if pixel_bits else (8 if bit_depth <= 8 else 16)
    if out is None:
        out = torch.empty((h, w, c), dtype=torch.uint8 if pb == 8 else torch.int16, device=planes.device)
    assert out.is_cuda and out.is_contiguous() and out.device == planes.device and out.element_size() * 8 == pb and out.numel() >= c * h * w
    check(capi.lib().ojphgpu_pack_pixels(_stream_ptr(torch, planes.device.index or 0), C.c_void_p(planes.data_ptr()),
                                         C.c_void_p(out.data_ptr()), w, h, c, planes.element_size() * 8, pb, int(bool(big_endian)),
                                         int(bit_depth)), "pack_pixels")
    return out.reshape(-1)[:c * h * w].reshape(h, w, c)

