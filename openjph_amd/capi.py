"""ctypes binding of include/ojphgpu.h (libojphgpu.so).

This module only *binds*; it contains no codec logic and no CPU fallback.  If the shared library
is missing it raises ImportError-like RuntimeError loudly (build it with
``python -c "import __graft_entry__ as g; g.build()"``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libojphgpu.so")

OK, E_INVALID, E_NOMEM, E_HIP, E_CODESTREAM, E_OVERFLOW, E_BLOCK, E_AGAIN, E_UNCOLLECTED, E_BUDGET, E_QUALITY = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10
RATE_GRID, STATS_BINS = 241, 80
VIDEO_V410, VIDEO_Y410, VIDEO_R210, VIDEO_R10K, VIDEO_Y4XX, VIDEO_AYUV, VIDEO_BGRA, VIDEO_RGBA, VIDEO_ARGB = range(0x21, 0x2A)   # section 7d
PROG_ORDERS = {"LRCP": 0, "RLCP": 1, "RPCL": 2, "PCRL": 3, "CPRL": 4}


class Coc(C.Structure):
    """ojphgpu_coc: a COC marker segment (per-component coding style)"""
    _fields_ = [
        ("rank", C.c_uint8), ("reversible", C.c_uint8), ("num_decomps", C.c_uint8),
        ("log_block_w", C.c_uint8), ("log_block_h", C.c_uint8), ("has_precincts", C.c_uint8),
        ("reserved", C.c_uint8 * 2), ("precinct_exps", C.c_uint8 * 36),
    ]


class LiftStep(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("e", C.c_int32), ("A", C.c_float)]


class Atk(C.Structure):
    """ojphgpu_atk: an ATK marker segment (a lifting kernel)"""
    _fields_ = [("index", C.c_uint8), ("reversible", C.c_uint8), ("num_steps", C.c_uint8), ("coeff_type", C.c_uint8),
                ("K", C.c_float), ("steps", LiftStep * 16)]


class Dfs(C.Structure):
    """ojphgpu_dfs: a DFS marker segment (which directions each decomposition level transforms)"""
    _fields_ = [("used", C.c_uint8), ("index", C.c_uint8), ("num_levels", C.c_uint8), ("reserved", C.c_uint8), ("types", C.c_uint8 * 32)]


class Lift(C.Structure):
    """ojphgpu_lift: a lifting kernel as the general DWT kernels take it"""
    _fields_ = [("num_steps", C.c_uint32), ("elem", C.c_uint32), ("horz", C.c_uint32), ("vert", C.c_uint32), ("K", C.c_float),
                ("steps", LiftStep * 16)]


class Params(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("num_comps", C.c_uint32),
        ("bit_depth", C.c_uint32), ("is_signed", C.c_uint32),
        ("reversible", C.c_uint32), ("num_decomps", C.c_uint32),
        ("block_w", C.c_uint32), ("block_h", C.c_uint32),
        ("color_transform", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
        ("prog_order", C.c_uint32), ("qstep", C.c_float),
        ("precinct_w", C.c_uint32), ("precinct_h", C.c_uint32), ("tlm", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
        ("precinct_exps", C.c_uint8 * 36),
        ("image_x0", C.c_uint32), ("image_y0", C.c_uint32), ("tile_x0", C.c_uint32), ("tile_y0", C.c_uint32),
        ("comp_dx", C.c_uint8 * 16), ("comp_dy", C.c_uint8 * 16),
        ("comp_depth", C.c_uint8 * 16), ("comp_sign", C.c_uint8 * 16),
        ("coc", Coc * 16),
        ("nlt_default", C.c_uint8), ("nlt_bd_default", C.c_uint8),
        ("nlt_comp", C.c_uint8 * 16), ("nlt_rank", C.c_uint8 * 16), ("nlt_bd", C.c_uint8 * 16),
        ("nlt_reserved", C.c_uint8 * 2),
        ("qcc_qfactor", C.c_uint8 * 16), ("qcc_ctype", C.c_uint8 * 16), ("qcc_rank", C.c_uint8 * 16),
        ("wavelet", C.c_uint8), ("part2_reserved", C.c_uint8 * 3), ("atk", Atk * 4), ("dfs", Dfs * 4),
    ]


class BandInfo(C.Structure):
    _fields_ = [
        ("tile", C.c_uint32), ("comp", C.c_uint32), ("res", C.c_uint32), ("band", C.c_uint32),
        ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
        ("K_max", C.c_uint32), ("delta", C.c_float), ("delta_inv", C.c_float),
        ("nbx", C.c_uint32), ("nby", C.c_uint32), ("first_block", C.c_uint32),
        ("plane_off", C.c_uint64), ("pitch", C.c_uint32), ("reserved", C.c_uint32),
    ]


class BlockInfo(C.Structure):
    _fields_ = [("band", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32),
                ("h", C.c_uint32), ("K_max", C.c_uint32)]


class LevelInfo(C.Structure):
    _fields_ = [
        ("tile", C.c_uint32), ("comp", C.c_uint32), ("res", C.c_uint32),
        ("w", C.c_uint32), ("h", C.c_uint32), ("x_even", C.c_uint32), ("y_even", C.c_uint32),
        ("src_off", C.c_uint64), ("src_pitch", C.c_uint32),
        ("ll_off", C.c_uint64), ("ll_pitch", C.c_uint32),
        ("hl_off", C.c_uint64), ("hl_pitch", C.c_uint32),
        ("lh_off", C.c_uint64), ("lh_pitch", C.c_uint32),
        ("hh_off", C.c_uint64), ("hh_pitch", C.c_uint32), ("kind", C.c_uint32),
    ]


class CodedBlock(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("len1", C.c_uint32), ("len2", C.c_uint32),
                ("missing_msbs", C.c_uint32), ("num_passes", C.c_uint32)]


class PaddedBlock(C.Structure):            # ojphgpu_padded_block
    _fields_ = [("block", C.c_uint32), ("got", C.c_uint32), ("offset", C.c_uint64), ("len1", C.c_uint32), ("len2", C.c_uint32),
                ("missing_msbs", C.c_uint32), ("num_passes", C.c_uint32)]


class DwtDesc(C.Structure):
    _fields_ = [
        ("src_off", C.c_uint64), ("ll_off", C.c_uint64), ("hl_off", C.c_uint64),
        ("lh_off", C.c_uint64), ("hh_off", C.c_uint64),
        ("src_pitch", C.c_uint32), ("ll_pitch", C.c_uint32), ("hl_pitch", C.c_uint32),
        ("lh_pitch", C.c_uint32), ("hh_pitch", C.c_uint32),
        ("w", C.c_uint32), ("h", C.c_uint32), ("x_even", C.c_uint32), ("y_even", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class DwtRegion(C.Structure):             # ojphgpu_dwt_region
    _fields_ = [
        ("rx0", C.c_uint32), ("ry0", C.c_uint32), ("rx1", C.c_uint32), ("ry1", C.c_uint32),
        ("out_off", C.c_uint64), ("out_pitch", C.c_uint32), ("reserved", C.c_uint32),
    ]


class CbDesc(C.Structure):
    _fields_ = [
        ("coef_off", C.c_uint64), ("pitch", C.c_uint32), ("w", C.c_uint16), ("h", C.c_uint16),
        ("K_max", C.c_uint8), ("reversible", C.c_uint8), ("missing_msbs", C.c_uint8),
        ("num_passes", C.c_uint8), ("delta", C.c_float), ("len1", C.c_uint32), ("len2", C.c_uint32),
        ("data_off", C.c_uint64), ("scratch_cap", C.c_uint32), ("reserved", C.c_uint32),
    ]


class CbResult(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("length", C.c_uint32)]


class ConvertDesc(C.Structure):
    _fields_ = [("plane_off", C.c_uint64), ("pitch", C.c_uint32), ("w", C.c_uint32),
                ("h", C.c_uint32), ("src_x0", C.c_uint32), ("src_y0", C.c_uint32),
                ("img_pitch", C.c_uint32), ("img_off", C.c_uint64), ("fmt", C.c_uint32), ("reserved", C.c_uint32)]


class StatsDesc(C.Structure):             # ojphgpu_stats_desc
    _fields_ = [("plane_off", C.c_uint64), ("pitch", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("slot", C.c_uint32)]


class RateInfo(C.Structure):              # ojphgpu_rate_info
    _fields_ = [("grid_index", C.c_uint32), ("qstep", C.c_float), ("bytes", C.c_uint64), ("bytes_finer", C.c_uint64),
                ("passes", C.c_uint32), ("first_guess", C.c_uint32)]


SIZE_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_uint32)      # ojphgpu_size_fn


class TruncInfo(C.Structure):             # ojphgpu_trunc_info
    _fields_ = [("level", C.c_uint32), ("passes", C.c_uint32), ("first_guess", C.c_uint32), ("max_dropped", C.c_uint32),
                ("lossless", C.c_uint32), ("reserved", C.c_uint32), ("bytes", C.c_uint64), ("bytes_finer", C.c_uint64)]


class NearLosslessInfo(C.Structure):      # ojphgpu_near_lossless_info
    _fields_ = [("level", C.c_uint32), ("passes", C.c_uint32), ("lossless", C.c_uint32), ("max_dropped", C.c_uint32),
                ("pae", C.c_uint32), ("level_coarser", C.c_uint32), ("pae_coarser", C.c_uint32), ("reserved", C.c_uint32),
                ("sse", C.c_uint64), ("sse_coarser", C.c_uint64), ("bytes", C.c_uint64)]


ERR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32))      # ojphgpu_err_fn


class RequantDesc(C.Structure):           # ojphgpu_requant_desc
    _fields_ = [("plane_off", C.c_uint64), ("pitch", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("delta_inv", C.c_float),
                ("delta", C.c_float), ("K_max", C.c_uint32)]


class ErrorComp(C.Structure):             # ojphgpu_error_comp
    _fields_ = [("first_elem", C.c_uint64), ("count", C.c_uint64), ("is_signed", C.c_uint32), ("reserved", C.c_uint32)]


class FrameErr(C.Structure):              # ojphgpu_frame_err
    _fields_ = [("sse", C.c_uint64), ("pae", C.c_uint32), ("reserved", C.c_uint32)]


class FitComp(C.Structure):               # ojphgpu_fit_comp
    _fields_ = [("first_elem", C.c_uint64), ("count", C.c_uint64), ("shift", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32),
                ("reserved", C.c_uint32)]


class ResampleComp(C.Structure):          # ojphgpu_resample_comp
    _fields_ = [("src_first", C.c_uint64), ("dst_first", C.c_uint64), ("src_w", C.c_uint32), ("src_h", C.c_uint32), ("dst_w", C.c_uint32),
                ("dst_h", C.c_uint32), ("fx", C.c_uint32), ("fy", C.c_uint32), ("px", C.c_uint32), ("py", C.c_uint32), ("shift", C.c_int32),
                ("lo", C.c_int32), ("hi", C.c_int32), ("reserved", C.c_uint32)]


class ColourTable(C.Structure):           # ojphgpu_colour_table
    _fields_ = [("m", (C.c_int32 * 3) * 3), ("off", C.c_int64 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("k", C.c_uint32)]


class ColourFrame(C.Structure):           # ojphgpu_colour_frame
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("fx", C.c_uint32), ("fy", C.c_uint32), ("rgb_first", C.c_uint64 * 3),
                ("ycc_first", C.c_uint64 * 3)]


class ChromaFrame(C.Structure):           # ojphgpu_chroma_frame
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("sfx", C.c_uint32), ("sfy", C.c_uint32), ("dfx", C.c_uint32), ("dfy", C.c_uint32),
                ("src_off", C.c_uint64 * 3), ("dst_off", C.c_uint64 * 3)]


class ColourSpec(C.Structure):            # ojphgpu_colour_spec
    _fields_ = [("standard", C.c_int), ("rgb_range", C.c_int), ("ycc_range", C.c_int), ("rgb_depth", C.c_uint32)]


COLOUR_STANDARD = {"bt601": 601, "bt709": 709, "bt2020": 2020}
COLOUR_DIRECTION = {"forward": 0, "inverse": 1}
COLOUR_RANGE = {"full": 0, "narrow": 1}
CHROMA_COSITED = 1
CHROMA = {"cosited": CHROMA_COSITED}
RESAMPLE_NONE, RESAMPLE_COSITED = 0, 1
RESAMPLE = {None: RESAMPLE_NONE, "none": RESAMPLE_NONE, "cosited": RESAMPLE_COSITED}


class QualityInfo(C.Structure):           # ojphgpu_quality_info
    _fields_ = [("grid_index", C.c_uint32), ("qstep", C.c_float), ("sse", C.c_uint64), ("sse_coarser", C.c_uint64),
                ("pae", C.c_uint32), ("passes", C.c_uint32), ("bytes", C.c_uint64)]


SSE_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64))      # ojphgpu_sse_fn


class CappedInfo(C.Structure):            # ojphgpu_capped_info
    _fields_ = [("grid_index", C.c_uint32), ("qstep", C.c_float), ("outcome", C.c_uint32), ("quality_index", C.c_uint32),
                ("quality_bytes", C.c_uint64), ("bytes", C.c_uint64), ("bytes_finer", C.c_uint64), ("sse", C.c_uint64),
                ("sse_coarser", C.c_uint64), ("pae", C.c_uint32), ("quality_passes", C.c_uint32), ("rate_passes", C.c_uint32),
                ("first_guess_q", C.c_uint32), ("first_guess_b", C.c_uint32), ("reserved", C.c_uint32)]


HIST_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p)                                       # ojphgpu_hist_fn
CAPPED_MET, CAPPED_BY_BUDGET = 0, 1


class Run(C.Structure):                   # ojphgpu_run
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("n", C.c_uint64)]


class T2Job(C.Structure):                 # ojphgpu_t2_job
    _fields_ = [("dst", C.c_uint64), ("src", C.c_uint64), ("n", C.c_uint32), ("blob", C.c_uint32)]


class VideoInfo(C.Structure):            # ojphgpu_video_info
    _fields_ = [("family", C.c_int), ("sub_x", C.c_uint32), ("sub_y", C.c_uint32), ("min_depth", C.c_uint32), ("max_depth", C.c_uint32),
                ("min_container_bits", C.c_uint32), ("pointer_align", C.c_uint32), ("pitch_align", C.c_uint32)]


_lib = None

# name -> (restype, argtypes); also the list every test checks against include/ojphgpu.h
SIGNATURES = {
    "ojphgpu_plan_create": (C.c_int, [C.POINTER(Params), C.POINTER(C.c_void_p)]),
    "ojphgpu_plan_destroy": (None, [C.c_void_p]),
    "ojphgpu_plan_params": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "ojphgpu_plan_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ojphgpu_plan_comp_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_plan_tile_parts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_dwt_forward_image16": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p]),
    "ojphgpu_dwt_inverse_image16": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p]),
    "ojphgpu_convert_forward16": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p]),
    "ojphgpu_convert_inverse16": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p]),
    "ojphgpu_encoder_run_device16": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_encoder_run_device8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_decoder_run_device8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_dwt_forward_image_ex": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "ojphgpu_dwt_inverse_image_ex": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "ojphgpu_convert_forward_ex": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_int]),
    "ojphgpu_convert_inverse_ex": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_int]),
    "ojphgpu_encode16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_decoder_run_device16": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_decode16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ojphgpu_ht_decode_layout": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ojphgpu_plan_comp_format": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ojphgpu_plan_comp_style": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_plan_comp_lift": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ojphgpu_plan_set_comments": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_uint16), C.POINTER(C.c_uint16),
                                            C.c_uint32]),
    "ojphgpu_plan_restrict_resolution": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "ojphgpu_plan_restrict_region": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ojphgpu_plan_region_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_decoder_region_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ojphgpu_dwt_inverse_region": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]),
    "ojphgpu_dwt_inverse_region_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_int]),
    "ojphgpu_plan_bands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_plan_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_plan_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_plan_comp_plane": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ojphgpu_plan_coded_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_t2_parse_restricted": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ojphgpu_plan_padded_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ojphgpu_t2_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]),
    "ojphgpu_t2_write_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "ojphgpu_t2_write_main_header": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_t2_parse": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "ojphgpu_dwt_forward_general": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ojphgpu_dwt_inverse_general": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ojphgpu_dwt_forward_general_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]),
    "ojphgpu_dwt_inverse_general_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]),
    "ojphgpu_dwt_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_void_p]),
    "ojphgpu_dwt_inverse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_void_p]),
    "ojphgpu_dwt_forward_image": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_dwt_inverse_image": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_ht_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ojphgpu_ht_encode_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_uint32, C.c_uint32]),
    "ojphgpu_ht_encode_kinds": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    "ojphgpu_ht_encode_launches": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_ht_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "ojphgpu_ht_decode_aux_words": (C.c_uint32, [C.c_uint32]),
    "ojphgpu_ht_decode_prep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_ht_decode_step1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "ojphgpu_ht_decode_step2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "ojphgpu_ht_decode_kinds": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    "ojphgpu_ht_decode_step2_kinds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int]),
    "ojphgpu_ht_decode_launches": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "ojphgpu_ht_decode_fused_shape": (C.c_int,[C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_ht_decode_fused_slices": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_ht_decode_fused_state_words": (C.c_uint64, [C.c_uint32]),
    "ojphgpu_ht_decode_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]),
    "ojphgpu_ht_decode_refine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ojphgpu_decoder_ht_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_convert_forward": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32,
                                          C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_convert_inverse": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32,
                                          C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_encoder_create": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_encoder_create_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_void_p)]),
    "ojphgpu_encoder_finish_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "ojphgpu_encoder_finish_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "ojphgpu_decoder_create_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_void_p)]),
    "ojphgpu_encoder_create_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ojphgpu_encoder_finish_frame": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_decoder_create_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_decoder_upload_frame": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "ojphgpu_encoder_destroy": (None, [C.c_void_p]),
    "ojphgpu_encoder_run_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_encoder_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_encoder_coded_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ojphgpu_decoder_create": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_decoder_destroy": (None, [C.c_void_p]),
    "ojphgpu_decoder_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_decoder_run_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_decoder_failed_blocks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_decoder_fused_retries": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_decoder_giveup_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ojphgpu_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ojphgpu_encoder_ht_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ojphgpu_encoder_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "ojphgpu_encoder_is_pending": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "ojphgpu_decoder_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "ojphgpu_decoder_pending": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "ojphgpu_encoder_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_decoder_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_encoder_level_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_decoder_level_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_enc_pipe_create": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ojphgpu_enc_pipe_destroy": (None, [C.c_void_p]),
    "ojphgpu_enc_pipe_acquire": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "ojphgpu_enc_pipe_submit": (C.c_int, [C.c_void_p]),
    "ojphgpu_enc_pipe_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "ojphgpu_enc_pipe_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ojphgpu_dec_pipe_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                          C.POINTER(C.c_void_p)]),
    "ojphgpu_dec_pipe_destroy": (None, [C.c_void_p]),
    "ojphgpu_dec_pipe_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_dec_pipe_acquire": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "ojphgpu_dec_pipe_submit": (C.c_int, [C.c_void_p]),
    "ojphgpu_dec_pipe_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "ojphgpu_dec_pipe_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ojphgpu_dec_pipe_fused_retries": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_multi_encoder_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_void_p)]),
    "ojphgpu_multi_encoder_destroy": (None, [C.c_void_p]),
    "ojphgpu_multi_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_multi_encode_container": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ojphgpu_multi_encoder_workers": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]),
    "ojphgpu_multi_decoder_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_uint32,
                                              C.POINTER(C.c_void_p)]),
    "ojphgpu_multi_decoder_destroy": (None, [C.c_void_p]),
    "ojphgpu_multi_decoder_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_multi_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "ojphgpu_host_unregister": (C.c_int, [C.c_void_p]),
    "ojphgpu_multi_decode_container": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]),
    "ojphgpu_enc_pipe_set_pixels": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ojphgpu_enc_pipe_set_packed": (C.c_int, [C.c_void_p, C.c_int]),
    "ojphgpu_enc_pipe_set_budget": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_enc_pipe_rate_info": (C.c_int, [C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_dec_pipe_set_packed": (C.c_int, [C.c_void_p, C.c_int]),
    "ojphgpu_unpack_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int]),
    "ojphgpu_pack_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int]),
    "ojphgpu_dec_pipe_set_pixels": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ojphgpu_unpack_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int]),
    "ojphgpu_pack_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32]),
    "ojphgpu_band_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_band_stats_int": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_plan_trunc_levels": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_plan_trunc_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ojphgpu_plan_trunc_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "ojphgpu_trunc_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, SIZE_FN, C.c_void_p, C.POINTER(TruncInfo)]),
    "ojphgpu_encoder_set_truncation": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_encoder_set_trunc_level": (C.c_int, [C.c_void_p, C.c_int32]),
    "ojphgpu_encoder_trunc_info": (C.c_int, [C.c_void_p, C.POINTER(TruncInfo)]),
    "ojphgpu_encoder_trunc_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_near_lossless_search": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, ERR_FN, C.c_void_p, C.POINTER(NearLosslessInfo)]),
    "ojphgpu_rate_grid_qstep": (C.c_int, [C.c_uint32, C.POINTER(C.c_float)]),
    "ojphgpu_rate_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, SIZE_FN, C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_rate_search_hint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, SIZE_FN, C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_rate_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "ojphgpu_encoder_set_budget": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_encoder_rate_info": (C.c_int, [C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_encoder_rate_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_encoder_set_budgets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]),
    "ojphgpu_encoder_rate_info_frame": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RateInfo)]),
    "ojphgpu_encoder_rate_rounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_rate_stepper_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_void_p)]),
    "ojphgpu_rate_stepper_next": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_rate_stepper_feed": (C.c_int, [C.c_void_p, C.c_int64]),
    "ojphgpu_rate_stepper_info": (C.c_int, [C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_rate_stepper_destroy": (None, [C.c_void_p]),
    "ojphgpu_rate_rounds_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    "ojphgpu_rate_rounds_next": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "ojphgpu_rate_rounds_feed": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ojphgpu_rate_rounds_frame": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RateInfo)]),
    "ojphgpu_rate_rounds_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_rate_rounds_destroy": (None, [C.c_void_p]),
    "ojphgpu_band_requantise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ojphgpu_frame_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ojphgpu_frame_error_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ojphgpu_quality_search": (C.c_int, [C.c_uint64, SSE_FN, C.c_void_p, C.POINTER(QualityInfo)]),
    "ojphgpu_quality_search_hint": (C.c_int, [C.c_uint64, C.c_int32, SSE_FN, C.c_void_p, C.POINTER(QualityInfo), C.POINTER(C.c_uint32)]),
    "ojphgpu_enc_pipe_set_quality": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_enc_pipe_quality_info": (C.c_int, [C.c_void_p, C.POINTER(QualityInfo), C.POINTER(C.c_uint32)]),
    "ojphgpu_enc_pipe_quality_comp": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "ojphgpu_encoder_set_quality": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_encoder_clear_quality": (C.c_int, [C.c_void_p]),
    "ojphgpu_encoder_quality_info": (C.c_int, [C.c_void_p, C.POINTER(QualityInfo)]),
    "ojphgpu_encoder_quality_comp": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "ojphgpu_encoder_quality_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_rate_stepper_create_under": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "ojphgpu_capped_search": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, SSE_FN, SIZE_FN, HIST_FN, C.c_void_p,
                                        C.POINTER(CappedInfo)]),
    "ojphgpu_enc_pipe_set_quality_capped": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "ojphgpu_enc_pipe_capped_info": (C.c_int, [C.c_void_p, C.POINTER(CappedInfo)]),
    "ojphgpu_encoder_set_quality_capped": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "ojphgpu_encoder_capped_info": (C.c_int, [C.c_void_p, C.POINTER(CappedInfo)]),
    "ojphgpu_plan_create_transcode": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(C.c_void_p)]),
    "ojphgpu_transcoder_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_transcoder_set_budget": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_transcoder_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "ojphgpu_transcoder_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "ojphgpu_transcoder_rate_info": (C.c_int, [C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_transcoder_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_transcoder_destroy": (None, [C.c_void_p]),
    "ojphgpu_plan_upload_runs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "ojphgpu_gather_runs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ojphgpu_assemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ojphgpu_copy_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "ojphgpu_dec_pipe_create_view": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_int, C.c_uint32,
                                               C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ojphgpu_dec_pipe_view_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ojphgpu_video_layout": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ojphgpu_unpack_video": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    "ojphgpu_pack_video": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]),
    "ojphgpu_video420_layout": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ojphgpu_unpack_video420": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.c_uint32, C.c_int]),
    "ojphgpu_pack_video420": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_int, C.c_uint32]),
    "ojphgpu_video444_layout": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ojphgpu_unpack_video444": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    "ojphgpu_pack_video444": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]),
    "ojphgpu_video_format_info": (C.c_int, [C.c_int, C.POINTER(VideoInfo)]),
    "ojphgpu_colour_table_make": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(ColourTable)]),
    "ojphgpu_frame_rgb_to_ycc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(ColourFrame), C.POINTER(ColourTable)]),
    "ojphgpu_frame_ycc_to_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(ColourFrame), C.POINTER(ColourTable)]),
    "ojphgpu_video_colour_fit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ColourSpec), C.POINTER(ColourTable), C.POINTER(ColourFrame),
                                           C.POINTER(C.c_uint64)]),
    "ojphgpu_enc_pipe_set_video_colour": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ColourSpec)]),
    "ojphgpu_dec_pipe_set_video_colour": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ColourSpec)]),
    "ojphgpu_frame_rechroma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ChromaFrame)]),
    "ojphgpu_video_chroma_fit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ChromaFrame), C.POINTER(C.c_uint64)]),
    "ojphgpu_enc_pipe_set_video_chroma": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ojphgpu_dec_pipe_set_video_chroma": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ojphgpu_enc_pipe_set_video": (C.c_int, [C.c_void_p, C.c_int]),
    "ojphgpu_dec_pipe_set_video": (C.c_int, [C.c_void_p, C.c_int]),
    "ojphgpu_tc_pipe_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ojphgpu_tc_pipe_destroy": (None, [C.c_void_p]),
    "ojphgpu_tc_pipe_acquire": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "ojphgpu_tc_pipe_submit": (C.c_int, [C.c_void_p]),
    "ojphgpu_tc_pipe_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "ojphgpu_tc_pipe_set_budget": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ojphgpu_tc_pipe_rate_info": (C.c_int, [C.c_void_p, C.POINTER(RateInfo)]),
    "ojphgpu_tc_pipe_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ojphgpu_tc_pipe_fused_retries": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ojphgpu_frame_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]),
    "ojphgpu_recoder_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_frame_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]),
    "ojphgpu_recoder_create_resampled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_recoder_resample_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ojphgpu_recoder_encoder": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ojphgpu_recoder_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "ojphgpu_recoder_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "ojphgpu_recoder_frame": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "ojphgpu_recoder_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ojphgpu_recoder_destroy": (None, [C.c_void_p]),
    "ojphgpu_version": (C.c_char_p, []),
}


def lib():
    """Loads libojphgpu.so; fails loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "openjph_amd: %s is missing -- the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU "
                "fallback." % LIB_PATH)
        # PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  Import it first so
        # that libojphgpu.so binds to the SAME HIP runtime instance torch uses -- streams and
        # device pointers are exchanged between the two.  (Pure C/C++ users simply get /opt/rocm's.)
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is plumbing only
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class OjphError(RuntimeError):
    """Mirrors the reference's OJPH_ERROR -> std::runtime_error("ojph error")."""

    def __init__(self, code, what=""):
        names = {E_INVALID: "invalid argument / unsupported parameters", E_NOMEM: "out of memory",
                 E_HIP: "HIP runtime error (no GPU?)", E_CODESTREAM: "malformed codestream",
                 E_OVERFLOW: "output buffer too small", E_BLOCK: "error decoding a codeblock",
                 E_AGAIN: "no free pipeline slot",
                 E_UNCOLLECTED: "the previous run of this decoder asked for a repeat and was never collected",
                 E_BUDGET: "the byte budget is below the codestream of the coarsest quantisation step / the last truncation level",
                 E_QUALITY: "the quality target is beyond the finest quantisation step"}
        super().__init__("ojph error: %s (%d) %s" % (names.get(code, "?"), code, what))
        self.code = code


def check(rc, what=""):
    if rc != OK:
        raise OjphError(rc, what)
