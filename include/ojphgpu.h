/* include/ojphgpu.h -- C ABI of the MI355X-native HTJ2K hot path (libojphgpu.so).
 *
 * This is the drop-in boundary for the hot path of aous72/OpenJPH 0.31.0: 5/3 + 9/7 DWT,
 * quantise transfer and the HT block coder.  In the reference that path sits behind three
 * per-line / per-block function-pointer tables
 *     struct codeblock_fun            src/core/codestream/ojph_codeblock_fun.h:93-119
 *     rev_/irv_ vert_step, horz_ana.. src/core/transform/ojph_transform.h:61-96
 *     colour / convert pointers       src/core/transform/ojph_colour.h:53-103
 * which are called once per image line or per code-block from resolution::push_line/pull_line
 * (ojph_resolution.cpp:547,713), codeblock::push/encode/decode/pull_line (ojph_codeblock.cpp:
 * 115-266) and tile::push/pull (ojph_tile.cpp:332-518).  A device round trip per line is not
 * workable, so the same data contracts are exposed here *batched*: one call transforms every
 * plane / codes every code-block of a frame, driven by descriptor tables that the host side
 * (the plan) derives with the reference's geometry rules.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * OJPHGPU_E_* code and never throws.  Pointers named d_* are device (HBM) pointers, h_* are
 * host pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 * device entry points are asynchronous on `stream`.
 */
#ifndef OJPHGPU_H
#define OJPHGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OJPHGPU_OK              0
#define OJPHGPU_E_INVALID      -1   /* bad argument / unsupported parameter combination      */
#define OJPHGPU_E_NOMEM        -2
#define OJPHGPU_E_HIP          -3   /* a HIP runtime call failed (no device, launch failure)  */
#define OJPHGPU_E_CODESTREAM   -4   /* malformed codestream (== the reference's OJPH_ERROR)   */
#define OJPHGPU_E_OVERFLOW     -5   /* output buffer too small; *out_len holds the need       */
#define OJPHGPU_E_BLOCK        -6   /* a code-block failed to decode (non-resilient mode)     */
#define OJPHGPU_E_AGAIN        -7   /* a frame pipeline has no free slot: collect a result first */
#define OJPHGPU_E_UNCOLLECTED  -8   /* ojphgpu_decoder_run_device*: the run BEFORE this one asked to be decoded again (see
                                     * ojphgpu_decoder_failed_blocks) and was never collected -- its frame was incomplete */
#define OJPHGPU_E_BUDGET       -9   /* a byte budget that not even the coarsest step of the rate grid meets (section 5b) */
#define OJPHGPU_E_QUALITY      -10  /* a quality target that not even the finest step of the rate grid meets (section 5c) */

/* ------------------------------------------------------------------------------------------ *
 * 1. Codestream parameters: what ojph::param_siz / param_cod / param_qcd setters carry
 *    (src/core/openjph/ojph_params.h:68-240).
 * ------------------------------------------------------------------------------------------ */
#define OJPHGPU_MAX_SUBSAMPLED_COMPS 16
#define OJPHGPU_MAX_COC_COMPS 16
/* Part 2 (ITU-T T.801) wavelets, as far as the reference reads them (it never writes them): an ATK marker segment = a
 * lifting kernel (param_atk, ojph_params_local.h:1105-1230, read :2770-2866: whole-sample symmetric kernels with one
 * coefficient per step, even-indexed first), a DFS marker segment = which directions every decomposition level
 * transforms (param_dfs, :1030-1100, read ojph_params.cpp:2596-2644).  A lifting step, in synthesis order:
 * reversible x -+= (b + a (l + r)) >> e, irreversible x -+= A (l + r). */
#define OJPHGPU_MAX_LIFT_STEPS 16
#define OJPHGPU_MAX_ATK 4
#define OJPHGPU_MAX_DFS 4
typedef struct ojphgpu_lift_step { int32_t a, b, e; float A; } ojphgpu_lift_step;
typedef struct ojphgpu_atk {
  uint8_t  index;                  /* Satk & 0xFF: 2..255 (0 and 1 name the Part-1 wavelets); 0 = entry unused       */
  uint8_t  reversible, num_steps;
  uint8_t  coeff_type;             /* how the coefficients are written: 0 8-bit, 1 16-bit integers, 2 float, 3 double */
  float    K;                      /* irreversible: the scaling factor                                                */
  ojphgpu_lift_step steps[OJPHGPU_MAX_LIFT_STEPS];
} ojphgpu_atk;
typedef struct ojphgpu_dfs {
  uint8_t  used, index;            /* Sdfs: 0..15                                                                     */
  uint8_t  num_levels, reserved;   /* Ids; levels beyond it repeat the last one (param_dfs::get_dwt_type :2539-2547)  */
  uint8_t  types[32];              /* per decomposition level, 1 = the first one applied to the image:
                                      0 none, 1 both directions, 2 horizontal only, 3 vertical only                   */
} ojphgpu_dfs;
/* A COC marker segment: what param_cod's comp_idx setters build (ojph_params.h:146-151,
 * ojph_params.cpp:255-282).  The reference starts a new COC from the SPcod defaults -- 5
 * decompositions, 64x64 blocks, wavelet_trans 0 (the 9/7), no precincts (ojph_params_local.h:344-353)
 * -- not from the COD; the facade does the same. */
typedef struct ojphgpu_coc {
  uint8_t  rank;                   /* 0: the component follows the COD.  k >= 1: it has a COC, the k-th one
                                      created (COCs are written in creation order, ojph_params.cpp:1081-1094) */
  uint8_t  reversible;             /* param_cod::set_reversible(comp_idx, ..)                       */
  uint8_t  num_decomps;            /* param_cod::set_num_decomposition(comp_idx, ..)                */
  uint8_t  log_block_w, log_block_h; /* param_cod::set_block_dims(comp_idx, ..), log2 (2..10)        */
  uint8_t  has_precincts;          /* param_cod::set_precinct_size(comp_idx, ..): precinct_exps[0..num_decomps] */
  uint8_t  reserved[2];            /* are PPx | PPy << 4 per resolution; 0 = 32768 x 32768 everywhere.
                                      reserved[0]: bit 0 vertically causal (parser); bit 7: the decomposition is defined
                                      by the DFS marker segment with the index in bits 1..4 -- the number of
                                      decompositions is then the COD's (ojph_params_local.h:503-516, :613-618);
                                      reserved[1]: the wavelet is the ATK marker segment with this index (2..255), 0 =
                                      `reversible` names the Part-1 wavelet */
  uint8_t  precinct_exps[36];
} ojphgpu_coc;
typedef struct ojphgpu_params {
  uint32_t width, height;        /* param_siz::set_image_extent                               */
  uint32_t num_comps;            /* param_siz::set_num_components  (all comps share the below) */
  uint32_t bit_depth;            /* param_siz::set_component(.., bit_depth, ..)               */
  uint32_t is_signed;
  uint32_t reversible;           /* param_cod::set_reversible                                 */
  uint32_t num_decomps;          /* param_cod::set_num_decomposition                          */
  uint32_t block_w, block_h;     /* param_cod::set_block_dims                                 */
  uint32_t color_transform;      /* param_cod::set_color_transform                            */
  uint32_t tile_w, tile_h;       /* param_siz::set_tile_size; 0 = one tile                    */
  uint32_t prog_order;           /* 0 LRCP 1 RLCP 2 RPCL 3 PCRL 4 CPRL (set_progression_order) */
  float    qstep;                /* param_qcd::set_irrev_quant; <= 0 selects 2^-min(16,B)     */
  uint32_t precinct_w, precinct_h; /* 0 = 32768 (no explicit precincts)                        */
  uint32_t tlm;                  /* codestream::request_tlm_marker                            */
  uint32_t reserved[4];          /* [0] bit 0: vertically causal code-block style (set by the parser)
                                    [1] codestream::set_tilepart_divisions: bit 0 = a tile-part per
                                        resolution, bit 1 = per component (what the progression
                                        order cannot honour is dropped as write_headers drops it)
                                    [2] param_qcd::set_qfactor: 1..100, 0 = not set            */
  uint8_t  precinct_exps[36];    /* param_cod::set_precinct_size with a list: per resolution (0 =
                                    lowest) PPx | PPy << 4; all zero = precinct_w/h everywhere  */
  /* reference grid (ojph_params.h:68-112).  width/height stay the image SIZE: the extent the
     reference's set_image_extent takes is image_x0 + width, image_y0 + height.                 */
  uint32_t image_x0, image_y0;   /* param_siz::set_image_offset                                 */
  uint32_t tile_x0, tile_y0;     /* param_siz::set_tile_offset (<= image offset)                */
  uint8_t  comp_dx[OJPHGPU_MAX_SUBSAMPLED_COMPS];   /* param_siz::set_component downsampling of   */
  uint8_t  comp_dy[OJPHGPU_MAX_SUBSAMPLED_COMPS];   /* component c < 16; 0 = 1; later ones are 1  */
  uint8_t  comp_depth[OJPHGPU_MAX_SUBSAMPLED_COMPS]; /* set_component bit depth of component c < 16 */
                                                     /* when it differs from bit_depth; 0 = same   */
  uint8_t  comp_sign[OJPHGPU_MAX_SUBSAMPLED_COMPS];  /* 0 = is_signed, 1 = unsigned, 2 = signed    */
  ojphgpu_coc coc[OJPHGPU_MAX_COC_COMPS];            /* per-component coding style of component c < 16 */
  /* NLT marker segments: param_nlt::set_nonlinear_transform (ojph_params.h:299-345).  Values: 0 = not
     set, 1 = type 0 (no non-linearity) set, 4 = type 3 (binary complement <-> sign magnitude, the only
     other type the reference supports) set.  nlt_default = the ALL_COMPS entry; nlt_comp[c] / nlt_rank[c]
     = component c < 16 and the order its entry was created in (1..); nlt_bd_* = BDnlt as read by the
     parser (0 when the plan was not parsed). */
  uint8_t  nlt_default, nlt_bd_default;
  uint8_t  nlt_comp[OJPHGPU_MAX_COC_COMPS], nlt_rank[OJPHGPU_MAX_COC_COMPS], nlt_bd[OJPHGPU_MAX_COC_COMPS];
  uint8_t  nlt_reserved[2];
  /* param_qcd::set_qfactor(comp_idx, ctype, qfactor) (ojph_params.h:251-254): a QCC for component
     c < 16 with its own quality factor (1..100; 0 = not set), the visual weights of ctype (0 Y, 1 Cb,
     2 Cr) and its place in the creation order (QCCs are written in that order, then the ones the
     library adds, ojph_params.cpp:1822-1834) */
  uint8_t  qcc_qfactor[OJPHGPU_MAX_COC_COMPS], qcc_ctype[OJPHGPU_MAX_COC_COMPS], qcc_rank[OJPHGPU_MAX_COC_COMPS];
  /* Part 2: the COD's wavelet when it is an ATK marker segment (its index, 2..255; 0 = `reversible` decides), and the
     ATK / DFS marker segments of the main header (see ojphgpu_atk / ojphgpu_dfs) */
  uint8_t  wavelet, part2_reserved[3];
  ojphgpu_atk atk[OJPHGPU_MAX_ATK];
  ojphgpu_dfs dfs[OJPHGPU_MAX_DFS];
} ojphgpu_params;

/* ------------------------------------------------------------------------------------------ *
 * 2. The plan: host-side geometry (tile -> tile-comp -> resolution -> subband -> code-block,
 *    precincts, K_max / delta per sub-band) derived with the reference's rules
 *    (ojph_tile.cpp:191-329, ojph_resolution.cpp:240-470, ojph_subband.cpp:117-276,
 *    ojph_params.cpp:1495-1760).  Host only; needs no GPU.
 * ------------------------------------------------------------------------------------------ */
typedef struct ojphgpu_plan ojphgpu_plan;

typedef struct ojphgpu_band_info {   /* one sub-band of one tile-component resolution */
  uint32_t tile, comp, res, band;    /* band: 0 LL 1 HL 2 LH 3 HH */
  uint32_t x0, y0, w, h;             /* band rectangle in band coordinates */
  uint32_t K_max;
  float    delta, delta_inv;         /* irreversible: step / 2^(31-K_max) and its inverse */
  uint32_t nbx, nby, first_block;    /* code-block grid and index of its first block */
  uint64_t plane_off;                /* element (4 B) offset of the band plane in the coefficient arena */
  uint32_t pitch;                    /* elements */
  uint32_t reserved;
} ojphgpu_band_info;

typedef struct ojphgpu_block_info {  /* one code-block */
  uint32_t band;                     /* index into the band table */
  uint32_t x0, y0, w, h;             /* rectangle relative to the band origin */
  uint32_t K_max;
} ojphgpu_block_info;

typedef struct ojphgpu_level_info {  /* one DWT level of one tile-component: res -> res-1 + 3 bands */
  uint32_t tile, comp, res;          /* res = resolution being analysed (>= 1) */
  uint32_t w, h, x_even, y_even;     /* input plane geometry */
  uint64_t src_off; uint32_t src_pitch;
  uint64_t ll_off;  uint32_t ll_pitch;
  uint64_t hl_off;  uint32_t hl_pitch;
  uint64_t lh_off;  uint32_t lh_pitch;
  uint64_t hh_off;  uint32_t hh_pitch;
  uint32_t kind;                     /* 1 both directions (always, without a DFS marker segment), 2 horizontal only (ll +
                                        hl), 3 vertical only (ll + lh), 0 no transform (ll = the plane) */
} ojphgpu_level_info;

typedef struct ojphgpu_coded_block { /* what the packet headers say about one code-block */
  uint64_t offset;                   /* byte offset of the block's data (encode: in the block-data
                                        buffer; decode: in the codestream) */
  uint32_t len1, len2;               /* pass_length[0], pass_length[1] (0,0 = not included) */
  uint32_t missing_msbs, num_passes;
} ojphgpu_coded_block;

int  ojphgpu_plan_create(const ojphgpu_params* params, ojphgpu_plan** out);
void ojphgpu_plan_destroy(ojphgpu_plan* plan);
int  ojphgpu_plan_params(const ojphgpu_plan* plan, ojphgpu_params* out);
/* counts: out[0]=tiles [1]=bands [2]=blocks [3]=dwt levels [4]=coefficient arena elements
 *         [5]=max coded bytes of one block [6]=precincts [7]=tile-comps */
int  ojphgpu_plan_counts(const ojphgpu_plan* plan, uint64_t out[8]);
/* user COM marker segments written after the library's own one (the `comments` argument of
 * codestream::write_headers, ojph_codestream_local.cpp:686-703): n segments, segment i = len[i] bytes
 * at data[i] with registration value rcom[i] (1 = Latin text, 0 = binary).  Replaces earlier ones. */
int  ojphgpu_plan_set_comments(ojphgpu_plan* plan, const uint8_t* const* data, const uint16_t* len,
                               const uint16_t* rcom, uint32_t n);
/* tile-parts every tile is written in (1 without tile-part divisions) */
int  ojphgpu_plan_tile_parts(const ojphgpu_plan* plan, uint32_t* parts_per_tile);
int  ojphgpu_plan_bands(const ojphgpu_plan* plan, ojphgpu_band_info* out, size_t n);
int  ojphgpu_plan_blocks(const ojphgpu_plan* plan, ojphgpu_block_info* out, size_t n);
int  ojphgpu_plan_levels(const ojphgpu_plan* plan, ojphgpu_level_info* out, size_t n);
/* element offset + pitch of tile-component (tile, comp)'s full-resolution plane in the arena;
 * rect = x0, y0, w, h of the tile-component on the component's own (sub-sampled) grid */
int  ojphgpu_plan_comp_plane(const ojphgpu_plan* plan, uint32_t tile, uint32_t comp,
                             uint64_t* off, uint32_t* pitch, uint32_t rect[4]);
/* The image buffer every codec call takes ("frame"): the int32 planes of the components one after
 * the other, component c being out[2] x out[3] samples (param_siz::get_recon_width / _height),
 * tightly packed, starting out[4] | out[5] << 32 elements into the frame.  out[0], out[1] = the
 * component's origin on its own grid (ceil(image offset / sub-sampling)); out[6], out[7] = its
 * sub-sampling factors.  comp == num_comps: out[4] | out[5] << 32 = elements of one whole frame. */
int  ojphgpu_plan_comp_info(const ojphgpu_plan* plan, uint32_t comp, uint32_t out[8]);
/* bit depth and signedness of a component (param_siz::get_bit_depth / is_signed) */
int  ojphgpu_plan_comp_format(const ojphgpu_plan* plan, uint32_t comp, uint32_t* bit_depth, uint32_t* is_signed);
/* coding style of a component, from its COC or the COD (param_cod's comp_idx getters,
 * ojph_params.cpp:374-399): out[0] decompositions, [1] reversible, [2] [3] log2 code-block width /
 * height, [4] 1 = the component has a COC, [5] decompositions left after restrict_resolution,
 * [6] 1 = the type 3 non-linearity applies to the component (NLT marker segment, signed component) */
int  ojphgpu_plan_comp_style(const ojphgpu_plan* plan, uint32_t comp, uint32_t out[8]);
/* the wavelet of decomposition level `level` (1 = the first one applied to the tile-component) of a component, as the
 * general lifting kernels take it: the steps of its ATK marker segment (or of the Part-1 wavelet its COD / COC names),
 * the directions its DFS marker segment has the level transform, elem by the component's sample path
 * (cod.access_atk() + param_dfs::get_dwt_type as resolution::finalize_alloc combines them, ojph_resolution.cpp:264-300) */
struct ojphgpu_lift;
int  ojphgpu_plan_comp_lift(const ojphgpu_plan* plan, uint32_t comp, uint32_t level, struct ojphgpu_lift* out);

/* ------------------------------------------------------------------------------------------ *
 * 3. Tier-2 on the host: marker segments + packet headers (tag trees, pass lengths) around the
 *    code-block bytes.  Replaces local::codestream::write_headers/flush
 *    (ojph_codestream_local.cpp:556-712,1148), tile::flush (ojph_tile.cpp:584-774),
 *    precinct::prepare_precinct/write/parse (ojph_precinct.cpp:94-573) and
 *    read_headers/read (ojph_codestream_local.cpp:769-1146).
 * ------------------------------------------------------------------------------------------ */
/* blocks[i] describes code-block i of the plan (plan order); len1 == 0 -> block not coded.
 * Writes a complete codestream (SOC .. EOC). */
int  ojphgpu_t2_write(const ojphgpu_plan* plan, const uint8_t* h_block_data,
                      const ojphgpu_coded_block* blocks, uint8_t* h_out, size_t cap,
                      size_t* out_len);
/* The same in pieces, for tile-sharded encoding (tiles are independent: own DWT, blocks, packets
 * and tile-parts, ojph_tile.cpp:584-774): the tile-parts (SOT .. last packet) of tiles
 * [tile_first, tile_first + tile_count) -- tile_part_len[i * parts_per_tile + k] receives Psot of
 * tile-part k of tile tile_first + i --
 * and the main header (SOC .. last main-header marker; needs every tile's Psot only when a TLM
 * marker was requested).  codestream = main header | tile-parts in tile order | EOC (0xFFD9). */
int  ojphgpu_t2_write_tiles(const ojphgpu_plan* plan, const uint8_t* h_block_data,
                            const ojphgpu_coded_block* blocks, uint32_t tile_first,
                            uint32_t tile_count, uint8_t* h_out, size_t cap, size_t* out_len,
                            uint32_t* tile_part_len);
int  ojphgpu_t2_write_main_header(const ojphgpu_plan* plan, const uint32_t* tile_part_len,
                                  uint8_t* h_out, size_t cap, size_t* out_len);
/* Parses main header + all tile-parts; creates the plan the codestream implies. */
int  ojphgpu_t2_parse(const uint8_t* h_codestream, size_t len, int resilient, ojphgpu_plan** out);
/* read_headers + restrict_input_resolution + read in the reference's order: the same as ojphgpu_t2_parse followed by
 * ojphgpu_plan_restrict_resolution on an undamaged codestream; on a damaged or truncated one the tile-parts are read the way
 * the reference reads them under the restriction (resolution-major progressions stop at the highest resolution wanted, packets
 * of unwanted resolutions are stepped over: ojph_tile.cpp:806-848, ojph_precinct.cpp:531-541). */
int  ojphgpu_t2_parse_restricted(const uint8_t* h_codestream, size_t len, int resilient, uint32_t skipped_res_for_data,
                                 uint32_t skipped_res_for_recon, ojphgpu_plan** out);
/* after ojphgpu_t2_parse: per-block coded info (offsets are into the parsed codestream) */
int  ojphgpu_plan_coded_blocks(const ojphgpu_plan* plan, ojphgpu_coded_block* out, size_t n);
/* after ojphgpu_t2_parse of a DAMAGED codestream: the blocks the reference would decode from bytes the codestream does not
 * hold -- a packet header promising more bytes than its tile-part has left makes bb_read_chunk (ojph_bitbuffer_read.h:134-150)
 * pad the block with zeros.  hdr = what the packet header said, got = how many of hdr.len1 + hdr.len2 bytes exist at
 * hdr.offset.  ojphgpu_plan_coded_blocks reports these blocks as not coded and the device decoder leaves them zero (what the
 * reference does with them when its block decoder refuses the padded bytes; the cases it does not are listed here).
 * *count receives how many there are (out == NULL: only that); OJPHGPU_E_OVERFLOW when cap is too small. */
typedef struct ojphgpu_padded_block { uint32_t block, got; ojphgpu_coded_block hdr; } ojphgpu_padded_block;
int  ojphgpu_plan_padded_blocks(const ojphgpu_plan* plan, ojphgpu_padded_block* out, size_t cap, size_t* count);
/* codestream::restrict_input_resolution (ojph_codestream_local.cpp:883-900) on a parsed plan, before
 * a decoder is created from it: the top `skipped_res_for_data` resolutions are not decoded and the
 * top `skipped_res_for_recon` (<= the former) are not synthesised.  The frame of the decoder -- and
 * what ojphgpu_plan_comp_info reports -- shrinks to ceil(size / 2^skipped_res_for_recon). */
int  ojphgpu_plan_restrict_resolution(ojphgpu_plan* plan, uint32_t skipped_res_for_data,
                                      uint32_t skipped_res_for_recon);
/* Region decoding (opj_set_decode_area, Kakadu -region): a decoder created from the plan afterwards does only the work the
 * samples of the rectangle depend on -- it decodes those code-blocks, uploads their bytes and synthesises those rows and
 * columns at every level -- and writes a frame that holds the region alone, bit for bit the crop of the whole frame.
 * (x0, y0, w, h) is a rectangle on the reference grid relative to the image origin: columns [image_x0 + x0, image_x0 + x0 + w),
 * also after restrict_resolution.  Component c, fx = XRsiz * 2^skipped_res_for_recon, gets the columns
 * [ceil(A0 / fx), ceil(A1 / fx)) of its own grid (A0, A1: the region's absolute bounds; rows alike); ojphgpu_plan_comp_info and
 * the frame size then describe the region frame, laid out as any frame.  A sub-sampled component may get an empty plane.
 * After ojphgpu_t2_parse (and after ojphgpu_plan_restrict_resolution, if at all; restrict_resolution on a region plan is
 * refused); once per plan.  OJPHGPU_E_INVALID, the plan unchanged: w or h 0, a rectangle not inside the image, a second call,
 * or a component of the general lifting kernels (an ATK wavelet, a DFS decomposition, 64-bit samples).
 * A region decoder takes ojphgpu_decoder_upload / run_device* / decode* / failed_blocks and the timing calls as any;
 * ojphgpu_decoder_create_batch when every plan carries the same region; ojphgpu_decoder_create_tiles only over all tiles.
 * failed_blocks counts the blocks the region needs, so a region decode fails only when one of those fails. */
int  ojphgpu_plan_restrict_region(ojphgpu_plan* plan, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
/* per block of the plan (plan order, n = the plan's block count): 1 = decoded for the region; blocks of resolutions that
 * are not read are 0.  A plan without a region: the blocks a whole-frame decoder decodes. */
int  ojphgpu_plan_region_blocks(const ojphgpu_plan* plan, uint8_t* mask, size_t n);
/* What a view decoder of a parsed plan (after any restriction) uploads: the bytes of the coded blocks it decodes
 * (ojphgpu_plan_region_blocks), as runs of blocks adjacent in the codestream.  Run i = n bytes at offset src of the
 * codestream, placed at dst of the staged bytes; sorted by src and strictly apart (src[i + 1] > src[i] + n[i]); every dst a
 * multiple of 64, the first one 64, dst[i + 1] >= align64(dst[i] + n[i]) + 64; *staged_len = align64(end of the last run) + 64.
 * Everything between the runs is zeros (the block decoder's 16-byte loads reach into the margins).  No coded block: no
 * runs, *staged_len = 0.  Blocks cut short by a damaged tile-part (ojphgpu_plan_padded_blocks) are not part of a run: their
 * copies go behind the staged bytes.  Host logic, no device: the table ojphgpu_gather_runs takes.
 * out == NULL: *count and *staged_len only; cap < *count: OJPHGPU_E_OVERFLOW with both set. */
typedef struct ojphgpu_run { uint64_t src, dst, n; } ojphgpu_run;
int  ojphgpu_plan_upload_runs(const ojphgpu_plan* plan, ojphgpu_run* out, size_t cap, size_t* count, uint64_t* staged_len);

/* ------------------------------------------------------------------------------------------ *
 * 4. Batched device stages.  Descriptor arrays live in device memory.
 * ------------------------------------------------------------------------------------------ */
typedef struct ojphgpu_dwt_desc {    /* one plane, one DWT level (32-bit elements everywhere) */
  uint64_t src_off, ll_off, hl_off, lh_off, hh_off;   /* element offsets from `base` */
  uint32_t src_pitch, ll_pitch, hl_pitch, lh_pitch, hh_pitch;
  uint32_t w, h;                                       /* size of the un-decomposed plane */
  uint32_t x_even, y_even;                             /* origin parity: 1 = even coordinate */
  uint32_t reserved;
} ojphgpu_dwt_desc;

/* K1-K4 (ojph_transform.cpp:209-852 driven by ojph_resolution.cpp:547-949).  `reversible`
 * selects the 5/3 integer or the 9/7 float lifting; `base` is int32 or float accordingly.
 * max_w / max_h = largest plane in the batch (sizes the launch grid). */
int ojphgpu_dwt_forward(void* stream, int reversible, const ojphgpu_dwt_desc* d_descs, uint32_t n,
                        uint32_t max_w, uint32_t max_h, void* d_base);
int ojphgpu_dwt_inverse(void* stream, int reversible, const ojphgpu_dwt_desc* d_descs, uint32_t n,
                        uint32_t max_w, uint32_t max_h, void* d_base);

/* The transform in its GENERAL form (kernels_lift.hip): any lifting kernel an ATK marker segment can describe
 * (param_atk, ojph_params.cpp:2654-2896), levels that transform one direction only (DFS marker segment:
 * resolution::pull_line's HORZ_TRX / VERT_TRX, ojph_resolution.cpp:290-300, :725-949), and 64-bit integer samples
 * (gen_rev_vert_step64 / gen_rev_horz_ana64 / _syn64, ojph_transform.cpp:261,415,593 -- the reference's sample path
 * for more than 32 bits of precision).  Steps are listed in synthesis order; a reversible step is
 * x -+= (b + a (l + r)) >> e, an irreversible one x -+= A (l + r) with K scaling around the steps.
 * elem: 0 = int32, 1 = int64 planes (an element offset of a descriptor still counts 32-bit elements, a pitch counts
 * samples), 2 = float.  horz / vert = 0: the level leaves that direction alone -- all its samples are "low" there, only
 * ll and hl (vert = 0) or ll and lh (horz = 0) are read / written.  The planes the descriptors name as src are
 * transformed IN PLACE before they are split into the bands (forward) / after they are joined (inverse). */
typedef struct ojphgpu_lift {
  uint32_t num_steps, elem, horz, vert;
  float    K;
  ojphgpu_lift_step steps[OJPHGPU_MAX_LIFT_STEPS];
} ojphgpu_lift;
int ojphgpu_dwt_forward_general(void* stream, const ojphgpu_lift* kernel, const ojphgpu_dwt_desc* d_descs, uint32_t n,
                                uint32_t max_w, uint32_t max_h, void* d_base);
int ojphgpu_dwt_inverse_general(void* stream, const ojphgpu_lift* kernel, const ojphgpu_dwt_desc* d_descs, uint32_t n,
                                uint32_t max_w, uint32_t max_h, void* d_base);
/* the top level of general-lifting components with the conversion from / to the image samples fused in, like
 * ojphgpu_dwt_forward_image_ex / _inverse_image_ex do it for the 5/3 and the 9/7 (rev_convert / irv_convert_to_float / ..._to_integer,
 * ojph_colour.cpp:238-436, applied in the level's loads / stores): int32 or float working samples (kernel->elem 0 / 2), one to
 * four lifting steps, both directions; d_descs address the image planes as for the _image_ex calls (reserved = the plane's own
 * bit depth | signed << 8, or 0 for params'); container_bits 8 / 16 / 32.  No colour transform. */
int ojphgpu_dwt_forward_general_image(void* stream, const ojphgpu_lift* kernel, const ojphgpu_params* params, const ojphgpu_dwt_desc* d_descs,
                                      uint32_t n, uint32_t max_w, uint32_t max_h, const void* d_image, void* d_base, int container_bits);
int ojphgpu_dwt_inverse_general_image(void* stream, const ojphgpu_lift* kernel, const ojphgpu_params* params, const ojphgpu_dwt_desc* d_descs,
                                      uint32_t n, uint32_t max_w, uint32_t max_h, void* d_image, void* d_base, int container_bits);

/* The same transforms with the sample conversion of the adjacent stage fused in (no colour
 * transform): the first analysis level reads the int32 image planes directly -- level shift
 * (gen_rev_convert, ojph_colour.cpp:238) or int -> float (gen_irv_convert_to_float, :388) applied
 * in the load -- and the last synthesis level writes them (gen_irv_convert_to_integer, :316).
 * For these two calls desc.src_off / src_pitch address the plane inside d_image (elements),
 * everything else inside d_base.  Saves one read + one write of the whole frame per direction. */
int ojphgpu_dwt_forward_image(void* stream, const ojphgpu_params* params,
                              const ojphgpu_dwt_desc* d_descs, uint32_t n, uint32_t max_w,
                              uint32_t max_h, const int32_t* d_image, void* d_base);
/* the general form of the four calls around it: container_bits = 32 | 16 | 8 (two's complement for signed
 * components, else the full unsigned range of the container; bit depths up to the container's width, 31 for
 * 32).  colour != 0: the descriptors come in triples -- the planes of the three colour components of a tile,
 * which share their geometry -- and the component transform (RCT for the 5/3, ICT for the 9/7:
 * gen_rct_forward / _backward, gen_ict_forward / _backward, ojph_colour.cpp:443-571) is applied in the same
 * loads / stores, so that a colour-transformed frame needs no conversion pass over HBM either. */
int ojphgpu_dwt_forward_image_ex(void* stream, const ojphgpu_params* params, const ojphgpu_dwt_desc* d_descs, uint32_t n,
                                 uint32_t max_w, uint32_t max_h, const void* d_image, void* d_base, int container_bits, int colour);
int ojphgpu_dwt_inverse_image_ex(void* stream, const ojphgpu_params* params, const ojphgpu_dwt_desc* d_descs, uint32_t n,
                                 uint32_t max_w, uint32_t max_h, void* d_image, void* d_base, int container_bits, int colour);
/* Region synthesis: regions[i] (device memory, parallel to the descriptors) is the range of descriptor i's plane whose samples
 * are wanted exactly, in plane coordinates; the launch covers the strips and row pairs over it.  d_image == NULL: a lower level,
 * written into the plane in the arena (whole strips, inside the plane).  d_image set: the top level, plane sample (x, y) of the
 * range written to element out_off + (y - ry0) * out_pitch + (x - rx0) of d_image in `container` (32 | 16 | 8)-bit samples,
 * converted with the descriptor's `reserved` = bit depth | is_signed << 8.  5/3 and 9/7 only.  Reads the descriptors and
 * regions back to size the grid (synchronises the stream); the decoders size it from their own copies.  _ex: colour != 0 =
 * descriptor triples of the three colour planes, the inverse component transform in the stores (as _image_ex). */
typedef struct ojphgpu_dwt_region {
  uint32_t rx0, ry0, rx1, ry1;       /* exact range [rx0, rx1) x [ry0, ry1) in plane coordinates (empty: nothing to do) */
  uint64_t out_off;                  /* top level: element offset of sample (rx0, ry0) in d_image */
  uint32_t out_pitch, reserved;      /* top level: elements per row of d_image */
} ojphgpu_dwt_region;
int ojphgpu_dwt_inverse_region(void* stream, int reversible, const ojphgpu_dwt_desc* d_descs, const ojphgpu_dwt_region* d_regions,
                               uint32_t n, void* d_base, void* d_image, int container);
int ojphgpu_dwt_inverse_region_ex(void* stream, int reversible, const ojphgpu_dwt_desc* d_descs, const ojphgpu_dwt_region* d_regions,
                                  uint32_t n, void* d_base, void* d_image, int container, int colour);
/* the same with the image samples in 16-bit containers: int16 (two's complement) for signed
 * components, uint16 otherwise; bit depths up to 16.  Halves the HBM traffic of the image side of
 * the top level (and the PCIe traffic of whoever fills / drains the image buffer). */
int ojphgpu_dwt_forward_image16(void* stream, const ojphgpu_params* params,
                                const ojphgpu_dwt_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                                const uint16_t* d_image, void* d_base);
int ojphgpu_dwt_inverse_image16(void* stream, const ojphgpu_params* params,
                                const ojphgpu_dwt_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                                uint16_t* d_image, void* d_base);
int ojphgpu_dwt_inverse_image(void* stream, const ojphgpu_params* params,
                              const ojphgpu_dwt_desc* d_descs, uint32_t n, uint32_t max_w,
                              uint32_t max_h, int32_t* d_image, void* d_base);

typedef struct ojphgpu_cb_desc {     /* one code-block */
  uint64_t coef_off;                 /* element offset of the block's first sample in `d_coef` */
  uint32_t pitch;                    /* elements */
  uint16_t w, h;
  uint8_t  K_max, reversible, missing_msbs, num_passes;   /* last two: decode only; reversible bit 1
                                        (decode): vertically causal code-block style; bit 2: the block is on the
                                        64-bit sample path (int64 samples at coef_off, the 64-bit block coder);
                                        bit 3 (encode, 32-bit reversible blocks only): code the block at
                                        p = 30 - missing_msbs, i.e. without its K_max - 1 - missing_msbs lowest
                                        magnitude planes (section 5f); without the bit missing_msbs is not read
                                        on encode */
  float    delta;                    /* irreversible: encode uses 1/delta, decode uses delta */
  uint32_t len1, len2;               /* decode: pass lengths */
  uint64_t data_off;                 /* decode: byte offset of the coded bytes in `d_data`;
                                        encode: byte offset of this block's scratch slot */
  uint32_t scratch_cap;              /* encode: bytes available at data_off; decode: offset of the
                                        block's first per-quad record in d_quad_scratch (elements),
                                        see ojphgpu_ht_decode_layout */
  uint32_t reserved;                 /* decode: offset of the block's area in d_aux (elements) */
} ojphgpu_cb_desc;

typedef struct ojphgpu_cb_result {   /* encode result per block */
  uint32_t offset;                   /* byte offset of the block in the compacted output */
  uint32_t length;                   /* pass_length[0]; 0 = block has no significant sample */
} ojphgpu_cb_result;

/* K5/K6 + K8: quantise transfer (ojph_codestream_gen.cpp:59-121) fused into the HT cleanup
 * encoder (ojph_block_encoder.cpp:542-1017).  One wavefront per code-block.  d_cursor is a
 * device uint32 (zeroed by the caller) that ends up holding the number of bytes written to
 * d_out; d_status (device uint32, zeroed) receives a non-zero value on scratch/out overflow. */
int ojphgpu_ht_encode(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                      const void* d_coef, uint8_t* d_scratch, uint8_t* d_out, uint32_t out_cap,
                      ojphgpu_cb_result* d_results, uint32_t* d_cursor, uint32_t* d_status);
/* The block encoder as a stage with what the encoder objects know and use: the kinds of the blocks, and output regions.
 * ojphgpu_ht_encode_ex: ojphgpu_ht_encode (== widths 3 | 32, nreg 0, first 0) with that knowledge.  d_blocks and d_results
 *   point at the FIRST block of the range that is coded; `first` is that block's index among all blocks of the caller (a
 *   caller that codes one array in several launches passes the same regions, cursor and output to each) and only chooses
 *   regions.  Regions: nreg = 0, the single cursor d_cursor[0] over d_out[0 .. out_cap); else nreg (a power of two) regions,
 *   d_regions[2 r] = first byte of region r in d_out, d_regions[2 r + 1] = its bytes, its cursor (zeroed by the caller) at
 *   d_cursor[32 r]; block i of the launch takes a 4-byte aligned slot in region (first + i) & (nreg - 1).  A block whose
 *   slot does not fit what is left of its region, or whose scratch slot is too small, reports offset 0, length 0, writes
 *   nothing to d_out and sets *d_status (d_cursor + 1 in the objects); a cursor counts every request, also a refused one.
 * `widths` says what the blocks of the range are; every launched kernel skips the blocks that are not its own:
 *   bit 0 (1)    blocks of at most 64 columns occur           bit 1 (2)    blocks of more than 64 columns occur
 *   bit 2 (4)    reversible blocks occur                      bit 3 (8)    irreversible blocks occur  (neither: both)
 *   bit 4 (16)   NO block of 33..64 columns occurs: the blocks of bit 0 take the layout of 8 quad pairs by 8 quad rows
 *   bit 5 (32)   blocks on the 64-bit sample path occur (cb_desc.reversible bit 2; bits 0..4 and 6 say nothing of them)
 *   bit 6 (64)   NO block of more than 128 columns occurs: the blocks of bit 1 take the narrow kernel, 32 pairs by 2 rows
 *   bit 7 (128)  reversible blocks that drop low bit-planes occur (cb_desc.reversible bit 3): instantiations of their own,
 *                launched behind the others in the layouts bits 0, 1, 4 and 6 name (such a block says nothing of bit 2).  A
 *                caller that does not know CANNOT coarsen this one in: without bit 7 no kernel owns a flagged block.
 * ojphgpu_ht_encode_kinds: host only -- the truthful widths of h_blocks[0 .. n), the statement the encoder objects use too
 *   (a descriptor without samples, w or h 0, counts with its w and reversible like any other: a kernel must report it).
 *   It is also where flagged descriptors are validated: one with missing_msbs >= K_max, on the 64-bit path (bit 2) or
 *   irreversible is OJPHGPU_E_INVALID -- a caller launches nothing then.
 * A caller may know LESS than ojphgpu_ht_encode_kinds says, never more.  The valid coarsenings of a truthful value, in any
 * combination:
 *   - clear bit 4: the blocks of at most 32 columns take the 16-pairs-by-4-rows layout of the 64-column blocks;
 *   - clear bit 6: the blocks of 65..128 columns take the raster-order wide kernel;
 *   - set both or neither of bits 2 and 3: both wavelets' instantiations run;
 *   - set bits 0, 1 or 5 that the truth lacks: a kernel is launched that finds no block of its own.
 * Everything else is invalid: clearing bit 0, 1 or 5 that the truth sets, stating one wavelet where the other occurs, or
 * setting bit 4 or 6 that the truth lacks.  Then no launched instantiation owns some block (e.g. bit 4 set with a 40-column
 * block present: the 8-by-8 layout takes blocks of at most 32 columns only) and that block's result is NEVER WRITTEN -- no
 * error is reported, d_results keeps what the caller left there.
 * ojphgpu_ht_encode_launches: host only, no HIP call -- what ojphgpu_ht_encode_ex launches for n blocks under `widths`, in
 *   issue order; it takes its launches from the same table.  *count launches (at most 7; 5 without bit 7), five values each in `out`:
 *   [0] 0 = ht_encode_kernel<REV, LOGP>, 1 = ht_encode_wide_kernel<S64>; [1] REV, or S64 (+ 2: the instantiation of the
 *   blocks that drop bit-planes -- 3 narrow, 2 wide); [2] LOGP (3: 8 pairs by 8 quad
 *   rows, 4: 16 by 4, 5: 32 by 2; 0 for the wide kernel); [3] workgroups; [4] blocks (wavefronts) per workgroup.  `cap` =
 *   the launches `out` has room for; E_INVALID (with *count set) where cap < *count. */
int ojphgpu_ht_encode_ex(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                         const void* d_coef, uint8_t* d_scratch, uint8_t* d_out, uint32_t out_cap,
                         ojphgpu_cb_result* d_results, uint32_t* d_cursor, uint32_t* d_status,
                         int widths, const uint32_t* d_regions, uint32_t nreg, uint32_t first);
int ojphgpu_ht_encode_kinds(const ojphgpu_cb_desc* h_blocks, uint32_t n, int* widths);
int ojphgpu_ht_encode_launches(uint32_t n, int widths, uint32_t* out, uint32_t cap, uint32_t* count);

/* K9 + K7: HT decoder (ojph_block_decoder32.cpp:742-1613) with the dequantise transfer
 * (ojph_codestream_gen.cpp:124-168) fused.  Three launches: prep (one wavefront per block:
 * un-stuffs the VLC and MEL segments into flat bit strings in d_aux), step 1 (the serial MEL /
 * VLC / U-VLC chains, one lane per block -> one 32-bit record per quad in d_quad_scratch), step 2
 * (MagSgn -> de-quantised samples, one wavefront per block, one lane per sample column).
 * The scratch of the two intermediate products is laid out by ojphgpu_ht_decode_layout, which fills
 * blocks[i].scratch_cap and blocks[i].reserved of the HOST copy of the descriptors before they are
 * uploaded:
 *  - per-quad records: step 1 advances 64 blocks per wavefront (descriptors 64g .. 64g+63 of a
 *    launch), one quad PAIR per lane and iteration, so the records of such a group are interleaved
 *    pair-major -- pair p of the group's lane l sits at group base + 2 * (64 p + l) -- and every store
 *    of the wavefront is one contiguous 512-byte segment.  blocks[i].scratch_cap = offset (uint32
 *    elements) of the block's pair 0; pair p = quad row * ceil(QW / 2) + quad pair follows 128 p
 *    elements further.  A launch over a sub-range must start at a multiple of 64 descriptors of the
 *    array that was laid out.
 *  - blocks[i].reserved = offset (uint32 elements) of the block's flat VLC / MEL strings inside
 *    d_aux, ojphgpu_ht_decode_aux_words(len1) elements long.
 * d_block_status[i] = 0 ok / non-zero failed (block zeroed), mirroring the bool of decode_cb32. */
uint32_t ojphgpu_ht_decode_aux_words(uint32_t len1);
int ojphgpu_ht_decode_layout(ojphgpu_cb_desc* h_blocks, uint32_t n, uint64_t* quad_elems, uint64_t* aux_elems);
int ojphgpu_ht_decode(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                      const uint8_t* d_data, void* d_coef, uint32_t* d_quad_scratch,
                      uint32_t* d_aux, uint8_t* d_block_status);
/* the three launches one by one (ojphgpu_ht_decode == prep, step1, step2 in this order) */
int ojphgpu_ht_decode_prep(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                           const uint8_t* d_data, uint32_t* d_aux);
int ojphgpu_ht_decode_step1(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                            const uint8_t* d_data, const uint32_t* d_aux, uint32_t* d_quad_scratch,
                            uint8_t* d_block_status);
int ojphgpu_ht_decode_step2(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                            const uint8_t* d_data, const uint32_t* d_quad_scratch, void* d_coef,
                            uint8_t* d_block_status);
/* The separate launches as a stage: step 2 with the caller's knowledge of the blocks, and what will run (host only).
 * `kinds` says what the blocks of a range are, OR-ed over the blocks; 0 = nothing is known, always valid:
 *   bit 0 (1)    blocks of at most 64 columns occur          bit 1 (2)    blocks of more than 64 columns occur
 *   bit 2 (4)    reversible blocks occur                     bit 3 (8)    irreversible blocks occur
 *   bit 4 (16)   blocks with SigProp / MagRef passes occur (num_passes > 1 and len2 > 0)
 *   bit 5 (32)   blocks on the 64-bit sample path occur (cb_desc.reversible bit 2; these launches skip them, the bit chooses nothing)
 *   bit 6 (64)   blocks of more than 32 columns occur        bit 7 (128)  blocks of more than 16 columns occur
 *   bit 8 (256)  bits 6 and 7 are filled in: only with it SET does a clear bit 6 / 7 mean "every block is at most 32 / 16 wide"
 * ojphgpu_ht_decode_kinds: host only -- the kinds of h_blocks[0 .. n), the statement of the bits the decoder objects use too.
 * The kernels are specialised by it (one transfer, narrow blocks, two or four blocks of at most 32 / 16 columns to a wavefront)
 * and a specialised kernel leaves alone or mis-decodes a block it was told does not occur.  So a caller may know LESS than
 * ojphgpu_ht_decode_kinds says, never more.  The valid coarsenings of a truthful value, in any combination:
 *   - set bit 7, or bits 6 and 7: two blocks, or one, to a wavefront where the truth allows four, or two;
 *   - clear bit 8: one block to a wavefront;
 *   - set both bits 2 and 3: the kernel that reads each block's transfer from its descriptor (also what bit 4 selects);
 *   - set bit 1: the kernel that also takes blocks of up to 128 columns.
 * Clearing any of bits 0..4, 6, 7 that ojphgpu_ht_decode_kinds sets, or setting bit 8 where it was not computed, is invalid.
 * ojphgpu_ht_decode_step2_kinds: ojphgpu_ht_decode_step2 (== kinds 0) with that knowledge.
 * ojphgpu_ht_decode_launches: host only, no HIP call -- what ojphgpu_ht_decode_step1 and ojphgpu_ht_decode_step2_kinds launch
 *   for n blocks of `kinds` under this process's OJPHGPU_S1_CH / OJPHGPU_DEC_PREP / OJPHGPU_DEC_DUAL (read once); both take
 *   their choice from it.  out[0] step 1 reads prep's flat strings (1: ht_dec_step1_kernel) or the raw bytes (0:
 *   ht_dec_step1_raw_kernel; ojphgpu_ht_decode_prep then launches nothing), [1] its CH (64 CH blocks per workgroup), [2] its
 *   workgroups; [3] step 2 is ht_dec_step2_multi_kernel<TX, NB> (1) or ht_dec_step2_kernel<TX, WD> (0), [4] TX (0: per block,
 *   1 reversible, 2 irreversible), [5] WD (1: no block wider than 64), [6] NB blocks per wavefront (1 for the single kernel),
 *   [7] its workgroups, [8] blocks per workgroup.  `out` holds 9 values. */
int ojphgpu_ht_decode_kinds(const ojphgpu_cb_desc* h_blocks, uint32_t n, int* kinds);
int ojphgpu_ht_decode_step2_kinds(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                                  const uint8_t* d_data, const uint32_t* d_quad_scratch, void* d_coef,
                                  uint8_t* d_block_status, int kinds);
int ojphgpu_ht_decode_launches(uint32_t n, int kinds, uint32_t* out);
/* Step 1 and step 2 in ONE launch (ht_dec_fused_kernel, what the decoder objects take for blocks of at most 64 columns
 * without refinement passes where it pays), as a stage of its own.
 * ojphgpu_ht_decode_fused_shape: host only -- how the launch deals n blocks out on `cus` compute units (0: 256) under the
 *   process's OJPHGPU_FUSED_SHAPE / OJPHGPU_FUSED_RINGS: out[0] shape, [1] chains per step-1 workgroup, [2] wavefronts per
 *   workgroup, [3] step-1 workgroups n1, [4] blocks per worker wavefront, [5] worker workgroups, [6] NR of the kernel
 *   instantiation (un-stuffing rings per worker wavefront), [7] 1 where n1 <= cus (the launch is able to run), else 0,
 *   [8] the blocks per worker wavefront the resident wavefront slots ask for, before the cap of 8 (more than [4]: worker
 *   workgroups beyond the resident ones, which start when others end).  `out` holds 9 values.
 * ojphgpu_ht_decode_fused_slices: host only -- the slices of quad rows of a launch whose tallest block has max_h rows:
 *   *count of them, slice i = quad rows [out_bounds[2i], out_bounds[2i + 1]); E_INVALID (with *count set) where cap < *count.
 * ojphgpu_ht_decode_fused_state_words: uint32 elements of d_state for n blocks.
 * ojphgpu_ht_decode_fused: the launch.  d_blocks: the whole array ojphgpu_ht_decode_layout laid out, every block at most 64
 *   columns wide, cleanup pass only, all reversible or all irreversible (`reversible`); d_quad_scratch: quad_elems elements
 *   of that layout; d_state: ojphgpu_ht_decode_fused_state_words(n) elements, zeroed ONCE -- nothing is cleared between
 *   runs, `epoch` > 0 must grow from run to run on it; max_h: the tallest block; d_block_status: n bytes and, at the next
 *   multiple of 4, the 4-byte RETRY word (== epoch after the run: a wait ran out, the blocks have to be decoded again through
 *   the separate launches); cus: the compute units to deal the work out for, 0 or more than the current device has = all
 *   of the device's (fewer only: every workgroup of the launch must be resident).  E_INVALID where the launch would need
 *   more step-1 workgroups than `cus`. */
int ojphgpu_ht_decode_fused_shape(uint32_t n, uint32_t cus, uint32_t* out);
int ojphgpu_ht_decode_fused_slices(uint32_t max_h, uint32_t* out_bounds, uint32_t cap, uint32_t* count);
uint64_t ojphgpu_ht_decode_fused_state_words(uint32_t n);
int ojphgpu_ht_decode_fused(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n, const uint8_t* d_data, void* d_coef,
                            uint32_t* d_quad_scratch, uint32_t* d_state, uint8_t* d_block_status, uint32_t epoch,
                            uint32_t max_h, int reversible, uint32_t cus);
/* fourth launch, only needed when some block has num_passes > 1 (foreign codestreams): SigProp +
 * MagRef passes (ojph_block_decoder32.cpp:1318-1609) over the blocks that carry them; step 2 left
 * those blocks as sign-magnitude words, this launch refines and de-quantises them.  Bit 1 of
 * blocks[i].reversible selects the vertically (stripe) causal mode of the code-block style.
 * d_quad_scratch: the records ojphgpu_ht_decode_step1 wrote -- the significance the passes start from
 * is the quads' rho bits, as in the reference (:1321-1351), not "the decoded sample is not zero". */
int ojphgpu_ht_decode_refine(void* stream, const ojphgpu_cb_desc* d_blocks, uint32_t n,
                             const uint8_t* d_data, const uint32_t* d_quad_scratch, void* d_coef,
                             const uint8_t* d_block_status);

typedef struct ojphgpu_convert_desc { /* one tile-component */
  uint64_t plane_off;                /* element offset in the arena */
  uint32_t pitch, w, h;
  uint32_t src_x0, src_y0;           /* position inside the component's image plane */
  uint32_t img_pitch;                /* width of that plane */
  uint64_t img_off;                  /* element offset of that plane in the image buffer (a frame
                                        batch adds the frame's offset) */
  uint32_t fmt;                      /* bit depth | signed << 8 of the component; 0 = from params;
                                        | 0x200 when bit 10 says which conversion the component takes
                                        (1 = reversible level shift, 0 = to float): components with a COC;
                                        | 0x800: NLT type 3 (negative v <-> -v - 2^(B-1) - 1, ojph_colour.cpp:273-311);
                                        | 0x1000: the component is on the 64-bit sample path, its plane holds int64
                                        samples (gen_rev_convert 32 <-> 64 bits, gen_rct_* with 64-bit Y Cb Cr,
                                        ojph_colour.cpp:250-268, :467-489, :517-541) */
  uint32_t reserved;
} ojphgpu_convert_desc;

/* K10/K11: level shift / int<->float conversion and RCT / ICT (ojph_colour.cpp:238-571 as
 * driven by tile::push/pull, ojph_tile.cpp:332-518).  Image samples are int32 planes
 * (component-major, see ojphgpu_plan_comp_info), like the i32 line_bufs the reference exchanges.
 * With the colour transform the first three components share their geometry. */
int ojphgpu_convert_forward(void* stream, const ojphgpu_params* params,
                            const ojphgpu_convert_desc* d_descs, uint32_t n_tiles,
                            uint32_t max_w, uint32_t max_h, const int32_t* d_image, void* d_arena);
int ojphgpu_convert_inverse(void* stream, const ojphgpu_params* params,
                            const ojphgpu_convert_desc* d_descs, uint32_t n_tiles,
                            uint32_t max_w, uint32_t max_h, int32_t* d_image, const void* d_arena);
/* container_bits = 32 | 16 | 8 */
int ojphgpu_convert_forward_ex(void* stream, const ojphgpu_params* params, const ojphgpu_convert_desc* d_descs, uint32_t n_tiles,
                               uint32_t max_w, uint32_t max_h, const void* d_image, void* d_arena, int container_bits);
int ojphgpu_convert_inverse_ex(void* stream, const ojphgpu_params* params, const ojphgpu_convert_desc* d_descs, uint32_t n_tiles,
                               uint32_t max_w, uint32_t max_h, void* d_image, const void* d_arena, int container_bits);
/* 16-bit sample containers (see ojphgpu_dwt_forward_image16) */
int ojphgpu_convert_forward16(void* stream, const ojphgpu_params* params,
                              const ojphgpu_convert_desc* d_descs, uint32_t n_tiles,
                              uint32_t max_w, uint32_t max_h, const uint16_t* d_image, void* d_arena);
int ojphgpu_convert_inverse16(void* stream, const ojphgpu_params* params,
                              const ojphgpu_convert_desc* d_descs, uint32_t n_tiles,
                              uint32_t max_w, uint32_t max_h, uint16_t* d_image, const void* d_arena);

/* Band statistics (section 5b builds on them): one pass over sub-band planes of fp32 coefficients, an 80-bin histogram of
 * the magnitudes in half octaves per slot.  With u the 32 bits of a coefficient, bin = clamp(((u >> 22) & 0x1FF) - 191,
 * 0, 79) -- the exponent field and the top mantissa bit: bin 0 holds zeros, denormals and everything below 2^-31, bin 63
 * holds [1, 1.5), bin 79 everything from 2^8 up, infinities and NaNs included.  Only the w x h samples of a plane count
 * (rows of `pitch` >= w elements; the padding does not, though it may be read); several descriptors may share a slot.
 * d_hist[slot][80] holds exact counts (uint32) and is zeroed by the caller.  max_w / max_h: the largest w / h among the
 * descriptors, as for the DWT; max_w at most 2^21. */
#define OJPHGPU_STATS_BINS 80
typedef struct ojphgpu_stats_desc { uint64_t plane_off; uint32_t pitch, w, h, slot; } ojphgpu_stats_desc;
int ojphgpu_band_stats(void* stream, const ojphgpu_stats_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                       const void* d_coef, uint32_t* d_hist);
/* The integer form (section 5f builds on it): the same pass over planes of int32 coefficients (the reversible path), the
 * same kernel with another counting function.  bin = the bit length of |v| -- 0 for 0, 1 for +-1, 31 for INT_MAX, 32 for
 * INT_MIN; bins 33 .. 79 of a slot stay zero.  Descriptors, slots, exact uint32 counts and the limits are those above. */
int ojphgpu_band_stats_int(void* stream, const ojphgpu_stats_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                           const void* d_coef, uint32_t* d_hist);

/* The two passes of a trial of the quality search (section 5c builds on them; kernels_quality.hip).
 *
 * ojphgpu_band_requantise: sub-band planes of fp32 coefficients in d_src_arena -> the same planes in d_dst_arena (same
 * offsets) as the decoder holds them after the block decoder, had the planes been coded with these band parameters.  Per
 * sample, in this order: the irreversible quantise transfer of the block encoder (f = coefficient * delta_inv rounded to
 * nearest, truncated to an integer; a product beyond +-2^31 or a NaN gives the zero word); with p = 31 - K_max and m =
 * magnitude >> p the word 0 when m == 0, else sign | m << p | 1 << (p - 1) -- the bits the cleanup pass carries and the
 * half bit the decoder puts below them; the irreversible de-quantise transfer of the block decoder ((float) magnitude *
 * delta, the sign OR-ed in; a zero word is +0.0f).  Writes the w x h samples of every plane and nothing else, reads the
 * source only.  A descriptor with K_max outside 1 .. 30, or wider than max_w, is skipped.  max_w / max_h: the largest w /
 * h among the descriptors, max_w at most 2^21. */
typedef struct ojphgpu_requant_desc { uint64_t plane_off; uint32_t pitch, w, h; float delta_inv, delta; uint32_t K_max; } ojphgpu_requant_desc;
int ojphgpu_band_requantise(void* stream, const ojphgpu_requant_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                            const void* d_src_arena, void* d_dst_arena);
/* ojphgpu_frame_error: component c = the elements [first_elem, first_elem + count) of two frames d_a, d_b in
 * container_bits (8 | 16 | 32)-bit containers -- int8 / int16 for is_signed != 0, else uint8 / uint16; 32-bit containers
 * hold int32 whatever is_signed says.  d_out[c].sse += the sum of (a - b)^2 over the run (exact; modulo 2^64, which
 * differences of 16 bits or fewer cannot reach below 2^32 samples), d_out[c].pae = max(d_out[c].pae, the largest |a - b|):
 * the caller zeroes d_out.  Integer sums: the result does not depend on the order.  A run may start at any element, count
 * may be 0; n_comps at most 65535. */
typedef struct ojphgpu_error_comp { uint64_t first_elem, count; uint32_t is_signed, reserved; } ojphgpu_error_comp;
typedef struct ojphgpu_frame_err { uint64_t sse; uint32_t pae, reserved; } ojphgpu_frame_err;
int ojphgpu_frame_error(void* stream, const void* d_a, const void* d_b, int container_bits, const ojphgpu_error_comp* d_comps,
                        uint32_t n_comps, ojphgpu_frame_err* d_out);
/* the same with the second frame in a container of its own: bits_b == bits_a, or 32 -- int32 samples against a frame in 8-
 * or 16-bit containers (is_signed says how the first frame's samples read).  What the quality search compares: a decoded
 * sample may lie one past its nominal range (256 for an 8-bit component: the reference rounds after its range test), which
 * int32 hands over as it is and a narrower container saturates. */
int ojphgpu_frame_error_ex(void* stream, const void* d_a, int bits_a, const void* d_b, int bits_b, const ojphgpu_error_comp* d_comps,
                           uint32_t n_comps, ojphgpu_frame_err* d_out);
/* ojphgpu_frame_fit (section 5e builds on it; kernels_fit.hip): an int32 frame as ojphgpu_decoder_run_device leaves it -> the
 * frame an encoder of another bit depth takes.  Component c = the elements [first_elem, first_elem + count) of both frames;
 * per sample v' = (v + 2^(shift - 1)) >> shift for shift > 0 (an arithmetic shift, round half up, evaluated in 64 bits),
 * v << -shift for shift < 0, v for shift == 0, then clamped to [lo, hi] -- what writing the decoded image to a file of the
 * output's depth and reading it back does (the reference's image writers saturate: src/apps/others/ojph_img_io.cpp:106-230, :1208-1296).
 * d_dst holds container_bits (8 | 16 | 32)-bit containers: int8 / int16 where lo < 0, else uint8 / uint16; 32-bit containers
 * hold int32.  d_dst == d_src is allowed at 32 bits (and only there); otherwise the frames do not overlap.  Writes the count
 * elements of every component and nothing else; a run may start at any element, count may be 0.  |shift| <= 31 and lo <=
 * hi, or the component is left alone; n_comps at most 65535. */
typedef struct ojphgpu_fit_comp { uint64_t first_elem, count; int32_t shift, lo, hi; uint32_t reserved; } ojphgpu_fit_comp;
int ojphgpu_frame_fit(void* stream, const int32_t* d_src, void* d_dst, int container_bits, const ojphgpu_fit_comp* d_comps,
                      uint32_t n_comps);
/* ojphgpu_frame_resample (section 5e, "a resampling recode"; kernels_fit.hip): the fit with components halved on the way, in
 * the same pass.  Component c = the src_w x src_h samples (rows src_w apart) from element src_first of the int32 frame ->
 * the dst_w x dst_h samples (rows dst_w apart) from element dst_first of d_dst's containers.  fx, fy: 1 (kept) or 2 (halved)
 * per direction; px, py: 0 or 1, the phase -- output sample i of a halved direction stands ON source sample 2 i + p, so
 * dst_w == (src_w + 1 - px) / 2 where fx == 2 (src_w where fx == 1; rows alike; either may come to 0: nothing is written).
 * Per output sample the taps (1, 2, 1) around that source sample in every halved direction, indices clamped into the
 * plane, summed exactly in 64 bits and rounded once ((acc + 2^(k-1)) >> k, k = 2 per halved direction); then the fit of
 * ojphgpu_frame_fit with shift, lo, hi, and its containers.  A component with fx == fy == 1 is that fit itself.  The frames
 * never overlap.  Writes the dst_w * dst_h elements of every component and nothing else.  A factor other than 1 or 2, a
 * phase above 1, |shift| > 31, lo > hi or sizes that contradict the rule: the component is left alone; n_comps at most
 * 65535.  (pipeline.resample_plane states the filter in numpy.) */
typedef struct ojphgpu_resample_comp {
  uint64_t src_first, dst_first; uint32_t src_w, src_h, dst_w, dst_h; uint32_t fx, fy, px, py; int32_t shift, lo, hi; uint32_t reserved;
} ojphgpu_resample_comp;
int ojphgpu_frame_resample(void* stream, const int32_t* d_src, void* d_dst, int container_bits, const ojphgpu_resample_comp* d_comps,
                           uint32_t n_comps);

/* ------------------------------------------------------------------------------------------ *
 * 5. Whole-frame codec objects: what an ojph::codestream-compatible facade calls from
 *    flush() (encode) and create()/pull() (decode).
 * ------------------------------------------------------------------------------------------ */
typedef struct ojphgpu_encoder ojphgpu_encoder;
typedef struct ojphgpu_decoder ojphgpu_decoder;

int  ojphgpu_encoder_create(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_encoder** out);
void ojphgpu_encoder_destroy(ojphgpu_encoder* enc);
/* An encoder that codes only tiles [tile_first, tile_first + tile_count) of the plan's frame: the
 * unit of multi-GPU sharding (one rank = one contiguous run of tiles).  d_image still addresses
 * the whole frame; only the rows/columns of the range's tiles are read. */
int  ojphgpu_encoder_create_tiles(const ojphgpu_plan* plan, int device, void* stream,
                                  uint32_t tile_first, uint32_t tile_count, ojphgpu_encoder** out);
/* D2H + host Tier-2 of the range: its tile-parts only (see ojphgpu_t2_write_tiles) */
int  ojphgpu_encoder_finish_tiles(ojphgpu_encoder* enc, uint8_t* h_out, size_t cap, size_t* out_len,
                                  uint32_t* tile_part_len);
/* the same with the tile-parts left in DEVICE memory (assembled there by a placement kernel; only the block
 * lengths visit the host): d_out receives *out_len bytes.  What a rank hands to the final codestream gather
 * of a multi-GPU encode (RCCL over xGMI) without a host round trip.  OJPHGPU_E_OVERFLOW + *out_len = need. */
int  ojphgpu_encoder_finish_tiles_device(ojphgpu_encoder* enc, uint8_t* d_out, size_t cap, size_t* out_len,
                                         uint32_t* tile_part_len);
/* An encoder for a BATCH of num_frames independent frames of the plan's shape (video: BASELINE
 * config "512 independent 4K frames"): one set of launches codes all of them, which is what fills
 * the GPU when a single frame does not.  d_image / h_image then hold the frames back to back
 * ([frame][comp][y][x]); every frame gets its own codestream from ojphgpu_encoder_finish_frame. */
int  ojphgpu_encoder_create_batch(const ojphgpu_plan* plan, int device, void* stream,
                                  uint32_t num_frames, ojphgpu_encoder** out);
int  ojphgpu_encoder_finish_frame(ojphgpu_encoder* enc, uint32_t frame, uint8_t* h_out, size_t cap,
                                  size_t* out_len);
/* device part only: d_image (int32 planes, resident in HBM) -> coded block bytes in HBM.
 * What a run leaves (all ojphgpu_encoder_run_device*): on return, in the order of the encoder's stream, the frame HAS BEEN
 * CONSUMED -- work enqueued on that stream afterwards may overwrite or free d_image -- and that is all the stream's order
 * says.  The products of the run (coded bytes, block lengths, cursors, the coefficient planes) live in the object's own
 * buffers and are reached only through the object's calls (_coded_bytes, _finish*, the timing getters, the next run,
 * _destroy, the setters of section 5b / 5c), each of which waits for them.  A plain run of a single-frame encoder with at
 * least two decompositions, into its own buffers and with per-launch timing off (ojphgpu_encoder_set_timing(enc, 0)), is
 * RELEASED: everything behind the last launch that reads d_image -- the top resolution's blocks, the lower transform
 * levels, the other blocks -- runs on two streams of the object's own and the caller's stream does not wait for it, so
 * the caller's next job on that stream starts beside the block coder.  Every other run (per-launch timing on, which is
 * the default; a byte budget or a quality target; a frame batch; the encoder of a frame pipe, a transcoder or a recoder;
 * OJPHGPU_NO_OVERLAP=1 or OJPHGPU_ENC_RELEASE=0 in the environment at creation) ends joined on the caller's stream.
 * The bytes are the same either way.
 * Consecutive released runs: an encoder that can release holds what a run produces -- coefficient planes, output buffer,
 * block results, cursors -- TWICE, and every released run takes the set the run before it did not use.  The next run no
 * longer waits for the previous one: its first transform level starts while the previous run's block coder is still
 * running, and on the caller's stream it waits only for the run two back.  The object's other calls (_coded_bytes,
 * _finish*, the timing getters, the setters of section 5b / 5c, a run that ends joined) wait for every run in flight and
 * then read the products of the LAST run.  A released run cuts the top resolution's blocks between its two streams at
 * OJPHGPU_ENC_TOP_SHARE_RELEASED percent (default 10 where the top resolution has more than 8192 blocks, else 50), a joined one where OJPHGPU_ENC_TOP_SHARE or the model says;
 * ojphgpu_encoder_ht_timing reports the cut of the last run.  Memory: the second set is one more arena, output buffer and
 * results table per such encoder -- about 0.7 GB for an 8K 4:4:4 frame; OJPHGPU_ENC_SETS=1 in the environment at
 * creation keeps one set (every run then waits for the one before it, as it did), and an encoder that can never release
 * holds one.  OJPHGPU_ENC_SIDE_CLEAR=0 keeps the cursor clear of a released run on the caller's stream.
 * Stream capture: a joined run is a fork and a join on the caller's stream and can be captured as it is; a released run
 * leaves two forked streams unjoined, and the next released run of the same object no longer joins them (it waits for the
 * run two back only).  A capture that holds released runs must therefore end with one of the calls that wait for every
 * run in flight and stay on the stream -- a run with per-launch timing on is the one that neither synchronises the host
 * nor is refused in a capture -- or the object runs with per-launch timing on (or OJPHGPU_ENC_RELEASE=0) throughout.
 * Two caller streams: a caller that drives encodes and decodes on two streams of its own keeps a decode of its own
 * priority waiting at all times and starves the low-priority branches of a released run; INTEGRATION.md section 5. */
int  ojphgpu_encoder_run_device(ojphgpu_encoder* enc, const int32_t* d_image);
/* diagnostic (tests, tools; not needed to use the object): *pending = 1 while a released run of the object has not been
 * waited for by one of the calls above, else 0 */
int  ojphgpu_encoder_is_pending(const ojphgpu_encoder* enc, int* pending);
/* the frame in 16-bit containers (same plane layout, 2-byte elements; int16 for signed components,
 * uint16 otherwise; every component at most 16 bits deep) */
int  ojphgpu_encoder_run_device16(ojphgpu_encoder* enc, const uint16_t* d_image);
/* 8-bit containers (int8 for signed components, uint8 otherwise; every component at most 8 bits deep): how 8-bit
 * frames exist in files and capture buffers -- a quarter of the upload of int32 samples */
int  ojphgpu_encoder_run_device8(ojphgpu_encoder* enc, const uint8_t* d_image);
int  ojphgpu_encode16(ojphgpu_encoder* enc, const uint16_t* h_image, uint8_t* h_out, size_t cap, size_t* out_len);
/* D2H of block bytes + lengths, then host Tier-2 -> complete codestream */
int  ojphgpu_encoder_finish(ojphgpu_encoder* enc, uint8_t* h_out, size_t cap, size_t* out_len);
/* convenience: H2D + run_device + finish */
int  ojphgpu_encode(ojphgpu_encoder* enc, const int32_t* h_image, uint8_t* h_out, size_t cap,
                    size_t* out_len);
/* total coded bytes produced by the last run_device (synchronises the stream) */
int  ojphgpu_encoder_coded_bytes(ojphgpu_encoder* enc, uint64_t* bytes);

/* plan must come from ojphgpu_t2_parse over (h_codestream, len) */
int  ojphgpu_decoder_create(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_decoder** out);
/* decodes only tiles [tile_first, tile_first + tile_count): writes their region of d_image */
int  ojphgpu_decoder_create_tiles(const ojphgpu_plan* plan, int device, void* stream,
                                  uint32_t tile_first, uint32_t tile_count, ojphgpu_decoder** out);
/* a decoder for a batch: plans[f] = ojphgpu_t2_parse of frame f's codestream; all frames must have
 * the same geometry.  Upload every frame's bytes with ojphgpu_decoder_upload_frame, then
 * ojphgpu_decoder_run_device writes d_image = [frame][comp][y][x]. */
int  ojphgpu_decoder_create_batch(const ojphgpu_plan* const* plans, uint32_t num_frames, int device,
                                  void* stream, ojphgpu_decoder** out);
int  ojphgpu_decoder_upload_frame(ojphgpu_decoder* dec, uint32_t frame, const uint8_t* h_codestream,
                                  size_t len);
void ojphgpu_decoder_destroy(ojphgpu_decoder* dec);
/* H2D of the codestream bytes */
int  ojphgpu_decoder_upload(ojphgpu_decoder* dec, const uint8_t* h_codestream, size_t len);
/* device part only: coded bytes in HBM -> d_image (int32 planes).
 * What a run orders (all ojphgpu_decoder_run_device*): d_image is WRITTEN IN THE ORDER OF THE DECODER'S STREAM -- only the
 * top synthesis level (and a stand-alone conversion) touches it, and they are enqueued on that stream; work enqueued there
 * before the call is complete before the first sample lands, work enqueued behind it sees the whole frame.  A plain run of
 * a single-frame decoder made by ojphgpu_decoder_create (or _create_tiles over all tiles) whose block decoder is the one
 * launch (blocks at most 64 wide and 64 rows tall, no refinement passes, at least two decompositions), whole frames, with
 * per-launch timing off (ojphgpu_decoder_set_timing(dec, 0)), is RELEASED: the block decoder -- which reads the object's
 * codestream bytes and descriptors and writes its own coefficient planes, records and status, nothing of the caller's --
 * runs on a stream of the object's own.  There it is ordered behind the object's last upload and behind the last
 * synthesis that read the planes it writes, NOT behind the caller's stream: it starts beside whatever that stream still
 * holds (the synthesis of the run before, an encode's first transform level).  The caller's stream waits for it in front
 * of the synthesis levels, which stay on the caller's stream (OJPHGPU_DEC_AHEAD_LEVELS=1 at creation: levels L..2 follow
 * the block decoder on the own stream and the caller's stream waits in front of the top level; measured slower).  An
 * object that can release takes its uploads (ojphgpu_decoder_upload*) on the same own stream and makes the caller's stream
 * wait for them: a caller that synchronises its stream may reuse the host buffer as before, and a fresh decoder on a busy
 * stream gets its upload and block decoder beside the work already queued.  It holds its coefficient planes TWICE
 * (released runs alternate; the block decoder of run n + 1 waits for the synthesis of run n - 1 only: + 0.4 GB at 8K
 * 4:4:4); OJPHGPU_DEC_SETS=1 in the environment at creation keeps one (it then waits for run n).
 * Every other run (per-launch timing on, which is the default; a batch; a region; a tile range; a frame with one
 * decomposition; the separate launches; the decoders of pipes, transcoders, recoders and multi-device decoders;
 * OJPHGPU_NO_OVERLAP=1 or OJPHGPU_DEC_RELEASE=0 at creation) is enqueued on the caller's stream as before, behind every
 * released run of the object.  What settles a released run (makes the caller's stream wait for everything the own stream
 * holds, without a host synchronisation, before it reads status or planes): ojphgpu_decoder_failed_blocks, the timing
 * getters, ojphgpu_decoder_set_timing, ojphgpu_decoder_giveup_epoch (which also drains the own stream), a run of the other
 * schedule; ojphgpu_decoder_destroy drains the own stream.  The samples are the same either way.
 * OJPHGPU_DEC_AHEAD_PRIO=high|normal|low: priority of the own stream (default high, as the side stream always was); read
 * at creation.  Stream capture: a released run forks to the own stream and joins it again inside the call, but waits there
 * for events of earlier runs and uploads; capture runs with per-launch timing on or under OJPHGPU_DEC_RELEASE=0. */
int  ojphgpu_decoder_run_device(ojphgpu_decoder* dec, int32_t* d_image);
/* diagnostic (tests, tools): *pending = 1 while a released run of the object has not been settled by one of the calls above */
int  ojphgpu_decoder_pending(const ojphgpu_decoder* dec, int* pending);
int  ojphgpu_decoder_run_device16(ojphgpu_decoder* dec, uint16_t* d_image);     /* 16-bit containers */
int  ojphgpu_decoder_run_device8(ojphgpu_decoder* dec, uint8_t* d_image);       /* 8-bit containers */
int  ojphgpu_decode16(ojphgpu_decoder* dec, const uint8_t* h_codestream, size_t len, uint16_t* h_image);
/* number of code-blocks that failed to decode in the last run (synchronises).  This call COLLECTS the run: when the
 * one-launch block decoder of that run gave up waiting for its own step-1 part (a chip held up for seconds by other
 * work; it marks the run instead of failing blocks), the frame is decoded again here through the separate launches,
 * into the same d_image -- so read d_image after this call, not before.  The reference decides per block at
 * codeblock::decode (ojph_codeblock.cpp:190-224); this is where its verdicts become visible.
 * A caller that consumes d_image on the device and never collects is told by a LATER ojphgpu_decoder_run_device* call,
 * which returns OJPHGPU_E_UNCOLLECTED (once per give-up, nothing enqueued) when a run before it had asked for the repeat.
 * The launch only says so when its wait has run out (about two seconds), so the notice may come more than one call
 * after the run it is about. */
int  ojphgpu_decoder_failed_blocks(ojphgpu_decoder* dec, uint32_t* count);
/* how many runs of this decoder were repeated that way (0 in any normal process) */
int  ojphgpu_decoder_fused_retries(ojphgpu_decoder* dec, uint32_t* count);
/* out[0] = code-blocks decoded per frame, out[1] = blocks of the plan, out[2] = codestream bytes uploaded per frame (the
 * first frame), out[3] = tiles touched.  A region decoder (ojphgpu_plan_restrict_region) uploads only the bytes of the
 * blocks it decodes, runs of them that are adjacent in the codestream gathered in one pinned buffer and copied at once; its
 * upload waits (on the host) until the copy of the previous upload has left that buffer, not for the decoder's runs. */
int  ojphgpu_decoder_region_info(ojphgpu_decoder* dec, uint64_t out[4]);
/* synchronises the decoder's stream; *current = the number of one-launch (fused) block-decoder runs enqueued so far,
 * *last_giveup = the number of the newest of them whose wait ran out (0 = none ever did).  A caller that times or pipelines
 * uncollected runs brackets them with two calls: no run in between gave up iff last_giveup <= the first call's *current. */
int  ojphgpu_decoder_giveup_epoch(ojphgpu_decoder* dec, uint32_t* last_giveup, uint32_t* current);
int  ojphgpu_decode(ojphgpu_decoder* dec, const uint8_t* h_codestream, size_t len,
                    int32_t* h_image);

/* timing of the last run_device, in milliseconds, measured with HIP events on the codec's own
 * stream: out[0]=convert+colour [1]=DWT [2]=HT block coder [3]=total */
/* per_launch = 1 (default): every launch is bracketed by HIP events so that the per-stage sums below
 * are available; 0: only the wall time of the run is recorded (out[3]), the other entries read 0 --
 * the event pairs cost a few microseconds each, which shows at these kernel durations.  An encoder's run with 0 may be
 * released (see ojphgpu_encoder_run_device); its total ends with the later of its two branches */
int  ojphgpu_encoder_set_timing(ojphgpu_encoder* enc, int per_launch);
int  ojphgpu_decoder_set_timing(ojphgpu_decoder* dec, int per_launch);
int  ojphgpu_encoder_timing(ojphgpu_encoder* enc, float out[4]);
int  ojphgpu_decoder_timing(ojphgpu_decoder* dec, float out[4]);
/* the block decoder's three launches of the last run_device: out[0]=prep [1]=step 1 [2]=step 2 (ms) */
int  ojphgpu_decoder_ht_timing(ojphgpu_decoder* dec, float out[3]);
/* the block encoder's launches of the last run_device, in issue order: when the top resolution's
 * blocks are coded on the side stream (single frames with >= 2 decompositions) there are two --
 * [0] = those blocks (*n_top of them, concurrent with the lower DWT levels), [1] = the rest */
int  ojphgpu_encoder_ht_timing(ojphgpu_encoder* enc, float* out, uint32_t cap, uint32_t* n, uint32_t* n_top);
/* duration (ms) of every DWT level launch of the last run_device, in launch order (encode:
 * highest resolution first; decode: lowest first); *n = number of levels written */
int  ojphgpu_encoder_level_timing(ojphgpu_encoder* enc, float* out, uint32_t cap, uint32_t* n);
int  ojphgpu_decoder_level_timing(ojphgpu_decoder* dec, float* out, uint32_t cap, uint32_t* n);

/* ------------------------------------------------------------------------------------------ *
 * 5b. Encoding to a byte budget.  The reference has no rate control for HTJ2K: the size of an irreversible codestream
 *    follows from the base step handed to param_qcd::set_irrev_quant, which scales it per sub-band and writes it with
 *    encode_SPqcd (ojph_params.cpp:1542-1612).  What is added here searches that one number: a fixed grid of
 *    OJPHGPU_RATE_GRID base steps, qstep(j) = (float) exp2(-1 - j / 16) evaluated in double and rounded once -- j = 0 the
 *    coarsest (0.5), j = 240 the finest (2^-16) -- and size(j) = the length, SOC to EOC, of the codestream the encoder
 *    writes for its plan's parameters with qstep = qstep(j).  A budgeted encode with max_bytes = B returns an index j* and
 *    the codestream of j* with size(j*) <= B and either j* == 240 or size(j* + 1) > B (the certificate); the bytes are
 *    exactly those of a plain encode at qstep(j*), QCD / QCC included, so decoders need nothing new.  size(0) > B:
 *    OJPHGPU_E_BUDGET, nothing written.
 * ------------------------------------------------------------------------------------------ */
#define OJPHGPU_RATE_GRID 241
int  ojphgpu_rate_grid_qstep(uint32_t j, float* qstep);            /* OJPHGPU_E_INVALID: j >= OJPHGPU_RATE_GRID */

typedef int64_t (*ojphgpu_size_fn)(void* user, uint32_t grid_index);   /* size(j); < 0 = error */
typedef struct ojphgpu_rate_info {
  uint32_t grid_index; float qstep; uint64_t bytes;      /* j*, qstep(j*), size(j*)               */
  uint64_t bytes_finer;                                  /* size(j* + 1), 0 when j* == 240        */
  uint32_t passes, first_guess;                          /* calls of size_fn; the model's first j */
} ojphgpu_rate_info;
/* The search, host only: hist = the band statistics of the frame, [bands of the plan][OJPHGPU_STATS_BINS] in band order
 * (NULL: no model, plain interval halving).  A model predicts size(j) from the histograms and every band's step at j; the
 * first trial is its index for the budget, and after every trial it is rescaled by observed / predicted before it proposes
 * the next.  Correctness does not rest on it: every trial shrinks the interval of candidates, a proposal outside the
 * interval is moved inside, and once six trials have produced no certificate the proposals are the interval's midpoint.
 * No index is asked twice, and passes <= 16 for every input -- fn need not be monotone.  The plan must be irreversible
 * throughout, without quality factors.  Returns OJPHGPU_E_BUDGET (out->passes, first_guess filled) when size(0) >
 * max_bytes, a negative value of fn as it is. */
int  ojphgpu_rate_search(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes,
                         ojphgpu_size_fn fn, void* user, ojphgpu_rate_info* out);
/* The same search started from a guess, for the frames of a sequence (hint = the previous frame's j*): the first trial is
 * `hint`, the second the neighbour its result points to (hint + 1 when it fit, hint - 1 when not) and, when that one points
 * the same way, the third the index beyond it -- each only where the index exists and the certificate is not complete --
 * so hint == j* takes the two trials the certificate consists of and hint == j* +- 1 at most three.  Where these have
 * not produced the certificate the search above goes on inside the interval they left, its model rescaled by the last
 * of them.  The hinted trials count among the six model-led ones: no index asked twice, passes <= 16.  out->first_guess
 * = hint.  hint = -1: no hint, exactly ojphgpu_rate_search; any other value outside 0 .. OJPHGPU_RATE_GRID - 1:
 * OJPHGPU_E_INVALID.  hist may be NULL (the hinted trials, then halving). */
int  ojphgpu_rate_search_hint(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, int32_t hint,
                              ojphgpu_size_fn fn, void* user, ojphgpu_rate_info* out);
/* The same search in steps, for callers whose measurements are shared (the rounds below advance one per frame over
 * common launches): _next hands out the index to measure -- 1: measure size(*j) and _feed it; 0: certified, _info holds
 * the answer; OJPHGPU_E_BUDGET: size(0) > max_bytes (_info: passes, first_guess) -- and _feed takes the size of the index
 * _next handed out; a size < 0 ends the stepper and comes back as it is.  ojphgpu_rate_search_hint is a loop over this:
 * the indices asked, passes, first_guess, the result and the codes are the same.  hist / hint as there; the histograms
 * are read by _create only.  OJPHGPU_E_INVALID: _next after the end or with an index still out, _feed without a _next. */
typedef struct ojphgpu_rate_stepper ojphgpu_rate_stepper;
int  ojphgpu_rate_stepper_create(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, int32_t hint,
                                 ojphgpu_rate_stepper** out);
int  ojphgpu_rate_stepper_next(ojphgpu_rate_stepper* st, uint32_t* j);
int  ojphgpu_rate_stepper_feed(ojphgpu_rate_stepper* st, int64_t size);
int  ojphgpu_rate_stepper_info(const ojphgpu_rate_stepper* st, ojphgpu_rate_info* out);
void ojphgpu_rate_stepper_destroy(ojphgpu_rate_stepper* st);
/* The stepper under a ceiling (the capped mode of section 5c): ceil_index in 1 .. 240 is an index the caller has measured
 * already, with size(ceil_index) = ceil_size > max_bytes.  The stepper starts with that as its upper end: it never hands
 * out an index >= ceil_index, a hint >= ceil_index is moved to ceil_index - 1, ceil_size is reported as bytes_finer when
 * j* == ceil_index - 1, and the model (if any) is scaled by ceil_size before its first proposal.  passes counts the
 * stepper's own trials only; passes <= 16 and no index twice, as above.  ceil_index == OJPHGPU_RATE_GRID: no ceiling,
 * exactly ojphgpu_rate_stepper_create (ceil_size is not read).  OJPHGPU_E_INVALID: ceil_index == 0 or beyond the grid's
 * size, under a ceiling a ceil_size <= max_bytes or above INT64_MAX, and what _create refuses. */
int  ojphgpu_rate_stepper_create_under(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, int32_t hint,
                                       uint32_t ceil_index, uint64_t ceil_size, ojphgpu_rate_stepper** out);
/* The searches of the `frames` frames of one encoder run, advanced together in ROUNDS over shared measurements, host only:
 * what ojphgpu_encoder_finish* drives for any frame count, for callers and tests that bring sizes of their own.  A stepper
 * per frame: hist = [frames][bands of the plan][OJPHGPU_STATS_BINS] (NULL: no model), max_bytes[frames], one hint for all.
 * _next -- 1: a round; code EVERY frame f at idx[f] -- an open frame's the index its stepper hands out, a certified frame's
 * its j*, a frame nothing fits index 0 -- and _feed sizes[f] = size(idx[f]) of the frames with measures[f] != 0 (1: a trial
 * of the frame's search; 2: j* coded once more because the frame's last trial was not j*, counted in its passes; the size
 * must be the one measured before, anything else is OJPHGPU_E_HIP); sizes of the other frames are not read.  0: the end
 * -- nobody measures and every frame was coded at its index in the last round.  A size < 0 ends the search and comes back
 * as it is, as does a stepper's error.  _frame: a closed frame's verdict, OJPHGPU_OK or OJPHGPU_E_BUDGET (info: passes,
 * first_guess), and what ojphgpu_rate_search_hint would report for it -- the same indices in the same order, passes one
 * higher exactly when its j* was coded once more; OJPHGPU_E_INVALID while the frame is open or after the search failed.
 * _count: rounds handed out so far; one frame: its passes.  At most 17 rounds.  OJPHGPU_E_INVALID: what
 * ojphgpu_rate_stepper_create refuses, frames == 0; _next after the end or with a round still out, _feed without one. */
typedef struct ojphgpu_rate_rounds ojphgpu_rate_rounds;
int  ojphgpu_rate_rounds_create(const ojphgpu_plan* plan, const uint32_t* hist, const uint64_t* max_bytes, uint32_t frames,
                                int32_t hint, ojphgpu_rate_rounds** out);
int  ojphgpu_rate_rounds_next(ojphgpu_rate_rounds* r, uint32_t* idx, uint8_t* measures);      /* idx[frames], measures[frames] */
int  ojphgpu_rate_rounds_feed(ojphgpu_rate_rounds* r, const int64_t* sizes);                  /* sizes[frames] */
int  ojphgpu_rate_rounds_frame(const ojphgpu_rate_rounds* r, uint32_t frame, ojphgpu_rate_info* info);
int  ojphgpu_rate_rounds_count(const ojphgpu_rate_rounds* r, uint32_t* rounds);
void ojphgpu_rate_rounds_destroy(ojphgpu_rate_rounds* r);
/* the model alone: predicted bytes of every grid index, out[OJPHGPU_RATE_GRID] (what tools/rate_bench.py reports) */
int  ojphgpu_rate_predict(const ojphgpu_plan* plan, const uint32_t* hist, double* out);

/* max_bytes > 0: the encoder codes every following frame to that budget; 0 switches it off (every call then behaves as
 * without this section).  With a budget, ojphgpu_encoder_run_device* enqueues conversion, DWT and the band statistics;
 * ojphgpu_encoder_finish* runs the search -- per trial the block coder's launches with the blocks' delta / K_max of
 * qstep(j), the block lengths come to the host and the Tier-2 layout gives size(j) -- and downloads the coded bytes
 * once, for j*.  OJPHGPU_E_BUDGET leaves the encoder usable.  OJPHGPU_E_INVALID: a plan with a reversible component (COC
 * included), a quality factor (global or per component), ATK / DFS wavelets, a band of 2^32 samples or more; an encoder
 * of a tile range that does not cover the frame; a batch encoder -- ON PURPOSE, also for equal budgets: the batch form is
 * the array call below, and callers rely on this refusal.  The per-block scratch slots and the output buffer are
 * re-sized for the finest step of the grid on the first call. */
int  ojphgpu_encoder_set_budget(ojphgpu_encoder* enc, uint64_t max_bytes);
/* What the budgeted ojphgpu_encoder_finish* of the LAST run found, frame 0 of _rate_info_frame below; after
 * OJPHGPU_E_BUDGET: OJPHGPU_OK with passes and first_guess.  OJPHGPU_E_INVALID: before the first budgeted finish; between a
 * ojphgpu_encoder_run_device* and its finish (the run has not been searched: the previous run's answer is not handed out);
 * with the budget switched off or a quality target set; after a search that ended with an error of its own. */
int  ojphgpu_encoder_rate_info(ojphgpu_encoder* enc, ojphgpu_rate_info* info);
/* A batch encoder (ojphgpu_encoder_create_batch) codes frame f of every following run to max_bytes[f]; n must be the
 * encoder's frame count (a single-frame encoder: n == 1, exactly ojphgpu_encoder_set_budget).  All zeros switches the
 * budgets off as set_budget(0) does; a zero among non-zero values is OJPHGPU_E_INVALID, and so is everything set_budget
 * refuses except "a batch encoder", and a batch whose output bound at the finest step of the grid does not fit the 32-bit
 * byte cursor (code fewer frames per batch).  ojphgpu_encoder_run_device* enqueues conversion, DWT and the statistics
 * of every frame.  The first ojphgpu_encoder_finish_frame of a run searches all frames together, in ROUNDS: one launch
 * sets every frame's step -- an open frame's the index its stepper hands out, a certified frame's its j*, a frame nothing
 * fits index 0 -- the block coder runs over the blocks of all frames, the lengths come back once and every open frame's
 * layout feeds its stepper; the rounds end when every frame was coded at its answer in the last one, and the bytes are
 * downloaded once.  finish_frame(f) then writes frame f: byte for byte the single-frame budgeted encode of that frame at
 * max_bytes[f].  A frame with size(0) > max_bytes[f] gets OJPHGPU_E_BUDGET from its own finish_frame only; the others
 * are written, and the encoder stays usable.  _rate_info_frame answers as the single encoder's _rate_info would for that
 * frame and budget (passes: the frame's own trials, plus one when the last of them was not j*) and is refused where
 * _rate_info is; _rate_rounds gives the rounds of the last search (ojphgpu_rate_rounds above is its loop, for one frame
 * and for many; a single-frame encoder: rounds == passes). */
int  ojphgpu_encoder_set_budgets(ojphgpu_encoder* enc, const uint64_t* max_bytes, uint32_t n);
int  ojphgpu_encoder_rate_info_frame(ojphgpu_encoder* enc, uint32_t frame, ojphgpu_rate_info* info);
int  ojphgpu_encoder_rate_rounds(ojphgpu_encoder* enc, uint32_t* rounds);
/* host clock of the last budgeted finish, ms: out[0] the search (every pass), [1] the part of it spent waiting for the
 * device and the copies of the block lengths, [2] the download and Tier-2 of j*; out[3] the band statistics kernel of the
 * run before it (device events; needs ojphgpu_encoder_set_timing's per-launch spans, the default) */
int  ojphgpu_encoder_rate_timing(ojphgpu_encoder* enc, float out[4]);

/* ------------------------------------------------------------------------------------------ *
 * 5f. A reversible frame under a byte cap: lossless where the frame fits, the nearest thing to it where it does not, in a
 *    codestream every 5/3 decoder reads.  Section 5b refuses reversible components -- there is no step to search.  What is
 *    searched here is how many of its lowest magnitude bit-planes each sub-band drops: a block of band b that drops t_b
 *    planes is coded at p = 30 - missing_msbs with missing_msbs = K_max(b) - 1 - t_b, the packet header says so, and a
 *    decoder puts the half bit below the kept planes (the reference's decoder reads such blocks; its encoder never writes
 *    them).  QCD / SIZ / COD are those of the plain encode.
 *
 *    The ladder.  A TABLE gives every band of the plan its t_b, 0 <= t_b <= K_max(b) - 1; a LEVEL j = 0 .. J - 1 names one:
 *      w_b    = log2(g_h g_v g_c), g_h / g_v the L2 norms of the 1-D 5/3 synthesis basis vector of the band's branch (low
 *               or high) at its decomposition depth -- a unit impulse taken through the linear inverse lifting, in double,
 *               away from the borders -- and g_c the L2 norm of the component's column of the inverse colour transform:
 *               with the RCT sqrt(3) for component 0, sqrt(11/16) for components 1 and 2, else 1;
 *      q_b    = floor(4 (w_b - min_b w_b) + 0.5), quarter planes;
 *      t_b(j) = clamp(floor((j + 3 - q_b) / 4), 0, K_max(b) - 1);      J = max_b(4 (K_max(b) - 1) + q_b) - 3 + 1.
 *    Level 0 is lossless and byte for byte the plain encode, level 1 drops one plane of the band(s) of lowest weight, level
 *    J - 1 leaves every band its top plane only.  Neighbouring levels may share a table (and then a size).  A block none of
 *    whose samples reaches 2^t_b is not coded (length 0).  size(j) = the length, SOC to EOC, of the codestream at level j.
 *    A capped encode with max_bytes = B returns the level j* with size(j*) <= B and (j* == 0 or size(j* - 1) > B), both
 *    measured; size(J - 1) > B: OJPHGPU_E_BUDGET.  Whole planes are coarse: neighbouring distinct sizes differ by tens of
 *    per cent, not by the 1-2 % of the grid of section 5b.
 *    Plans: reversible Part-1 5/3 in every component (COC included) with one number of decompositions, no ATK / DFS, no
 *    component on the 64-bit sample path; anything else is OJPHGPU_E_INVALID from every call of this section.
 * ------------------------------------------------------------------------------------------ */
int  ojphgpu_plan_trunc_levels(const ojphgpu_plan* plan, uint32_t* levels);           /* J */
int  ojphgpu_plan_trunc_weights(const ojphgpu_plan* plan, int32_t* q);                /* q[bands of the plan] */
int  ojphgpu_plan_trunc_table(const ojphgpu_plan* plan, uint32_t j, uint8_t* t);      /* t[bands]; j >= J: OJPHGPU_E_INVALID */
typedef struct ojphgpu_trunc_info {
  uint32_t level;                                        /* j*                                                  */
  uint32_t passes, first_guess;                          /* calls of size_fn; the level of the second of them -- the
                                                            model's guess -- or 0 when level 0 was the only one  */
  uint32_t max_dropped;                                  /* the largest t_b of level j*                         */
  uint32_t lossless;                                     /* j* == 0: the codestream is the plain encode's       */
  uint32_t reserved;
  uint64_t bytes, bytes_finer;                           /* size(j*); size(j* - 1), 0 when j* == 0              */
} ojphgpu_trunc_info;
/* The search, host only: hist = the integer band statistics of the frame (ojphgpu_band_stats_int), [bands of the plan]
 * [OJPHGPU_STATS_BINS] in band order, or NULL.  fn(user, j) = size(j).  Levels that share a table are one measurement:
 * only the first level of such a run is ever asked, and j* is one of those.  The first trial is level 0: the frame that
 * fits -- what the mode is for -- takes one pass.  With hist a model (a coefficient of bit length L > t_b costs about
 * L - t_b + 3 bits, the constants of section 5b's model, rescaled by observed / predicted after every trial, the first of
 * them included) leads the second trial.  Then the interval between a level measured not to fit and one measured to fit is
 * halved.  Correctness never rests on the
 * model or on fn being monotone: the certificate is two measurements.  passes <= 2 + ceil(log2 J) for every fn.
 * OJPHGPU_E_BUDGET (info: passes, first_guess) when the last level does not fit; a negative value of fn as it is. */
int  ojphgpu_trunc_search(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, ojphgpu_size_fn fn, void* user,
                          ojphgpu_trunc_info* info);
/* max_bytes > 0: the encoder codes every following frame under that cap; 0 switches the mode off.  ojphgpu_encoder_run_device*
 * then enqueues conversion, DWT and the integer band statistics; ojphgpu_encoder_finish runs the search -- per trial the
 * table goes into the block descriptors, the block coder runs, the block lengths come to the host and the Tier-2 layout
 * gives size(j) -- and writes the codestream of j*.  OJPHGPU_E_BUDGET leaves the encoder usable.  The scratch slots and
 * the output of the plain plan hold every level.  _set_trunc_level: a fixed level instead (no search, no statistics);
 * j < 0 switches it off, j >= J is OJPHGPU_E_INVALID.  The two replace each other.  Tiled frames: the cap is the whole
 * codestream's.  OJPHGPU_E_INVALID, encoder unchanged: a plan this section refuses (above); a batch encoder; an encoder of
 * a tile range that does not cover the frame; together with ojphgpu_encoder_set_budget(s) / _set_quality*.  In this mode
 * ojphgpu_encoder_finish_tiles* are refused.  _trunc_info: what the last finish found (a fixed level: that level, passes 1,
 * bytes_finer 0); OJPHGPU_E_INVALID before the first finish of the mode. */
int  ojphgpu_encoder_set_truncation(ojphgpu_encoder* enc, uint64_t max_bytes);
int  ojphgpu_encoder_set_trunc_level(ojphgpu_encoder* enc, int32_t j);
int  ojphgpu_encoder_trunc_info(ojphgpu_encoder* enc, ojphgpu_trunc_info* info);
/* after such a finish, ms: out[0] host clock of the coding inside it (every trial, and j* once more when the last trial was
 * another level); out[1] the integer statistics kernel of the run before it (device events; needs
 * ojphgpu_encoder_set_timing's per-launch spans), 0 at a fixed level */
int  ojphgpu_encoder_trunc_timing(ojphgpu_encoder* enc, float out[2]);

/* ------------------------------------------------------------------------------------------ *
 * 5g. Near-lossless coding of a reversible frame, the host side: the other half of section 5f's rate control -- the
 *    smallest codestream of the ladder whose decode stays within an error bound.  What is here is the contract and the
 *    search; the encoder mode that would measure the levels on the device is not built yet.
 *
 *    u[0] = 0 < u[1] < ... < u[U - 1]: the levels of section 5f whose table differs from the level before.  SSE(j) / PAE(j):
 *    the exact sum of squared differences / the largest absolute difference between the caller's frame and the int32 frame
 *    ojphgpu_decoder_run_device returns for the codestream of level j (ojphgpu_encoder_set_trunc_level(j)), over every
 *    component on its own grid.  A target is max_sse = T and / or max_pae = E; UINT64_MAX / UINT32_MAX: no bound; both
 *    unbounded: OJPHGPU_E_INVALID.  A level MEETS when SSE(j) <= T and PAE(j) <= E.  The result is an index k*, u[k*] the
 *    level to code -- at k* = 0 the plain lossless encode.  The certificate: u[k*] meets (measured; level 0 meets by the
 *    reversible path's own contract and is never measured), and k* == U - 1 or u[k* + 1] is measured not to meet.  Neither
 *    figure is monotone over the ladder: any index with the certificate is an answer, and nothing is assumed between two
 *    measured levels.  There is no failure code: level 0 always meets, and T = 0 or E = 0 gives it without a trial (then no
 *    coarser neighbour is measured either).
 *
 *    No block needs coding to measure a level: the planes truncated per band -- magnitude m -> 0 where m >> t == 0, else
 *    (m >> t << t) | 1 << (t - 1), sign kept -- and taken through the decoder's synthesis ARE the decode of the codestream
 *    of that table, sample for sample (tests/test_cpu_near_lossless.py, against the reference's decode).
 *    Plans: those of section 5f, and no component deeper than 16 bits (ojphgpu_frame_error's sum bound).
 * ------------------------------------------------------------------------------------------ */
typedef struct ojphgpu_near_lossless_info {
  uint32_t level;                                        /* u[k*]                                               */
  uint32_t passes;                                       /* calls of err_fn                                     */
  uint32_t lossless;                                     /* k* == 0: the codestream is the plain encode's       */
  uint32_t max_dropped;                                  /* the largest t_b of that level                       */
  uint32_t pae, level_coarser, pae_coarser, reserved;    /* PAE(u[k*]) (0 at level 0); u[k* + 1] and its PAE --  */
  uint64_t sse, sse_coarser;                             /* SSE likewise -- the neighbour measured not to meet,
                                                            zeros when k* == U - 1 or nothing was measured       */
  uint64_t bytes;                                        /* the codestream's length: for the caller that codes
                                                            the level to fill; the search leaves 0               */
} ojphgpu_near_lossless_info;
typedef int (*ojphgpu_err_fn)(void* user, uint32_t level, uint64_t* sse, uint32_t* pae);   /* 0, or an error (returned as it is) */
/* The search, host only (no HIP call): lo = 0 (meets, unmeasured), hi = U (virtual, does not meet); u[lo + (hi - lo) / 2] is
 * measured and the end its verdict names moves there, until hi - lo == 1: k* = lo.  passes <= ceil(log2 U) for every
 * err_fn, no level is asked twice.  (A first guess led by the integer band statistics, as section 5f has one, is not made.) */
int  ojphgpu_near_lossless_search(const ojphgpu_plan* plan, uint64_t max_sse, uint32_t max_pae, ojphgpu_err_fn err_fn, void* user,
                                  ojphgpu_near_lossless_info* info);

/* ------------------------------------------------------------------------------------------ *
 * 5c. Encoding to a quality target: the other half of rate control.  Over the grid of section 5b, SSE(j) = the sum, over
 *    every component and every sample of it on its own grid, of (original - decoded)^2, where `decoded` is what
 *    ojphgpu_decoder_run_device returns (int32 samples: a sample the reference leaves one past its range stays there, where a
 *    narrower container would saturate) for the codestream the encoder writes at qstep(j); PAE(j) = the largest absolute
 *    difference.  Both are exact integers (the decoder is sample-exact against the reference).  An encode with max_sse = T
 *    returns an index j*, the codestream of j* -- byte for byte the plain encode at qstep(j*) -- and the certificate
 *    SSE(j*) <= T and (j* == 0 or SSE(j* - 1) > T), both sides measured: the coarsest step found to meet the target.  SSE
 *    is not monotone in j (it rises again in places on real frames) and the search does not assume it is: any index with
 *    the certificate is an answer.  SSE(240) > T: OJPHGPU_E_QUALITY, nothing written.
 *
 *    No block is coded for a trial.  The block coder is lossless over the quantised indices, so the decode of the
 *    codestream of step j is fixed by the unquantised planes the forward transform left in the arena and the band
 *    parameters of j: ojphgpu_band_requantise writes the planes the decoder would hold into a second arena, the decoder's
 *    own synthesis launches (a synthesis-only decoder object made from the encoder's plan) turn them into an int32 frame, and
 *    ojphgpu_frame_error_ex compares it with the caller's: 16 bytes per component come to the host.  j* is then block-coded
 *    once.  In a frame pipeline: ojphgpu_enc_pipe_set_quality (section 6).  Not available for batches, tile ranges or the
 *    multi-GPU encoder.
 * ------------------------------------------------------------------------------------------ */
typedef int64_t (*ojphgpu_sse_fn)(void* user, uint32_t grid_index, uint64_t* sse);   /* 0 and *sse = SSE(j); < 0 = error */
typedef struct ojphgpu_quality_info {
  uint32_t grid_index; float qstep;                      /* j*, qstep(j*)                                              */
  uint64_t sse, sse_coarser;                             /* SSE(j*); SSE(j* - 1), 0 when j* == 0                       */
  uint32_t pae, passes;                                  /* PAE(j*) (the encoder fills it); calls of the sse_fn        */
  uint64_t bytes;                                        /* the codestream's length (the encoder fills it)             */
} ojphgpu_quality_info;
/* The search, host only.  The first trial is j = 240 (not met: OJPHGPU_E_QUALITY, out->passes = 1), the second j = 0 (met:
 * the answer); from then on the interval between an index that fails (lo) and one that meets (hi) is halved until hi - lo
 * == 1, which is the certificate.  passes <= 10 and no index is asked twice, whatever fn returns.  A negative value of fn
 * is returned as it is. */
int  ojphgpu_quality_search(uint64_t max_sse, ojphgpu_sse_fn fn, void* user, ojphgpu_quality_info* out);
/* The same search started from a guess, for the frames of a sequence (hint = the previous frame's j*).  It keeps an index
 * measured to fail (lo; none at first) and one measured to meet (hi; none at first) and assumes nothing between two measured
 * indices.  The first trial is `hint`; then up to two neighbours on the side its result points to -- hint - 1, hint - 2
 * while they still meet, hint + 1, hint + 2 while they still fail -- stopping at the first that turns round, which is the
 * certificate.  While nothing has met, the next trial is 240 (OJPHGPU_E_QUALITY only on a measured SSE(240) > max_sse);
 * while nothing has failed and hi > 0, it is 0 (met: the answer); then (lo, hi) is halved until hi - lo == 1.  So an
 * unchanged answer costs the two trials of its certificate (one at index 0), passes <= 12 = 3 + 1 + ceil(log2(238)), and
 * no index is asked twice.  *first_guess = the first index tried.  hint = -1: no hint, the indices of ojphgpu_quality_search
 * in its order; any other value outside 0 .. OJPHGPU_RATE_GRID - 1: OJPHGPU_E_INVALID.  A negative value of fn is returned
 * as it is. */
int  ojphgpu_quality_search_hint(uint64_t max_sse, int32_t hint, ojphgpu_sse_fn fn, void* user, ojphgpu_quality_info* out,
                                 uint32_t* first_guess);

/* The encoder codes every following frame to max_sse (0 is a target like any other: the finest step at which nothing is
 * lost may exist); ojphgpu_encoder_clear_quality switches the mode off.  With a target, ojphgpu_encoder_run_device*
 * enqueues conversion and DWT and returns -- the caller's frame must stay valid and unchanged until ojphgpu_encoder_finish*
 * has returned, which runs the search against it, codes the blocks of j* and writes its codestream.  OJPHGPU_E_QUALITY
 * leaves the encoder usable (quality_info: passes).  OJPHGPU_E_INVALID: everything ojphgpu_encoder_set_budget refuses; a
 * component deeper than 16 bits; a band whose K_max at the finest step is above 30; a byte budget set at the same time
 * (and set_budget while a target is set); ojphgpu_encoder_finish_tiles*.  The first call re-sizes the scratch slots and
 * the output for the finest step and allocates the second arena and the reconstructed frame. */
int  ojphgpu_encoder_set_quality(ojphgpu_encoder* enc, uint64_t max_sse);
int  ojphgpu_encoder_clear_quality(ojphgpu_encoder* enc);
/* what the last finish with a target found (OJPHGPU_E_INVALID before one) */
int  ojphgpu_encoder_quality_info(ojphgpu_encoder* enc, ojphgpu_quality_info* info);
/* SSE and PAE of component `comp` at j* */
int  ojphgpu_encoder_quality_comp(ojphgpu_encoder* enc, uint32_t comp, uint64_t* sse, uint32_t* pae);
/* host clock of the last finish with a target, ms: out[0] the search (every trial), [1] the part of it spent waiting for
 * the device, [2] coding j*, its download and Tier-2 */
int  ojphgpu_encoder_quality_timing(ojphgpu_encoder* enc, float out[3]);

/* Under a byte cap: hold the quality target T = max_sse, but never exceed B = cap_bytes > 0.  A capped encode returns an
 * index j*, an outcome and the codestream of j*, byte for byte the plain encode at qstep(j*); every figure below is measured
 * for that frame.
 *   OJPHGPU_CAPPED_MET:       SSE(j*) <= T and (j* == 0 or SSE(j* - 1) > T) -- the quality certificate -- and size(j*) <= B.
 *   OJPHGPU_CAPPED_BY_BUDGET: size(j*) <= B and (j* == 240 or size(j* + 1) > B) -- the budget certificate of section 5b --
 *                             and a witness that the target does not fit: an index q > j* that carries the quality
 *                             certificate with size(q) > B (quality_index, quality_bytes), or a measured SSE(240) > T
 *                             (quality_index == OJPHGPU_RATE_GRID: no step of the grid meets the target).  SSE(j*) and
 *                             PAE(j*) are measured and reported whatever they are.
 * The cap wins: OJPHGPU_E_QUALITY is never returned in this mode.  size(0) > B: OJPHGPU_E_BUDGET, nothing written (the
 * passes are reported).  Neither SSE nor size is assumed monotone in j. */
#define OJPHGPU_CAPPED_MET        0
#define OJPHGPU_CAPPED_BY_BUDGET  1
typedef struct ojphgpu_capped_info {
  uint32_t grid_index; float qstep;                      /* j*, qstep(j*)                                                 */
  uint32_t outcome;                                      /* OJPHGPU_CAPPED_*                                              */
  uint32_t quality_index;                                /* q; OJPHGPU_RATE_GRID: none, SSE(240) > T was measured         */
  uint64_t quality_bytes;                                /* size(q); 0 when q was never coded                             */
  uint64_t bytes, bytes_finer;                           /* size(j*); BY_BUDGET: size(j* + 1), 0 when j* == 240; MET: 0   */
  uint64_t sse, sse_coarser;                             /* SSE(j*); MET: SSE(j* - 1), 0 when j* == 0; BY_BUDGET: 0       */
  uint32_t pae;                                          /* PAE(j*) (the encoder fills it)                                */
  uint32_t quality_passes, rate_passes;                  /* calls of the sse_fn; of the size_fn (the encoder: codings)    */
  uint32_t first_guess_q, first_guess_b;                 /* the first index each side tried (b: q when only q was coded)  */
  uint32_t reserved;
} ojphgpu_capped_info;
typedef const uint32_t* (*ojphgpu_hist_fn)(void* user);  /* the frame's band statistics as ojphgpu_rate_search reads them, or NULL */
/* The combined search, host only.  (1) ojphgpu_quality_search_hint(max_sse, hint_q): q, or "none" on a measured SSE(240) >
 * T.  (2) With a q: size_fn(q); it fits: MET.  (3) Otherwise hist_fn is called ONCE (it may return NULL: plain halving)
 * and the stepper of section 5b runs with hint_b -- under the ceiling q (ojphgpu_rate_stepper_create_under), or over the
 * whole grid when there is no q; q == 0 that does not fit is OJPHGPU_E_BUDGET at once.  (4) OJPHGPU_E_BUDGET comes back as
 * it is (info: the passes, the first guesses, quality_index / quality_bytes).  (5) SSE(j*) is the figure of the quality
 * trial of j* where one was made, else one more sse_fn call, counted.  quality_passes <= 12 + 1, rate_passes <= 1 + 16, no
 * index is asked twice by either callback; hist_fn is never called on MET.  hint_q / hint_b: -1 = none (the indices of
 * ojphgpu_quality_search; the model's guess).  A negative value of a callback ends the search and comes back as it is.
 * OJPHGPU_E_INVALID: cap_bytes == 0, a null callback, a hint outside -1 .. 240, a plan ojphgpu_rate_search refuses. */
int  ojphgpu_capped_search(const ojphgpu_plan* plan, uint64_t max_sse, uint64_t cap_bytes, int32_t hint_q, int32_t hint_b,
                           ojphgpu_sse_fn sse_fn, ojphgpu_size_fn size_fn, ojphgpu_hist_fn hist_fn, void* user,
                           ojphgpu_capped_info* info);
/* The encoder codes every following frame to max_sse under cap_bytes.  cap_bytes == 0: exactly ojphgpu_encoder_set_quality;
 * ojphgpu_encoder_clear_quality switches the mode off.  Refused where set_quality is refused (batches, tile ranges,
 * components deeper than 16 bits, a byte budget set, ojphgpu_encoder_finish_tiles*).  ojphgpu_encoder_run_device* enqueues
 * conversion and DWT only, as with a target alone; ojphgpu_encoder_finish* runs ojphgpu_capped_search -- a quality trial as
 * in section 5c, a size trial as in section 5b -- and launches the band statistics only when the cap binds (the
 * unquantised planes are still in the arena).  When the last coding of the search was not j*, j* is coded once more and
 * counted in rate_passes.  OJPHGPU_E_BUDGET leaves the encoder usable (capped_info: the passes).  While a cap is set,
 * ojphgpu_encoder_quality_info and ojphgpu_encoder_rate_info return OJPHGPU_E_INVALID; ojphgpu_encoder_quality_comp answers
 * for j*. */
int  ojphgpu_encoder_set_quality_capped(ojphgpu_encoder* enc, uint64_t max_sse, uint64_t cap_bytes);
/* what the last capped finish found (OJPHGPU_E_INVALID before one, or without a cap set) */
int  ojphgpu_encoder_capped_info(ojphgpu_encoder* enc, ojphgpu_capped_info* info);

/* ------------------------------------------------------------------------------------------ *
 * 5d. Transcoding: a codestream recoded to another packaging, step or byte budget without leaving the coefficient domain.
 *    T(cs, out) is the codestream a plain encode of the plan `out` writes when its sub-band planes hold what the block
 *    decoder leaves of `cs`: every code-block of the source decoded and de-quantised as the decoder does (a block that is
 *    not coded is zero), the planes quantised with out's K_max / delta as the encoder's transfer does (its skip rule
 *    included), the result block-coded and laid out by Tier-2.  No inverse transform, no samples, no forward transform:
 *    the block decoder writes the planes of ONE arena and the block coder reads them.
 *    Two identities follow from the decoder's reconstruction point (q + 0.5) delta: at the source's own step the planes
 *    quantise back to q, so T is byte for byte the direct encode of the original image with out's packaging; and at a
 *    step 2^k times the source's, floor((q + 0.5) / 2^k) = floor(q / 2^k), again the direct encode at that step.  A
 *    reversible source is carried over coefficient by coefficient.  Any other step gives a codestream of its own.
 *
 *    ojphgpu_plan_create_transcode (host only): the plan of out_params, checked against the parsed `src`.  out_params =
 *    ojphgpu_plan_params(src) with only these changed: block_w / block_h, precinct_w / precinct_h / precinct_exps,
 *    prog_order, tlm, reserved[1] (tile-part divisions), qstep.  OJPHGPU_E_INVALID, no plan: any other difference; a
 *    differing arena size, or a band whose rectangle, place or pitch differs; a source restricted in resolution or to a
 *    region; ATK / DFS wavelets, a component on the 64-bit sample path, vertically causal blocks; quality factors; a
 *    reversible output with qstep > 0; a reversible band whose K_max is below the source's.  An irreversible output with
 *    qstep <= 0 (a codestream does not carry its base step) is a plan for a transcoder with a byte budget only.
 * ------------------------------------------------------------------------------------------ */
int  ojphgpu_plan_create_transcode(const ojphgpu_plan* src, const ojphgpu_params* out_params, ojphgpu_plan** out);
/* The object: the block decoder of `src` and the block coder of `out` (both outlive it) on one arena -- no frame, no
 * conversion or DWT descriptors.  OJPHGPU_E_INVALID: plans ojphgpu_plan_create_transcode would not have paired.
 * _set_budget: as ojphgpu_encoder_set_budget (section 5b) with size(j) = the length of T(cs, out at qstep(j)); what that
 *   call refuses is refused (a reversible output), 0 switches the budget off.
 * _submit: parses the codestream (resilient as in ojphgpu_t2_parse), checks it against `src` -- another geometry is
 *   OJPHGPU_E_INVALID and leaves the object usable --, uploads its block bytes (the host buffer may go when the call
 *   returns) and enqueues the block decoder as ojphgpu_decoder_run_device chooses it, with a budget the band statistics
 *   behind it.  OJPHGPU_E_INVALID also for an irreversible output with qstep <= 0 and no budget.
 * _finish: collects the decode first (as ojphgpu_decoder_failed_blocks does, repeat included); *failed_blocks (may be
 *   NULL) = the blocks that failed.  A source that was not parsed resiliently with a failed block: OJPHGPU_E_BLOCK, nothing
 *   written; a resilient one: those blocks are zero.  Then the blocks are coded -- without a budget in the encoder's plain
 *   schedule, with one by the search of section 5b -- downloaded and written as ojphgpu_encoder_finish writes them
 *   (OJPHGPU_E_OVERFLOW: *out_len holds the need, call again; OJPHGPU_E_BUDGET leaves the object usable).
 * _rate_info: ojphgpu_encoder_rate_info of the last budgeted finish.
 * _timing (ms): out[0] the block decoder, [1] the band statistics (device events of the last submit); [2] search and
 *   coding, [3] download and Tier-2 (host clock of the last finish). */
typedef struct ojphgpu_transcoder ojphgpu_transcoder;
int  ojphgpu_transcoder_create(const ojphgpu_plan* src, const ojphgpu_plan* out, int device, void* stream, ojphgpu_transcoder** t);
int  ojphgpu_transcoder_set_budget(ojphgpu_transcoder* t, uint64_t max_bytes);
int  ojphgpu_transcoder_submit(ojphgpu_transcoder* t, const uint8_t* h_codestream, size_t len, int resilient);
int  ojphgpu_transcoder_finish(ojphgpu_transcoder* t, uint8_t* h_out, size_t cap, size_t* out_len, uint32_t* failed_blocks);
int  ojphgpu_transcoder_rate_info(ojphgpu_transcoder* t, ojphgpu_rate_info* info);
int  ojphgpu_transcoder_timing(ojphgpu_transcoder* t, float out[4]);
void ojphgpu_transcoder_destroy(ojphgpu_transcoder* t);

/* ------------------------------------------------------------------------------------------ *
 * 5e. Recoding through the sample domain: what section 5d refuses -- another wavelet or number of decompositions, other
 *    tiles, another bit depth, a source restricted in resolution or to a region.  It is what ojph_expand followed by
 *    ojph_compress do through an image file (src/apps/ojph_expand/ojph_expand.cpp, src/apps/ojph_compress/ojph_compress.cpp),
 *    with the frame staying in HBM.  For a source codestream cs, its view V (the restrictions `src` carries: none,
 *    ojphgpu_plan_restrict_resolution, ojphgpu_plan_restrict_region, or both) and the output plan `out`:
 *        F = what ojphgpu_decoder_run_device gives for cs under V (int32; a sample past its nominal range included)
 *        G = fit(F): per component, with s = source depth - output depth, ojphgpu_frame_fit with shift = s and [lo, hi] =
 *            the output's nominal range -- [0, 2^Bo - 1], or [-2^(Bo-1), 2^(Bo-1) - 1] for a signed component.  The clamp
 *            always applies, also at s == 0: it is what the image file in between does (ojph_img_io.cpp:106-230).
 *        R(cs, V, out) = what an encoder of `out` writes for G, in whatever mode it is in.
 *    G sits in the narrowest container the encoder takes for `out`: 8-bit when every output depth is at most 8, 16-bit when
 *    every one is at most 16 (int8 / int16 for signed components, uint8 / uint16 otherwise, as ojphgpu_encoder_run_device8 /
 *    16 read them), else int32.
 *
 *    _create: `src` = a plan of ojphgpu_t2_parse*, restricted or not (it outlives the object, as `out` does).
 *      OJPHGPU_E_INVALID: a source plan that is not a parsed one, an output plan that is; a component count, or a
 *      component's width or height (ojphgpu_plan_comp_info of the restricted source against the output's), that differs --
 *      nothing is resampled here; a component whose signedness changes; a component on the 64-bit sample path on either
 *      side; a region whose absolute origin (image offset + x0, y0) is not a multiple of XRsiz * 2^skipped_res_for_recon
 *      horizontally or YRsiz * 2^skipped_res_for_recon vertically for every component (the sizes may coincide, but the
 *      chroma would be sited half a cell off); and what ojphgpu_decoder_create / ojphgpu_encoder_create refuse.
 *    _encoder: the encoder half, BORROWED: it takes the setters and infos of sections 5b and 5c -- ojphgpu_encoder_set_budget,
 *      _set_quality, _set_quality_capped, _clear_quality, _rate_info, _quality_info, _quality_comp, _capped_info, and the
 *      timing calls -- so that the three modes stay in one place.  ojphgpu_encoder_run_device*, _finish*, _encode* and
 *      _destroy on it are the recoder's alone.  A quality target is measured against G.  Its runs end joined (section 5).
 *    _submit: parses the codestream (resilient as in ojphgpu_t2_parse) and restricts it as `src` is restricted, checks it
 *      against `src` -- another geometry is OJPHGPU_E_INVALID and leaves the object usable --, uploads the bytes of the blocks
 *      it decodes (the host buffer may go when the call returns) and enqueues the decoder's run into the int32 frame, the fit
 *      and the encoder's run on G.  G stays the recoder's until _finish has returned.
 *    _finish: collects the decoder's verdicts first (as ojphgpu_decoder_failed_blocks does; when that repeated the decode,
 *      the fit and the encoder's run are enqueued again before anything is written); *failed_blocks (may be NULL) = the
 *      blocks that failed.  A source that was not parsed resiliently with a failed block: OJPHGPU_E_BLOCK, nothing written; a
 *      resilient one: those blocks are zero, as the decoder leaves them.  Then ojphgpu_encoder_finish (OJPHGPU_E_OVERFLOW:
 *      *out_len holds the need, call again; OJPHGPU_E_BUDGET and OJPHGPU_E_QUALITY leave the object usable).
 *    _frame: G of the last submit (device memory of the object's; valid until the next submit) and its container.
 *    _timing (ms): out[0] the decoder's run, [1] the fit, [2] the encoder's run (device events of the last submit, read
 *      after a wait for the stream); [3] ojphgpu_encoder_finish (host clock of the last finish: searches included).
 *    Memory: the two objects' own, one int32 frame, and G where its container is narrower (at 32 bits the int32 frame is
 *    fitted in place).
 *
 *    A resampling recode (4:4:4 -> 4:2:2 / 4:2:0, 4:2:2 -> 4:2:0, ...): _create_resampled with OJPHGPU_RESAMPLE_COSITED
 *    accepts an output whose components are sub-sampled further than the view's: per component, with a the view's and b
 *    the output's, b.dx == a.dx * fx and b.dy == a.dy * fy with fx, fy each 1 or 2, independently.  Then
 *        G = fit(resample(F)): per component ojphgpu_frame_resample (section 4) with those factors -- taps (1, 2, 1) in a
 *            halved direction, centred ON a source sample, because component sample i sits at reference-grid column
 *            i * XRsiz: with the source component's origin xs0 = ceil(X0 / a.dx), output sample i stands on source index
 *            2 i + px, px = xs0 & 1 (0 under any view, whose output has no image offset; rows alike) -- then the fit above.
 *    F has the view's layout, G the output's; a component with fx == fy == 1 is exactly the fit.  Everything else (the
 *    encoder's modes, a quality target measured against G, _finish, _frame, _timing with the stage as out[1]) is as above.
 *    OJPHGPU_E_INVALID in addition to the list above (a component's size must now be what the output's canvas gives for
 *    the halved grid, (a.w + 1 - px) / 2): a factor other than 1 or 2; upsampling; a view whose absolute origin is not a
 *    multiple of the OUTPUT's XRsiz * 2^skipped_res_for_recon (YRsiz ...).  With OJPHGPU_RESAMPLE_NONE the call is
 *    ojphgpu_recoder_create.  The output plan itself refuses a colour transform over sub-sampled chroma.
 *    _resample_table: the plans judged as _create_resampled judges them, without a device: fills comps[0 .. *n) (cap at
 *    least the component count, else OJPHGPU_E_INVALID) with what the recoder uploads for ojphgpu_frame_resample.
 *    Memory: G gets a buffer of its own also in a 32-bit container whenever a component is resampled.
 * ------------------------------------------------------------------------------------------ */
#define OJPHGPU_RESAMPLE_NONE    0
#define OJPHGPU_RESAMPLE_COSITED 1
typedef struct ojphgpu_recoder ojphgpu_recoder;
int  ojphgpu_recoder_create(const ojphgpu_plan* src, const ojphgpu_plan* out, int device, void* stream, ojphgpu_recoder** r);
int  ojphgpu_recoder_create_resampled(const ojphgpu_plan* src, const ojphgpu_plan* out, int resample, int device, void* stream,
                                      ojphgpu_recoder** r);
int  ojphgpu_recoder_resample_table(const ojphgpu_plan* src, const ojphgpu_plan* out, int resample, ojphgpu_resample_comp* comps,
                                    uint32_t cap, uint32_t* n);
int  ojphgpu_recoder_encoder(ojphgpu_recoder* r, ojphgpu_encoder** enc);
int  ojphgpu_recoder_submit(ojphgpu_recoder* r, const uint8_t* h_codestream, size_t len, int resilient);
int  ojphgpu_recoder_finish(ojphgpu_recoder* r, uint8_t* h_out, size_t cap, size_t* out_len, uint32_t* failed_blocks);
int  ojphgpu_recoder_frame(ojphgpu_recoder* r, const void** d_frame, int* container_bits);
int  ojphgpu_recoder_timing(ojphgpu_recoder* r, float out[4]);
void ojphgpu_recoder_destroy(ojphgpu_recoder* r);

/* ------------------------------------------------------------------------------------------ *
 * 6. Frame pipelines: sequences of frames of one shape with PCIe copies, kernels and host Tier-2 of
 *    consecutive frames overlapped (pinned staging, separate copy-in / compute / copy-out streams).
 *    In the reference one codestream object is re-used across the frames of a sequence through
 *    codestream::restart() (ojph_codestream.h:204, ojph_codestream_local.cpp:78-110): exchange() hands out
 *    line buffers, flush() writes the file (:1148-1270); read_headers() / create() / pull() read one
 *    (:769-1146, :1227-1270).  The pipe keeps that contract per frame -- the caller writes samples into
 *    memory the library hands out and receives a finished codestream, or the other way round -- and
 *    keeps `depth` (2..16) frames in flight.  One caller thread per pipe; results come back in
 *    submission order.  container_bits = 8 | 16 | 32 (see ojphgpu_encoder_run_device16 / 8); host_threads =
 *    threads that do a frame's host part (packet headers / parsing), 0 = 2.
 *    Three pipes: the encoder's (frames in, codestreams out), the decoder's (codestreams in, frames out) and, at the end
 *    of this section, the transcoder's (ojphgpu_tc_pipe: codestreams in, codestreams out, section 5d frame after frame).
 * ------------------------------------------------------------------------------------------ */
typedef struct ojphgpu_enc_pipe ojphgpu_enc_pipe;
typedef struct ojphgpu_dec_pipe ojphgpu_dec_pipe;

int  ojphgpu_enc_pipe_create(const ojphgpu_plan* plan, int device, uint32_t depth, int container_bits,
                             uint32_t host_threads, ojphgpu_enc_pipe** out);
void ojphgpu_enc_pipe_destroy(ojphgpu_enc_pipe* pipe);
/* pinned host memory for the next frame -- the frame layout of ojphgpu_plan_comp_info in container_bits-bit
 * elements -- which the caller fills (what exchange() hands out line by line).  OJPHGPU_E_AGAIN when all
 * `depth` slots are in flight: collect first. */
int  ojphgpu_enc_pipe_acquire(ojphgpu_enc_pipe* pipe, void** h_frame, size_t* bytes);
/* the acquired frame is complete (flush()): queues H2D -> kernels -> D2H of the block lengths -> packet
 * headers (host threads) -> codestream assembly on the device -> D2H, and returns at once */
int  ojphgpu_enc_pipe_submit(ojphgpu_enc_pipe* pipe);
/* the oldest submitted frame's codestream (SOC .. EOC, byte-identical to ojphgpu_encode's); blocks until it
 * is complete.  *h_codestream is pinned memory of the pipe, valid until the next _collect / _destroy. */
int  ojphgpu_enc_pipe_collect(ojphgpu_enc_pipe* pipe, const uint8_t** h_codestream, size_t* len);
/* out[0] frames completed, [1] mean host Tier-2 time per frame (ms), [2] mean submit -> codestream latency
 * (ms), [3] host threads coding the packet headers of one frame */
int  ojphgpu_enc_pipe_stats(ojphgpu_enc_pipe* pipe, double out[4]);

/* The frames of this pipe are handed over PIXEL-INTERLEAVED (R G B R G B ..., the order of .ppm files and of capture
 * buffers; ppm_in::read, src/apps/others/ojph_img_io.cpp:338-375) instead of as planes: pixel_bits = 8 or 16 per
 * sample, 16-bit samples big endian (as in the files) when big_endian != 0.  _acquire then hands out width * height *
 * components * pixel_bits / 8 bytes, and a launch on the device turns them into the planar containers
 * (ojphgpu_unpack_pixels).  Components must have one size and be unsigned, pixel_bits must hold the bit depth and
 * must not exceed container_bits.  Call before the first _acquire; until then the call may be repeated with a different
 * value (the buffers follow), and pixel_bits = 0 switches back to planes.  The three hand-overs -- this one, _set_packed,
 * _set_video -- exclude each other: while one is on, the setters of the other two return OJPHGPU_E_INVALID whatever their
 * argument, 0 included.  A refusal leaves the pipe as it was. */
int  ojphgpu_enc_pipe_set_pixels(ojphgpu_enc_pipe* pipe, int pixel_bits, int big_endian);
/* ... or as planes of bit-packed samples (ojphgpu_unpack_bits: bits = 10, 12, 14; the whole frame one bit string in
 * the plane order of the planar layout): _acquire hands out ceil(samples * bits / 8) bytes rounded up to whole groups
 * of 32 samples.  Unsigned components whose depth fits `bits`, 16- or 32-bit containers.  Before the first _acquire,
 * repeatable until then with a different value; bits = 0 switches back. */
int  ojphgpu_enc_pipe_set_packed(ojphgpu_enc_pipe* pipe, int bits);
/* ... or as one 4:2:2 video buffer (section 7b: format = OJPHGPU_VIDEO_*; 0 switches back to planes): _acquire hands out
 * the format's frame_bytes (ojphgpu_video_layout) and a launch on the device turns them into the planes
 * (ojphgpu_unpack_video).  Call before the first _acquire -- until then the call may be repeated with a different format --
 * not together with _set_pixels / _set_packed.
 * OJPHGPU_E_INVALID unless the pipe's plan has exactly three unsigned components of one bit depth that fits the format and
 * the container, of sizes (w, h), (ceil(w / 2), h), (ceil(w / 2), h); a refusal leaves the pipe as it was.
 * Or as one 4:2:0 video buffer (section 7c: OJPHGPU_VIDEO_NV12 / _NV21 / _P0XX): the same rules, the chroma planes
 * (ceil(w / 2), ceil(h / 2)) each; _acquire hands out frame_bytes of the TIGHT layout of ojphgpu_video420_layout -- the luma
 * plane, then the chroma plane, both at row_bytes -- and the launch is ojphgpu_unpack_video420.  A 4:2:2 format on a 4:2:0
 * plan is refused, and a 4:2:0 format on a 4:2:2 plan.  The bytes on the link are those of planes in the matching
 * containers; what is saved is the host's de-interleaving pass.
 * Or as one 4:4:4 packed buffer (section 7d: OJPHGPU_VIDEO_V410 ... _ARGB): exactly three unsigned components of one depth
 * that the format and the container hold, all of the size of component 0 (a sub-sampled plan is refused, as a 4:2:2 or 4:2:0
 * format stays refused on a 4:4:4 plan); _acquire hands out frame_bytes of the tight layout of ojphgpu_video444_layout, rows at
 * row_bytes, and the launch is ojphgpu_unpack_video444.  A 10-bit frame crosses the link in two thirds of the bytes of its
 * planes in 16-bit containers. */
int  ojphgpu_enc_pipe_set_video(ojphgpu_enc_pipe* pipe, int format);
/* The frames are handed over as one RGB buffer and coded as Y, Cb, Cr 4:4:4, 4:2:2 or 4:2:0: an RGB member of the 4:4:4
 * family (OJPHGPU_VIDEO_BGRA / _RGBA / _ARGB / _R210 / _R10K) and a colour spec (section 7e: OJPHGPU_COLOUR_* standard and
 * ranges; rgb_depth: of the buffer's samples, 0 = the plan's depth).  Two launches per frame on the compute stream behind the
 * upload: ojphgpu_unpack_video444 into a buffer of 3 w h containers of the slot, then ojphgpu_frame_rgb_to_ycc into the slot's
 * image with the FORWARD table of (standard, rgb_depth, the plan's depth, the ranges) and the plan's chroma cell.  Every
 * codestream is, byte for byte, the plain encode of those planes; a byte budget, a quality target and a cap combine with it
 * as with _set_video (a target is measured against the Y, Cb, Cr planes).  The calling window of _set_video; excludes
 * _set_pixels / _set_packed AND the plain _set_video (one or the other, for the life of the pipe or until set back to planes
 * by format 0); _set_video itself is unchanged.
 * OJPHGPU_E_INVALID, the pipe left as it was: a null spec; a format that is not one of the five (v410, Y410, AYUV, Y4XX hold
 * Y, Cb, Cr already; the 4:2:2 and 4:2:0 formats); an unknown standard or range; a plan that has not exactly three unsigned
 * components of one depth of 8 .. 16 bits that the container holds, component 0 on the reference grid (XRsiz = YRsiz = 1),
 * components 1 and 2 sub-sampled alike by 1 or 2 each way with planes of (ceil(w / fx), ceil(h / fy)); an odd image offset in a
 * halved direction (the chroma sample would stand on the cell's second luma sample: phase 1); an rgb_depth that the format
 * does not hold (the byte formats: 8; R210 / R10K: 8 .. 10) or that is wider than the container.  (A colour transform over
 * sub-sampled components is refused by the plan already; over a 4:4:4 plan it applies to Y, Cb, Cr as to any three planes.) */
typedef struct ojphgpu_colour_spec { int standard, rgb_range, ycc_range; uint32_t rgb_depth; } ojphgpu_colour_spec;
int  ojphgpu_enc_pipe_set_video_colour(ojphgpu_enc_pipe* pipe, int format, const ojphgpu_colour_spec* spec);

/* Every frame of this pipe is coded to a byte budget (section 5b): each collected codestream is, byte for byte, the plain
 * encode of its frame at qstep(j*), with the certificate size(j*) <= budget < size(j* + 1) measured for that frame.
 * Switched on by a call with max_bytes > 0 before the first _acquire (the refusals are ojphgpu_encoder_set_budget's, and
 * the output buffers are re-sized for the finest step of the grid: one per slot and one spare); from then on the call may
 * be repeated between frames, and the value in force at _submit is that frame's budget (a bit-reservoir controller moves
 * it every frame).  OJPHGPU_E_INVALID: switching on after the first _acquire, and 0 once the mode is on; 0 on a plain
 * pipe before the first _acquire changes nothing.  The search of a frame starts from the j* of the last certified frame
 * (ojphgpu_rate_search_hint) and alternates its trials between two output buffers, so a frame whose answer is its
 * predecessor's costs the two trials the certificate consists of and nothing is coded twice.  A frame whose budget not
 * even index 0 meets: its _collect returns OJPHGPU_E_BUDGET, its slot is free again, the frames around it are not
 * affected.  Combines with _set_pixels / _set_packed.  A pipe that never had a budget issues what it issued without
 * this call.  A refusal leaves the pipe as it was; should switching on fail later (OJPHGPU_E_NOMEM while the buffers
 * change size), the pipe is neither plain nor budgeted any more and every call but _destroy returns OJPHGPU_E_INVALID. */
int  ojphgpu_enc_pipe_set_budget(ojphgpu_enc_pipe* pipe, uint64_t max_bytes);
/* what the search of the frame collected last found (after OJPHGPU_E_BUDGET: passes and first_guess); OJPHGPU_E_INVALID
 * before the first _collect of a budgeted pipe and after a frame that failed otherwise */
int  ojphgpu_enc_pipe_rate_info(ojphgpu_enc_pipe* pipe, ojphgpu_rate_info* info);

/* Every frame of this pipe is coded to a quality target (section 5c): each collected codestream is, byte for byte, the
 * plain encode of its frame at qstep(j*), with the certificate SSE(j*) <= max_sse and (j* == 0 or SSE(j* - 1) > max_sse)
 * measured for that frame.  The rules are the budget's: switched on by the first call before the first _acquire -- 0 is a
 * target, so the call itself is the switch, not its value -- and from then on the call may be repeated between frames; the
 * value in force at _submit is that frame's target; there is no way back.  OJPHGPU_E_INVALID: whatever
 * ojphgpu_encoder_set_quality refuses; switching on after the first _acquire; a pipe with a byte budget (and _set_budget on
 * a pipe with a target: a target under a byte cap is ojphgpu_enc_pipe_set_quality_capped below).  The first call re-sizes every slot's output buffer for the finest
 * step of the grid and allocates what ojphgpu_encoder_set_quality allocates; should it fail later than its refusals, the
 * pipe answers as ojphgpu_enc_pipe_set_budget describes.  The search of a frame starts from the j* of the last certified
 * frame (ojphgpu_quality_search_hint), runs on the pipe's compute stream in frame order and compares against the slot's own
 * copy of the frame -- the planes in container_bits-bit elements, after the unpacking of _set_pixels / _set_packed -- so the
 * caller keeps nothing valid; the decoded side stays int32 (a sample one past an 8-bit container's range counts as it is).
 * A frame whose answer is its predecessor's costs the two trials of the certificate (one at index 0) and the one coding of
 * its blocks.  A frame whose target not even index 240 meets: its _collect returns OJPHGPU_E_QUALITY, its slot is free
 * again, the hint stays where it was and the frames around it are not affected.  A pipe that never had a target issues
 * what it issued without this call. */
int  ojphgpu_enc_pipe_set_quality(ojphgpu_enc_pipe* pipe, uint64_t max_sse);
/* what the search of the frame collected last found, and the first index it tried (after OJPHGPU_E_QUALITY: passes and
 * first_guess); OJPHGPU_E_INVALID before the first _collect of such a pipe and after a frame that failed otherwise */
int  ojphgpu_enc_pipe_quality_info(ojphgpu_enc_pipe* pipe, ojphgpu_quality_info* info, uint32_t* first_guess);
/* SSE and PAE of component `comp` of that frame at j* (OJPHGPU_E_INVALID when it was not certified) */
int  ojphgpu_enc_pipe_quality_comp(ojphgpu_enc_pipe* pipe, uint32_t comp, uint64_t* sse, uint32_t* pae);
/* Every frame of this pipe is coded to a quality target under a byte cap (section 5c, "under a byte cap"): each collected
 * codestream is, byte for byte, what ojphgpu_encoder_set_quality_capped writes for that frame and pair.  Switched on by the
 * first call with cap_bytes > 0 before the first _acquire, or never; from then on both values may move between frames (this
 * call, or _set_quality for the target alone), the pair in force at _submit is the frame's, and the cap may not go back to
 * 0.  cap_bytes == 0 on a pipe without a cap is exactly ojphgpu_enc_pipe_set_quality.  OJPHGPU_E_INVALID: what that call
 * refuses; a quality pipe made without a cap (it has no spare output set and no pinned histograms: it cannot gain one);
 * cap_bytes == 0 on a capped pipe.  _set_budget on such a pipe stays refused.  The ordered worker runs
 * ojphgpu_capped_search per frame: the quality trials start from the q of the last certified frame, the size trials
 * alternate between the slot's output set and the spare -- the set with the answer is never overwritten and nothing is
 * coded twice -- and start from the j* of the last frame the cap bound; the band statistics are launched only when the
 * cap binds.  Both hints stay where they are after a frame that fails.  A frame with size(0) > cap: its own _collect returns
 * OJPHGPU_E_BUDGET and the sequence goes on.  On an unchanged frame: MET costs two quality trials and one coding,
 * BY_BUDGET at most three and three. */
int  ojphgpu_enc_pipe_set_quality_capped(ojphgpu_enc_pipe* pipe, uint64_t max_sse, uint64_t cap_bytes);
/* what the capped search of the frame collected last found (after OJPHGPU_E_BUDGET: the passes); OJPHGPU_E_INVALID before the
 * first _collect of such a pipe and after a frame that failed otherwise.  ojphgpu_enc_pipe_quality_comp answers for j*. */
int  ojphgpu_enc_pipe_capped_info(ojphgpu_enc_pipe* pipe, ojphgpu_capped_info* info);

/* the first codestream of the sequence fixes the frame geometry (it is only parsed, not decoded); every
 * submitted codestream must describe the same frame format and code-block grid (quantisation may differ) */
int  ojphgpu_dec_pipe_create(const uint8_t* h_codestream, size_t len, int resilient, int device, uint32_t depth,
                             int container_bits, uint32_t host_threads, ojphgpu_dec_pipe** out);
/* A pipe that decodes a VIEW of every frame: at reduced resolution (ojphgpu_plan_restrict_resolution with the two counts;
 * 0, 0: none), a rectangle { x0, y0, w, h } of the reference grid (ojphgpu_plan_restrict_region, applied after the
 * resolution; NULL: none), or both -- frame for frame what a decoder object created from the plan restricted that way
 * decodes.  What those two calls refuse (a skip beyond the decompositions, w or h 0, a rectangle outside the image, a region
 * on Part-2 or 64-bit components) is refused here with OJPHGPU_E_INVALID.  The frames handed out, ojphgpu_dec_pipe_plan and
 * _set_pixels / _set_packed describe the view's frame (_set_pixels: the view's component planes must be of one size).
 * Of the codestream only the bytes of the code-blocks the view depends on cross PCIe (and the aligned dwords around each
 * run): a kernel reads them as runs (ojphgpu_plan_upload_runs) out of the slot's pinned codestream and lays them out in
 * device memory (ojphgpu_gather_runs).  Beside them go, as in a plain pipe, the block descriptors, and the run table (24
 * bytes per run, one copy into device memory ahead of the kernel).  0, 0, NULL is
 * ojphgpu_dec_pipe_create.  The view is fixed for the life of the pipe. */
int  ojphgpu_dec_pipe_create_view(const uint8_t* h_codestream, size_t len, int resilient, uint32_t skipped_res_for_data,
                                  uint32_t skipped_res_for_recon, const uint32_t* region, int device, uint32_t depth,
                                  int container_bits, uint32_t host_threads, ojphgpu_dec_pipe** out);
/* of the frame collected last (whatever its outcome; zeros where it failed before its descriptors were filled):
 * out[0] code-blocks decoded, [1] code-blocks of the codestream, [2] bytes staged for the block decoder -- of a view: what
 * the gather lays out; of a plain pipe: the byte range uploaded -- [3] runs (0: a plain pipe), [4] coded bytes of the
 * decoded blocks.  OJPHGPU_E_INVALID before the first _collect. */
int  ojphgpu_dec_pipe_view_info(ojphgpu_dec_pipe* pipe, uint64_t out[5]);
void ojphgpu_dec_pipe_destroy(ojphgpu_dec_pipe* pipe);
int  ojphgpu_dec_pipe_plan(ojphgpu_dec_pipe* pipe, const ojphgpu_plan** plan);   /* owned by the pipe */
/* pinned host memory for the next codestream of `len` bytes (read the file straight into it) */
int  ojphgpu_dec_pipe_acquire(ojphgpu_dec_pipe* pipe, size_t len, uint8_t** h_codestream);
/* queues parse (host threads) -> H2D of the code-block bytes + descriptors -> kernels -> D2H of the frame */
int  ojphgpu_dec_pipe_submit(ojphgpu_dec_pipe* pipe);
/* the oldest submitted frame: container_bits-bit samples in the layout of ojphgpu_plan_comp_info, in
 * pinned memory valid until the next _collect / _destroy.  OJPHGPU_E_BLOCK when code-blocks failed and the
 * pipe is not resilient (the frame is still handed out, failed blocks zeroed, *failed_blocks counts them). */
int  ojphgpu_dec_pipe_collect(ojphgpu_dec_pipe* pipe, const void** h_frame, size_t* bytes, uint32_t* failed_blocks);
/* out[0] frames completed, [1] mean host parse time per frame (ms), [2] mean submit -> frame latency (ms), [3] host threads */
int  ojphgpu_dec_pipe_stats(ojphgpu_dec_pipe* pipe, double out[4]);
/* frames this pipe decoded twice because the one-launch block decoder asked for it (ojphgpu_decoder_failed_blocks) */
int  ojphgpu_dec_pipe_fused_retries(ojphgpu_dec_pipe* pipe, uint32_t* count);
/* decoded frames come back pixel-interleaved, clamped to [0, 2^depth - 1] -- ONE depth for the frame: the components
 * must share their bit depth (a .ppm has one maxval), otherwise OJPHGPU_E_INVALID -- (ppm_out::write and its converters,
 * ojph_img_io.cpp:99-226, :539-556); same conditions as ojphgpu_enc_pipe_set_pixels; call before the first _submit.  For
 * all three setters of a decoder pipe: until then the call may be repeated with a different value, and they exclude each
 * other as the encoder pipe's do. */
int  ojphgpu_dec_pipe_set_pixels(ojphgpu_dec_pipe* pipe, int pixel_bits, int big_endian);
int  ojphgpu_dec_pipe_set_packed(ojphgpu_dec_pipe* pipe, int bits);     /* decoded frames come back bit-packed, clamped to [0, 2^bits - 1] */
/* decoded frames come back as one 4:2:2 video buffer (section 7b), clamped to [0, 2^depth - 1]: _collect hands back the
 * format's frame_bytes.  The conditions of ojphgpu_enc_pipe_set_video, judged on the view's plan when the pipe decodes a
 * view: a reduced resolution always passes, a region when its planes have those sizes (an even x0 guarantees it).  Call
 * before the first _submit, not together with _set_pixels / _set_packed; 0 switches back to planes.  The 4:2:0 formats
 * of section 7c come back in the tight layout (ojphgpu_pack_video420); a window passes when its x0 AND y0 are even, and one
 * with an odd y0 is refused whatever its height, as one with an odd x0 is.  The 4:4:4 formats of section 7d come back in
 * the tight layout too (ojphgpu_pack_video444, alpha opaque); there is no chroma cell, so a window passes at any x0, y0. */
int  ojphgpu_dec_pipe_set_video(ojphgpu_dec_pipe* pipe, int format);
/* decoded Y, Cb, Cr frames come back as one RGB buffer: ojphgpu_frame_ycc_to_rgb with the INVERSE table from the slot's image
 * into its buffer of 3 w h containers, then ojphgpu_pack_video444 -- the mirror of ojphgpu_enc_pipe_set_video_colour, with its
 * conditions, judged on the view's plan when the pipe decodes a view: a reduced resolution always passes, a window when its
 * x0 is even where fx == 2 and its y0 is even where fy == 2 (both together: a multiple of 2^(skip_recon + 1), even on the
 * reduced grid).  The samples enter as the pipe's containers hold them (a decoded
 * sample past its range is not clamped first; a 16-bit container saturates at 0 and 65535, an 8-bit one at 0 and 255).  A pipe
 * with 32-bit containers is refused: its planes are int32 and may hold negative samples.  The calling window and the
 * exclusions of _set_video. */
int  ojphgpu_dec_pipe_set_video_colour(ojphgpu_dec_pipe* pipe, int format, const ojphgpu_colour_spec* spec);

/* The transcode pipe: host codestream in, host codestream out -- section 5d's T(cs, out), source after source, with the
 * parse, the upload, the download and Tier-2 of neighbouring frames overlapped with the device as the other two pipes do
 * it.  Every collected codestream is, byte for byte, what ojphgpu_transcoder_submit + _finish give for its source.
 * A frame passes three stages: host threads parse it, check it, fill its block descriptors into pinned memory and enqueue
 * the uploads on the copy-in stream; ONE ordered thread per pipe owns the compute stream and runs, frame by frame in submit
 * order, the block decoder, the collection of its verdicts (with the repeat a one-launch run may ask for; no block is coded
 * before the verdicts are in) and the coding -- plain, or the budget's search; host threads lay the codestream out from
 * the block lengths, and the assembly and the download run on the copy-out stream.  The pipe has one transcoder object and
 * so one arena: frame n + 1's block decoder writes the planes frame n's coding reads, hence the frames are strictly serial
 * on the compute stream and only the front and the finish of their neighbours overlap it.
 * _create: the first source (parsed as ojphgpu_t2_parse parses it with `resilient`, as every later one is; it fixes the
 *   geometry) and the output plan ojphgpu_plan_create_transcode made from that parse (it outlives the pipe); depth and
 *   host_threads as above (that many threads for the front, and as many for the finish).  Refused: what
 *   ojphgpu_transcoder_create refuses.  An irreversible output with qstep <= 0 is a pipe for a byte budget only: unless
 *   _set_budget has switched one on, its first _acquire returns OJPHGPU_E_INVALID.
 * _acquire: pinned host memory for the next source of `len` bytes, as ojphgpu_dec_pipe_acquire; OJPHGPU_E_AGAIN when all
 *   slots are in flight.
 * _submit: queues the acquired source and returns at once.
 * _collect: the oldest submitted frame's output codestream, in pinned memory of the pipe that stays valid until its slot is
 *   acquired again; *failed_blocks (may be NULL) = the source's blocks that failed to decode (zero blocks in the output of
 *   a resilient pipe).  A frame fails from its own _collect only, its slot is free again, and the frames around it are byte
 *   for byte what they are without it: a source that does not parse (the parser's code), one of another geometry
 *   (OJPHGPU_E_INVALID), failed blocks in a pipe that is not resilient (OJPHGPU_E_BLOCK), a budget no step fits
 *   (OJPHGPU_E_BUDGET).
 * _set_budget: the rules of ojphgpu_enc_pipe_set_budget -- on from before the first _acquire or never, the value in force
 *   at _submit is the frame's, it may move between frames but not back to 0 -- with the refusals of
 *   ojphgpu_transcoder_set_budget.  The search of a frame starts from the j* of the last certified frame and alternates its
 *   trials between the slot's output buffer and one spare: `passes` counts trials only and nothing is coded twice.
 * _rate_info: of the frame collected last, as ojphgpu_enc_pipe_rate_info.
 * _stats: out[0] frames completed, [1] mean host parse + descriptor time per frame (ms), [2] mean host Tier-2 time per frame
 *   (ms), [3] mean submit -> codestream latency (ms).
 * _fused_retries: frames whose block decoder ran twice because the one launch asked for it (ojphgpu_dec_pipe_fused_retries). */
typedef struct ojphgpu_tc_pipe ojphgpu_tc_pipe;
int  ojphgpu_tc_pipe_create(const uint8_t* h_codestream, size_t len, int resilient, const ojphgpu_plan* out_plan, int device,
                            uint32_t depth, uint32_t host_threads, ojphgpu_tc_pipe** out);
void ojphgpu_tc_pipe_destroy(ojphgpu_tc_pipe* pipe);
int  ojphgpu_tc_pipe_acquire(ojphgpu_tc_pipe* pipe, size_t len, uint8_t** h_codestream);
int  ojphgpu_tc_pipe_submit(ojphgpu_tc_pipe* pipe);
int  ojphgpu_tc_pipe_collect(ojphgpu_tc_pipe* pipe, const uint8_t** h_out, size_t* len, uint32_t* failed_blocks);
int  ojphgpu_tc_pipe_set_budget(ojphgpu_tc_pipe* pipe, uint64_t max_bytes);
int  ojphgpu_tc_pipe_rate_info(ojphgpu_tc_pipe* pipe, ojphgpu_rate_info* info);
int  ojphgpu_tc_pipe_stats(ojphgpu_tc_pipe* pipe, double out[4]);
int  ojphgpu_tc_pipe_fused_retries(ojphgpu_tc_pipe* pipe, uint32_t* count);

/* ---------------------------------------------------------------------------------------------
 * 7. Pixel-interleaved samples <-> planar containers on the device (kernels_pixels.hip)
 * ------------------------------------------------------------------------------------------- */
/* d_pixels: width * height pixels of num_comps samples each, pixel_bits = 8 or 16 bits per sample (16-bit samples
 * byte-swapped when big_endian != 0); d_planes: num_comps planes of width * height samples in container_bits-bit
 * elements (8, 16, 32; not narrower than pixel_bits).  Replaces the per-sample loops of the reference's image
 * readers (ppm_in::read, ojph_img_io.cpp:338-375). */
int  ojphgpu_unpack_pixels(void* stream, const void* d_pixels, void* d_planes, uint32_t width, uint32_t height,
                           uint32_t num_comps, int pixel_bits, int big_endian, int container_bits);
/* the way back, values clamped to [0, 2^bit_depth - 1] (gen_cvrt_32b*_to_*, ojph_img_io.cpp:99-226) */
int  ojphgpu_pack_pixels(void* stream, const void* d_planes, void* d_pixels, uint32_t width, uint32_t height,
                         uint32_t num_comps, int container_bits, int pixel_bits, int big_endian, uint32_t bit_depth);
/* Bit-packed samples: 10, 12 or 14 bits each, consecutive in one little-endian bit string (sample i = bits
 * [i * bits, (i + 1) * bits)), the buffer padded to a multiple of 32 samples (4 * bits bytes, 4-byte aligned) <-> 16- or
 * 32-bit containers.  A 12-bit frame crosses PCIe in 1.5 instead of 2 bytes per sample this way (the link is what
 * bounds the frame pipelines).  Packing clamps to [0, 2^bits - 1].  No counterpart in the reference, whose files hold
 * such samples in 16-bit words. */
int  ojphgpu_unpack_bits(void* stream, const void* d_packed, void* d_samples, uint64_t num_samples, int bits, int container_bits);
int  ojphgpu_pack_bits(void* stream, const void* d_samples, void* d_packed, uint64_t num_samples, int container_bits, int bits);
/* ---- 7b. 4:2:2 video buffers (kernels_video.hip): the frame as capture cards, SDI / ST 2110 receivers, ffmpeg's rawvideo
 * and display paths hold it, one packed buffer.  The frame is width x height luma samples; Cb and Cr hold cw = ceil(width /
 * 2) samples per row; pair k of a row holds Y[2k], Y[2k + 1], Cb[k], Cr[k], and for odd width the last pair's second luma is
 * padding.  Rows follow each other at row_bytes.
 *   OJPHGPU_VIDEO_UYVY  bytes Cb Y0 Cr Y1 per pair                                    row_bytes 4 * cw     depth <= 8
 *   OJPHGPU_VIDEO_YUY2  bytes Y0 Cb Y1 Cr per pair                                    row_bytes 4 * cw     depth <= 8
 *   OJPHGPU_VIDEO_V210  groups of 6 pixels = four little-endian dwords of three 10-bit fields each (bits 0-9, 10-19, 20-29;
 *                       bits 30-31 zero): (Cb0, Y0, Cr0) (Y1, Cb1, Y2) (Cr1, Y3, Cb2) (Y4, Cr2, Y5); the row padded with
 *                       zero groups to a multiple of 48 pixels          row_bytes 128 * ceil(width / 48)   depth <= 10
 *   OJPHGPU_VIDEO_Y2XX  little-endian 16-bit words Y0 Cb Y1 Cr per pair, the sample in the high `depth` bits (Y210, Y212,
 *                       Y216)                                                         row_bytes 8 * cw     9 <= depth <= 16
 * Unpacking: a sample is its field (Y2XX: word >> (16 - depth)); padding fields and groups, bits 30-31 and the low bits of
 * a Y2XX word are not looked at, no value is range-checked.  Packing: every sample is clamped to [0, 2^depth - 1] as
 * ojphgpu_pack_pixels does (no "legal range"), a Y2XX sample is shifted up with zero low bits, and every byte of [0,
 * row_bytes * height) is written -- padding fields, padding groups and bits 30-31 as zero -- and nothing beyond.
 * d_planes: the frame layout of ojphgpu_plan_comp_info for such a frame -- Y width x height, then Cb and Cr cw x height
 * each, tightly packed -- in container_bits-bit elements (8: UYVY and YUY2 only; 16; 32).  OJPHGPU_E_INVALID: an unknown
 * format, a null pointer, a zero size, a bit_depth outside the format's column, a container narrower than bit_depth, a
 * d_video that is not 16-byte aligned. */
#define OJPHGPU_VIDEO_UYVY 1
#define OJPHGPU_VIDEO_YUY2 2
#define OJPHGPU_VIDEO_V210 3
#define OJPHGPU_VIDEO_Y2XX 4
int  ojphgpu_video_layout(int format, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* frame_bytes);   /* host only */
int  ojphgpu_unpack_video(void* stream, int format, const void* d_video, void* d_planes, uint32_t width, uint32_t height,
                          uint32_t bit_depth, int container_bits);
int  ojphgpu_pack_video(void* stream, int format, const void* d_planes, void* d_video, uint32_t width, uint32_t height,
                        int container_bits, uint32_t bit_depth);
/* ---- 7c. 4:2:0 video buffers (kernels_video420.hip): the frame as hardware video decoders and encoders, ffmpeg's hardware
 * frames and most 8-bit and HDR delivery paths hold it, TWO planes.  The frame is width x height luma samples; with cw =
 * ceil(width / 2) and ch = ceil(height / 2), Cb and Cr are cw x ch each.  The luma plane has `height` rows; the chroma plane
 * has ch rows, element k of a row being the pair (Cb[k], Cr[k]).
 *   OJPHGPU_VIDEO_NV12  bytes; chroma Cb Cr                                        row_bytes 2 * cw     depth <= 8
 *   OJPHGPU_VIDEO_NV21  bytes; chroma Cr Cb                                        row_bytes 2 * cw     depth <= 8
 *   OJPHGPU_VIDEO_P0XX  little-endian 16-bit words, the sample in the high `depth` bits (P010, P012, P016); chroma Cb Cr
 *                                                                                  row_bytes 4 * cw     9 <= depth <= 16
 * row_bytes is that of both planes: for odd width a luma row ends in one padding sample.  The TIGHT layout, which the pipes
 * hand out (ojphgpu_video420_layout): luma rows at row_bytes, the chroma plane at chroma_offset = row_bytes * height,
 * frame_bytes = row_bytes * (height + ch).  The two stages take the planes as two pointers, each with its own pitch in bytes
 * (>= row_bytes), so that a decoder's surface, whose pitch and chroma offset are its own, is read or written in place.
 * Unpacking: a sample is its element (P0XX: word >> (16 - depth)); the padding luma sample, the low bits of a P0XX word and
 * everything between row_bytes and the pitch are not looked at, no value is range-checked.  Packing: every sample is clamped
 * to [0, 2^depth - 1] as ojphgpu_pack_video does, a P0XX sample is shifted up with zero low bits, every byte of [0,
 * row_bytes) of every row of both planes is written -- padding as zero -- and NOTHING else: the bytes between row_bytes and
 * the pitch and everything outside the two planes keep their contents.
 * d_planes: the frame layout of ojphgpu_plan_comp_info for such a frame -- Y width x height, then Cb, then Cr cw x ch, tightly
 * packed -- in container_bits-bit elements (8: NV12 and NV21 only; 16; 32).  OJPHGPU_E_INVALID: an unknown format (the codes
 * of section 7b included), a null pointer, a zero size, a bit_depth outside the format's column, a container narrower than
 * bit_depth or 8 with P0XX, a pitch below row_bytes, a d_luma, d_chroma or pitch that is not a multiple of the chroma element
 * (2 bytes for NV12 / NV21, 4 for P0XX), row_bytes or height + ch beyond 32 bits.  No further alignment is required: in the
 * tight layout of an odd-sized frame the chroma plane starts 2 bytes off a dword, and a pitch may change the alignment row
 * by row; the kernels take, per row, the widest piece its address allows. */
#define OJPHGPU_VIDEO_NV12 0x11
#define OJPHGPU_VIDEO_NV21 0x12
#define OJPHGPU_VIDEO_P0XX 0x13
int  ojphgpu_video420_layout(int format, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* chroma_offset,
                             uint64_t* frame_bytes);   /* host only */
int  ojphgpu_unpack_video420(void* stream, int format, const void* d_luma, uint32_t luma_pitch, const void* d_chroma,
                             uint32_t chroma_pitch, void* d_planes, uint32_t width, uint32_t height, uint32_t bit_depth,
                             int container_bits);
int  ojphgpu_pack_video420(void* stream, int format, const void* d_planes, void* d_luma, uint32_t luma_pitch, void* d_chroma,
                           uint32_t chroma_pitch, uint32_t width, uint32_t height, int container_bits, uint32_t bit_depth);
/* ---- 7d. 4:4:4 packed video (kernels_video444.hip): the frame as capture cards, SDI / ST 2110 receivers, graphics surfaces
 * and ffmpeg's rawvideo hold it, ONE buffer of width x height pixels, one interleaved word per pixel, the rows following each
 * other at a pitch; row_bytes = pixel_bytes * width.  Components 0, 1, 2 of the plan are (Y, Cb, Cr) or (R, G, B), as the
 * format names them; the codec's colour transform is the plan's business, as it is with _set_pixels.
 *   constant            pixel                                fields                                            depth b    containers
 *   OJPHGPU_VIDEO_V410  one little-endian dword              Cb bits 2-11, Y 12-21, Cr 22-31; bits 0-1 padding  b <= 10    16, 32
 *   OJPHGPU_VIDEO_Y410  one little-endian dword              Cb 0-9, Y 10-19, Cr 20-29; bits 30-31 alpha        b <= 10    16, 32
 *   OJPHGPU_VIDEO_R210  one BIG-endian dword                 R 20-29, G 10-19, B 0-9; bits 30-31 padding        b <= 10    16, 32
 *   OJPHGPU_VIDEO_R10K  one BIG-endian dword                 R 22-31, G 12-21, B 2-11; bits 0-1 padding         b <= 10    16, 32
 *   OJPHGPU_VIDEO_Y4XX  four little-endian 16-bit words      Cb, Y, Cr, A; the sample in the high b bits of its
 *                                                            word (Y412, Y416)                                  9 <= b <= 16  16, 32
 *   OJPHGPU_VIDEO_AYUV  bytes Cr, Cb, Y, A (Microsoft AYUV; ffmpeg vuya)                                        b <= 8     8, 16, 32
 *   OJPHGPU_VIDEO_BGRA  bytes B, G, R, A                                                                        b <= 8     8, 16, 32
 *   OJPHGPU_VIDEO_RGBA  bytes R, G, B, A                                                                        b <= 8     8, 16, 32
 *   OJPHGPU_VIDEO_ARGB  bytes A, R, G, B                                                                        b <= 8     8, 16, 32
 * Unpacking: a sample is its field (Y4XX: word >> (16 - b)); padding bits, alpha, the low bits of a Y4XX word and everything
 * between row_bytes and the pitch are not looked at, no value is range-checked.  Packing: every sample is clamped to [0, 2^b -
 * 1] as ojphgpu_pack_video does, padding bits are zero, alpha is opaque (3 for Y410, 0xFF for the byte formats, (2^b - 1) <<
 * (16 - b) for Y4XX), a Y4XX sample is shifted up with zero low bits; every byte of [0, row_bytes) of every row is written and
 * NOTHING else: the bytes between row_bytes and the pitch and everything in front of and behind the buffer keep their
 * contents.
 * d_planes: three planes width x height, tightly packed one after the other, in container_bits-bit elements.
 * OJPHGPU_E_INVALID: an unknown format (the codes of sections 7b and 7c included), a null pointer, a zero size, a bit_depth
 * outside the format's column, a container narrower than bit_depth, an 8-bit container with a format that is not a byte
 * format, a pitch below row_bytes, a d_video or pitch that is not a multiple of the pixel's size (4 bytes, Y4XX: 8), row_bytes
 * beyond 32 bits.  No further alignment is required, so a pitched surface that is already in device memory is read or written
 * in place; the kernels take, per row, the widest piece its address allows.  Sections 7b and 7c refuse these codes. */
#define OJPHGPU_VIDEO_V410 0x21
#define OJPHGPU_VIDEO_Y410 0x22
#define OJPHGPU_VIDEO_R210 0x23
#define OJPHGPU_VIDEO_R10K 0x24
#define OJPHGPU_VIDEO_Y4XX 0x25
#define OJPHGPU_VIDEO_AYUV 0x26
#define OJPHGPU_VIDEO_BGRA 0x27
#define OJPHGPU_VIDEO_RGBA 0x28
#define OJPHGPU_VIDEO_ARGB 0x29
int  ojphgpu_video444_layout(int format, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* frame_bytes);   /* host only */
int  ojphgpu_unpack_video444(void* stream, int format, const void* d_video, uint32_t pitch, void* d_planes, uint32_t width,
                             uint32_t height, uint32_t bit_depth, int container_bits);
int  ojphgpu_pack_video444(void* stream, int format, const void* d_planes, void* d_video, uint32_t pitch, uint32_t width,
                           uint32_t height, int container_bits, uint32_t bit_depth);
/* The rules of sections 7b - 7d for one OJPHGPU_VIDEO_* constant, as the stages and the pipes' _set_video apply them: family,
 * chroma cell (a chroma sample covers sub_x x sub_y luma samples), depth column, narrowest container, what a video pointer and
 * a pitch must be multiples of (pitch_align 0: no pitch, rows at row_bytes).  OJPHGPU_E_INVALID: an unknown format, a null out. */
#define OJPHGPU_VIDEO_FAMILY_422 422
#define OJPHGPU_VIDEO_FAMILY_420 420
#define OJPHGPU_VIDEO_FAMILY_444 444
typedef struct ojphgpu_video_info {                  /* family: OJPHGPU_VIDEO_FAMILY_* */
  int family; uint32_t sub_x, sub_y, min_depth, max_depth, min_container_bits, pointer_align, pitch_align;
} ojphgpu_video_info;
int  ojphgpu_video_format_info(int format, ojphgpu_video_info* out);   /* host only */
/* ---- 7e. RGB <-> YCbCr 4:4:4 / 4:2:2 / 4:2:0 (kernels_colour.hip): the matrix of a video standard, the range mapping, the
 * change of depth and the halving / doubling of chroma in ONE integer pass over planar containers.  Exact integer arithmetic;
 * pipeline.colour_table / rgb_to_ycc / ycc_to_rgb state the same in numpy, entry for entry and sample for sample.
 *   The table.  (Kr, Kb) = (0.299, 0.114) BT601, (0.2126, 0.0722) BT709, (0.2627, 0.0593) BT2020 (non-constant luminance); Kg
 *   = 1 - Kr - Kb.  A signal of depth B (8 .. 16, the RGB side's and the YCbCr side's chosen independently, as their ranges
 *   are) has an offset and a span, s = 2^(B - 8): RGB or luma (0, 2^B - 1) full, (16 s, 219 s) narrow; chroma (2^(B-1), 2^B -
 *   1) full, (128 s, 224 s) narrow.  k = 16 fraction bits.
 *   FORWARD (RGB -> YCbCr): rows A = luma (Kr, Kg, Kb), Cb (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)), Cr (1 - Kr, -Kg, -Kb) / (2 (1 -
 *   Kr)); m[c][0] and m[c][2] = llround(A[c][i] * span_ycc[c] / span_rgb * 65536.0); the GREEN coefficient m[c][1] = the row's
 *   rounded total -- llround(span_ycc[0] / span_rgb * 65536.0) for luma, 0 for chroma -- minus the other two, so that every
 *   grey gives exactly mid chroma and black and white exactly the ends of the luma range; off[c] = (offset_ycc[c] << 16) -
 *   offset_rgb * (m[c][0] + m[c][1] + m[c][2]).
 *   INVERSE (YCbCr -> RGB), from the closed form: R = Y + 2 (1 - Kr) Cr, B = Y + 2 (1 - Kb) Cb, G = Y - (2 Kb (1 - Kb) / Kg) Cb
 *   - (2 Kr (1 - Kr) / Kg) Cr; each of the nine m[c][i] = llround(coef * span_rgb / span_ycc[i] * 65536.0) on its own (the two
 *   structural zeros stay 0); off[c] = (offset_rgb << 16) - sum_i m[c][i] * offset_ycc[i].
 *   lo = 0, hi = 2^(depth of the output side) - 1 both ways: super-white and sub-black survive, the container's range holds.
 *   The stages.  frame: w x h the RGB and the luma planes; fx, fy (1 | 2 each) the chroma cell, chroma planes cw x ch with cw =
 *   (w + 1) / 2 where fx == 2 (else w), ch alike; *_first: the first element of each plane in its buffer, rows tightly packed.
 *   Containers: unsigned 8 / 16 / 32 bits, either side's on its own.  All sums in 64-bit two's complement.
 *   _rgb_to_ycc: per pixel t_c = m[c] . (R, G, B).  Component c's sample (i, j) stands ON source sample (fx i, fy j) -- luma:
 *   factors 1 --: in every halved direction the taps (1, 2, 1) over t_c, indices clamped into the plane (section 5e's filter
 *   and siting, phase 0), kk = 2 per halved direction; out = clamp((acc + (off[c] << kk) + 2^(k + kk - 1)) >> (k + kk), lo[c],
 *   hi[c]), an arithmetic shift, ONE rounding.
 *   _ycc_to_rgb: chroma at luma column x of a halved direction = 2 C[x / 2] (x even), C[(x - 1) / 2] + C[min((x + 1) / 2, cw -
 *   1)] (x odd); rows alike, the product in 2-D; kk = 1 per halved direction, luma enters as Y << kk; out = clamp((m[c] . (Y',
 *   Cb', Cr') + (off[c] << kk) + 2^(k + kk - 1)) >> (k + kk), lo[c], hi[c]).  Samples are taken as they stand: one past its
 *   nominal range is not clamped first.
 *   A stage writes the samples of its three destination planes and NOTHING else.  [lo, hi] is narrowed to what the destination
 *   container holds.  Table and frame travel as kernel arguments: nothing is uploaded, nothing allocated.  OJPHGPU_COLOUR_WGS
 *   (read per call; 1 .. 65535) caps the workgroups of the launch.
 * OJPHGPU_E_INVALID: a null pointer, a factor other than 1 or 2, k != 16, lo > hi, a container that is not 8 / 16 / 32 bits, a
 * buffer not aligned to its container, w or h of 0, a source plane that overlaps a destination plane; _colour_table_make: an
 * unknown standard, direction or range, a depth outside 8 .. 16. */
#define OJPHGPU_COLOUR_BT601  601
#define OJPHGPU_COLOUR_BT709  709
#define OJPHGPU_COLOUR_BT2020 2020
#define OJPHGPU_COLOUR_FORWARD 0                     /* RGB -> YCbCr */
#define OJPHGPU_COLOUR_INVERSE 1                     /* YCbCr -> RGB */
#define OJPHGPU_COLOUR_FULL   0
#define OJPHGPU_COLOUR_NARROW 1
typedef struct ojphgpu_colour_table { int32_t m[3][3]; int64_t off[3]; int32_t lo[3], hi[3]; uint32_t k; } ojphgpu_colour_table;
typedef struct ojphgpu_colour_frame { uint32_t w, h, fx, fy; uint64_t rgb_first[3], ycc_first[3]; } ojphgpu_colour_frame;
int  ojphgpu_colour_table_make(int standard, int direction, uint32_t rgb_depth, uint32_t ycc_depth, int rgb_range, int ycc_range,
                               ojphgpu_colour_table* out);   /* host only */
int  ojphgpu_frame_rgb_to_ycc(void* stream, const void* d_rgb, int rgb_container_bits, void* d_ycc, int ycc_container_bits,
                              const ojphgpu_colour_frame* frame, const ojphgpu_colour_table* table);
int  ojphgpu_frame_ycc_to_rgb(void* stream, const void* d_ycc, int ycc_container_bits, void* d_rgb, int rgb_container_bits,
                              const ojphgpu_colour_frame* frame, const ojphgpu_colour_table* table);
/* The plan judgement of ojphgpu_enc_pipe_set_video_colour (decoding == 0) / ojphgpu_dec_pipe_set_video_colour (decoding != 0)
 * without a pipe or a device: OJPHGPU_OK or the setter's OJPHGPU_E_INVALID; a restricted plan is judged as the view it is (its
 * window's origin included).  Any of table (the one the pipe would use), frame (where the six planes stand: R, G, B one after
 * the other, Y, Cb, Cr as in the plan's frame) and frame_bytes (of the RGB buffer) may be null. */
int  ojphgpu_video_colour_fit(const ojphgpu_plan* plan, int container_bits, int decoding, int format, const ojphgpu_colour_spec* spec,
                              ojphgpu_colour_table* table, ojphgpu_colour_frame* frame, uint64_t* frame_bytes);   /* host only */

/* ---- 7f. A Y, Cb, Cr frame of one chroma format -> another (kernels_chroma.hip): 4:4:4, 4:2:2, 4:2:0 and 4:4:0 into each other
 * over planar containers, so that a pipe takes or hands back a video buffer whose chroma cell is not its plan's.  Exact integer
 * arithmetic; pipeline.rechroma_plane / rechroma_frame state the same in numpy, sample for sample.
 *   frame: w x h the luma plane; (sfx, sfy) the source's chroma cell, (dfx, dfy) the destination's, each factor 1 | 2; a chroma
 *   plane of cell (cx, cy) is ceil(w / cx) x ceil(h / cy); *_off: the first element of each plane in its buffer, rows tightly
 *   packed.  One container for both sides: 8 / 16 bits unsigned, 32 bits int32 (a decoder's planes may hold negative samples).
 *   Luma is copied.  A chroma plane, per direction with source factor s and destination factor d: s == d: the index as it is,
 *   weight 1.  d == 2 s (halved): output i stands ON source sample 2 i -- the taps (1, 2, 1) around it, indices clamped into
 *   the plane (section 5e's filter and siting, phase 0), 2 bits.  s == 2 d (doubled): _ycc_to_rgb's rule, 2 C[x / 2] (x even),
 *   C[(x - 1) / 2] + C[min((x + 1) / 2, n - 1)] (x odd), n the source length, 1 bit.  The directions are independent (one may
 *   halve while the other doubles: 4:2:2 <-> 4:4:0); the sum is the 2-D product of their taps, exact, rounded ONCE: (acc + 2^(k -
 *   1)) >> k, an arithmetic shift, k the bits of both directions; k == 0 is a copy.  No clamp: every weight is positive and they
 *   sum to 2^k, so an output lies between the smallest and the largest input.
 *   One launch for the three planes.  It writes the samples of the three destination planes and NOTHING else.  The frame
 *   travels as a kernel argument: nothing is uploaded, nothing allocated.  OJPHGPU_CHROMA_WGS (read per call; 1 .. 65535) caps
 *   the workgroups of the launch (default 2048, of 256 threads).
 * OJPHGPU_E_INVALID: a null pointer, a factor other than 1 or 2, w or h of 0, a container that is not 8 / 16 / 32 bits, a buffer
 * not aligned to its container, a source plane that overlaps a destination plane. */
#define OJPHGPU_CHROMA_COSITED 1
typedef struct ojphgpu_chroma_frame { uint32_t w, h, sfx, sfy, dfx, dfy; uint64_t src_off[3], dst_off[3]; } ojphgpu_chroma_frame;
int  ojphgpu_frame_rechroma(void* stream, const void* d_src, void* d_dst, int container_bits, const ojphgpu_chroma_frame* frame);
/* The frames of an encoder pipe are handed over as one video buffer whose chroma cell need not be the plan's: any format of
 * sections 7b - 7d except the five RGB names (BGRA / RGBA / ARGB / R210 / R10K hold R, G, B: _set_video_colour is their way), mode
 * = OJPHGPU_CHROMA_COSITED.  Two launches per frame on the compute stream behind the upload: the family's unpack into a buffer of
 * the slot sized to the FORMAT's planes, then ojphgpu_frame_rechroma into the slot's image.  Every codestream is, byte for byte,
 * the plain encode of pipeline.rechroma_frame(unpacked planes, the format's cell, the plan's cell); a byte budget, a quality
 * target and a cap combine with it as with _set_video (a target is measured against the planes in the plan's chroma format).
 * _acquire hands out the format's tight layout for the luma size.  A format whose cell IS the plan's is accepted and is exactly
 * the _set_video hand-over: one launch, no intermediate buffer.  The calling window of _set_video; excludes _set_pixels /
 * _set_packed, the plain _set_video and _set_video_colour (for the life of the pipe or until set back to planes by format 0 with
 * mode 0 or OJPHGPU_CHROMA_COSITED); those setters are unchanged.
 * OJPHGPU_E_INVALID, the pipe left as it was: an unknown format or one of the five RGB names; a mode other than
 * OJPHGPU_CHROMA_COSITED (0 only with format 0); a plan that has not exactly three unsigned components of one depth that the
 * format and the container hold, component 0 on the reference grid, components 1 and 2 sub-sampled alike by 1 or 2 each way with
 * planes of (ceil(w / fx), ceil(h / fy)), in the tight frame layout; an odd image offset in a direction where EITHER side's cell
 * is 2 (the chroma sample would stand on the cell's second luma sample: phase 1). */
int  ojphgpu_enc_pipe_set_video_chroma(ojphgpu_enc_pipe* pipe, int format, int mode);
/* The mirror: decoded frames come back as that video buffer -- ojphgpu_frame_rechroma from the slot's image into its buffer of
 * the format's planes, then the family's pack (which clamps to [0, 2^depth - 1], negative int32 samples included: a pipe with
 * 32-bit containers is accepted).  The samples enter the stage as the pipe's containers hold them.  Judged on the view's plan
 * when the pipe decodes a view: a reduced resolution always passes; a window when its x0 is even where either side's fx == 2 and
 * its y0 is even where either side's fy == 2 (with a reduced resolution too: a multiple of 2^(skip_recon + 1) there). */
int  ojphgpu_dec_pipe_set_video_chroma(ojphgpu_dec_pipe* pipe, int format, int mode);
/* The plan judgement of the two setters (decoding == 0 / != 0) without a pipe or a device: OJPHGPU_OK or the setter's
 * OJPHGPU_E_INVALID; a restricted plan is judged as the view it is.  frame (may be null): the stage's descriptor -- source and
 * destination as the pipe would launch it, the format's planes w h, then the two chroma planes, one after the other, the
 * plan's as in its frame; equal cells: both sides the plan's, which no launch uses.  buffer_bytes (may be null): of the video
 * buffer. */
int  ojphgpu_video_chroma_fit(const ojphgpu_plan* plan, int container_bits, int decoding, int format, int mode, ojphgpu_chroma_frame* frame,
                              uint64_t* buffer_bytes);   /* host only */
/* Runs of bytes scattered over a source -> the staged layout a view decoder reads (kernels_assemble.hip).  d_src: the
 * device address of the source -- mapped pinned host memory (hipHostGetDevicePointer; the kernel then reads across PCIe
 * exactly the dwords that hold the runs) or device memory -- 16-byte aligned; src_cap: the bytes of it that may be read, a
 * multiple of 4 from 16 to below 2^34 (otherwise OJPHGPU_E_INVALID).  d_runs: n entries as ojphgpu_plan_upload_runs builds
 * them, where the device can read them -- device memory for choice: every workgroup reads a window of the table per
 * 16 KB step, which from mapped host memory would cross PCIe beside the payload.  Every byte of d_dst[0, staged_len) is written: run i's bytes at dst[i], zeros everywhere else; nothing at or
 * beyond staged_len (a multiple of 64; d_dst 16-byte aligned).  Loads stay inside [0, src_cap) whatever the table holds (a
 * run that reaches beyond it is the caller's mistake: those bytes come out unspecified).  staged_len == 0: no launch. */
int  ojphgpu_gather_runs(void* stream, const void* d_src, size_t src_cap, const ojphgpu_run* d_runs, uint32_t n, void* d_dst,
                         uint64_t staged_len);
/* Codestream assembly as a stage (kernels_assemble.hip, assemble_codestream): job i copies n bytes from d_blob + src (blob
 * != 0) or d_data + src (blob == 0) to d_out + dst, one wavefront per job; source and destination are byte-aligned
 * arbitrarily.  The n bytes at dst are written and nothing else.  The kernel reads whole aligned dwords: up to 3 bytes in
 * front of a job's first byte and up to 3 behind its last, inside the dwords that hold them, so a source buffer ends on a
 * dword boundary (hipMalloc's alignment with a size that is a multiple of 4).  d_jobs: the table in device memory.  n_jobs ==
 * 0: no launch.  OJPHGPU_E_INVALID: a null d_jobs, d_blob or d_out.  Nothing is range-checked: the jobs are the caller's. */
typedef struct ojphgpu_t2_job { uint64_t dst, src; uint32_t n, blob; } ojphgpu_t2_job;
int  ojphgpu_assemble(void* stream, const ojphgpu_t2_job* d_jobs, uint32_t n_jobs, const uint8_t* d_blob, const uint8_t* d_data,
                      uint8_t* d_out);
/* The copy kernel of the pipes as a stage (copy_to_host_kernel): `bytes` bytes from d_src (device memory) to d_dst (the
 * device address of pinned host memory, or device memory), both 16-byte aligned (otherwise OJPHGPU_E_INVALID).  Exactly
 * [0, bytes) of d_dst is written.  bytes == 0: no launch.  OJPHGPU_COPY_WGS (read once per process) sets the workgroups of
 * this kernel and of ojphgpu_gather_runs. */
int  ojphgpu_copy_to_host(void* stream, void* d_dst, const void* d_src, size_t bytes);

const char* ojphgpu_version(void);

/* ---------------------------------------------------------------------------------------------
 * 8. One frame over several GPUs of the node, from one process (ojphgpu_multi.cpp)
 * ---------------------------------------------------------------------------------------------
 * Tiles are independent (every tile has an object tree of its own in the reference, ojph_codestream_local.cpp:113-180, and
 * codestream::flush writes them one after the other, ojph_tile.cpp:584-610): a tiled frame shards by contiguous runs of
 * tiles, device k of n taking tiles [k * T / n ...) -- the first T % n runs one tile longer -- with one host thread and one
 * codec object per device and NO exchange between the devices while they code.  The only meeting point is the caller's
 * thread: main header from everybody's Psot lengths, a prefix sum of the runs' lengths, and every device copies its
 * tile-parts straight to its place in the caller's buffer (encode) / its tiles' rectangles to the caller's image (decode).
 * A frame of one tile uses the first device only.  h_image: the frame as int32 planes (ojphgpu_plan_comp_info); host
 * buffers should be pinned for the copies to run at link speed.  The same device may be listed more than once. */
typedef struct ojphgpu_multi_encoder ojphgpu_multi_encoder;
typedef struct ojphgpu_multi_decoder ojphgpu_multi_decoder;
int  ojphgpu_multi_encoder_create(const ojphgpu_plan* plan, const int* devices, uint32_t num_devices, ojphgpu_multi_encoder** out);
void ojphgpu_multi_encoder_destroy(ojphgpu_multi_encoder* enc);
/* whole codestream (SOC .. EOC) into h_out; OJPHGPU_E_OVERFLOW with *out_len = the bytes needed when cap is too small */
int  ojphgpu_multi_encode(ojphgpu_multi_encoder* enc, const int32_t* h_image, uint8_t* h_out, size_t cap, size_t* out_len);
/* the same with the frame's samples in container_bits-bit containers (32 | 16 | 8, as ojphgpu_encoder_run_device16 / 8):
 * half / a quarter of the bytes over every device's link */
int  ojphgpu_multi_encode_container(ojphgpu_multi_encoder* enc, const void* h_image, int container_bits, uint8_t* h_out, size_t cap,
                                    size_t* out_len);
/* how the frame was dealt out: workers (<= num_devices, <= tiles) and the tiles of each */
int  ojphgpu_multi_encoder_workers(const ojphgpu_multi_encoder* enc, uint32_t* num_workers, uint32_t* tiles_per_worker, uint32_t cap);
/* parses the codestream once (codestream::read_headers + read, with restrict_input_resolution when the skips are not 0) */
int  ojphgpu_multi_decoder_create(const uint8_t* h_codestream, size_t len, int resilient, uint32_t skipped_res_for_data,
                                  uint32_t skipped_res_for_recon, const int* devices, uint32_t num_devices, ojphgpu_multi_decoder** out);
void ojphgpu_multi_decoder_destroy(ojphgpu_multi_decoder* dec);
int  ojphgpu_multi_decoder_plan(ojphgpu_multi_decoder* dec, const ojphgpu_plan** plan);      /* owned by the decoder */
/* the codestream the decoder was created for -> h_image; OJPHGPU_E_BLOCK when blocks failed and the decoder is not resilient */
int  ojphgpu_multi_decode(ojphgpu_multi_decoder* dec, const uint8_t* h_codestream, size_t len, int32_t* h_image, uint32_t* failed_blocks);
/* Host memory the caller got elsewhere (a shared-memory segment several processes write one codestream into, a file
 * mapping) made known to the HIP runtime this library runs on, so that copies from / to it run at link speed
 * (hipHostRegister / hipHostUnregister).  openjph_amd/shard.py HostGather: every rank of a node copies its tile-parts over
 * its own GPU's link straight to their place in ONE segment -- the gather of SURVEY 8(e) without a receiving GPU. */
int  ojphgpu_host_register(void* h_ptr, size_t bytes);
int  ojphgpu_host_unregister(void* h_ptr);
int  ojphgpu_multi_decode_container(ojphgpu_multi_decoder* dec, const uint8_t* h_codestream, size_t len, void* h_image, int container_bits,
                                    uint32_t* failed_blocks);

#ifdef __cplusplus
}
#endif
#endif /* OJPHGPU_H */
