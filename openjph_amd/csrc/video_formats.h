// openjph_amd/csrc/video_formats.h -- the ONE table of the video formats' rules (ojphgpu.h sections 7b - 7d): family and chroma
// cell, depth column, smallest container, the alignment of a video pointer and of a pitch, the layout of a row.  Host code only:
// the three stage files (kernels_video*.hip) and the pipes' hand-over (ojphgpu_pipe.cpp) judge a call with it.
#pragma once
#include <stdint.h>
#include "../../include/ojphgpu.h"

// r: what ojphgpu_video_format_info hands out; a row is unit_bytes per unit_pixels, row_bytes = unit_bytes * ceil(width / unit_pixels)
struct VideoDesc { int format; ojphgpu_video_info r; uint32_t unit_bytes, unit_pixels; };

// format (of `family`, when one is named) -> its rules, or null
inline const VideoDesc* video_desc(int format, int family = 0)
{
  enum { F422 = OJPHGPU_VIDEO_FAMILY_422, F420 = OJPHGPU_VIDEO_FAMILY_420, F444 = OJPHGPU_VIDEO_FAMILY_444 };
  static const VideoDesc table[] = {       // family cell   depths  container  pointer pitch   row: bytes per pixels
    { OJPHGPU_VIDEO_UYVY, { F422, 2, 1,   1, 8,   8,         16, 0 },   4, 2 },      // (4:2:2 takes no pitch: rows at row_bytes)
    { OJPHGPU_VIDEO_YUY2, { F422, 2, 1,   1, 8,   8,         16, 0 },   4, 2 },
    { OJPHGPU_VIDEO_V210, { F422, 2, 1,   1, 10,  16,        16, 0 },   128, 48 },   // (a v210 field is 10 bits whatever the depth says)
    { OJPHGPU_VIDEO_Y2XX, { F422, 2, 1,   9, 16,  16,        16, 0 },   8, 2 },
    { OJPHGPU_VIDEO_NV12, { F420, 2, 2,   1, 8,   8,         2, 2 },    2, 2 },      // pointers and pitches: a chroma pair
    { OJPHGPU_VIDEO_NV21, { F420, 2, 2,   1, 8,   8,         2, 2 },    2, 2 },
    { OJPHGPU_VIDEO_P0XX, { F420, 2, 2,   9, 16,  16,        4, 4 },    4, 2 },
    { OJPHGPU_VIDEO_V410, { F444, 1, 1,   1, 10,  16,        4, 4 },    4, 1 },      // pointer and pitch: a pixel
    { OJPHGPU_VIDEO_Y410, { F444, 1, 1,   1, 10,  16,        4, 4 },    4, 1 },
    { OJPHGPU_VIDEO_R210, { F444, 1, 1,   1, 10,  16,        4, 4 },    4, 1 },
    { OJPHGPU_VIDEO_R10K, { F444, 1, 1,   1, 10,  16,        4, 4 },    4, 1 },
    { OJPHGPU_VIDEO_Y4XX, { F444, 1, 1,   9, 16,  16,        8, 8 },    8, 1 },
    { OJPHGPU_VIDEO_AYUV, { F444, 1, 1,   1, 8,   8,         4, 4 },    4, 1 },
    { OJPHGPU_VIDEO_BGRA, { F444, 1, 1,   1, 8,   8,         4, 4 },    4, 1 },
    { OJPHGPU_VIDEO_RGBA, { F444, 1, 1,   1, 8,   8,         4, 4 },    4, 1 },
    { OJPHGPU_VIDEO_ARGB, { F444, 1, 1,   1, 8,   8,         4, 4 },    4, 1 },
  };
  for (const VideoDesc& d : table) if (d.format == format && (family == 0 || d.r.family == family)) return &d;
  return nullptr;
}

// The tight layout of a frame: rows at row_bytes; 4:2:0: the chroma plane's ceil(height / 2) rows behind the luma plane's, at
// chroma_offset (else 0).  false: no format, a zero size, row_bytes or the rows of both planes beyond 32 bits.
inline bool video_layout(const VideoDesc* d, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* chroma_offset, uint64_t* frame_bytes)
{
  if (!d || width == 0 || height == 0) return false;
  const uint64_t rb = d->unit_bytes * (((uint64_t)width + d->unit_pixels - 1) / d->unit_pixels);
  const uint64_t ch = d->r.family == OJPHGPU_VIDEO_FAMILY_420 ? ((uint64_t)height + 1) / 2 : 0;
  if (rb > 0xFFFFFFFFull || height + ch > 0xFFFFFFFFull) return false;
  *row_bytes = (uint32_t)rb; *chroma_offset = ch ? rb * height : 0; *frame_bytes = rb * (height + ch);
  return true;
}

// What every stage and both _set_video setters refuse alike: no format, a zero size, a depth outside the format's column, a
// container that is not 8, 16 or 32 bits, narrower than the depth or narrower than the format takes.
inline bool video_check(const VideoDesc* d, uint32_t width, uint32_t height, uint32_t bit_depth, int container_bits)
{
  if (!d || width == 0 || height == 0 || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return false;
  return bit_depth >= d->r.min_depth && bit_depth <= d->r.max_depth && (uint32_t)container_bits >= bit_depth && (uint32_t)container_bits >= d->r.min_container_bits;
}
