// tools/sanitize/video444_host.cpp -- the text of kernels_video444.hip compiled for the HOST (hip_shim/ stands in for the
// HIP headers and runs a launch lane by lane) and run over the cases of video444_cases.py, built with
// -fsanitize=address,undefined: every access of the kernels inside its buffer and aligned to its width, readfirstlane only
// of wave-uniform values, and the results byte for byte those of the numpy statement.  Every buffer is an allocation of its
// exact size at the case's offset from a 256-byte boundary, so one byte beyond the buffer is an error.  CPU only.
//     video444_host CASE_FILE
#include "../../openjph_amd/csrc/kernels_video444.hip"

#include <string.h>
#include <string>

namespace {

struct Buf {                       // `size` bytes that start `off` bytes behind a 256-byte boundary and end where the allocation ends
  uint8_t* base = nullptr; uint8_t* p = nullptr; size_t off, size;
  Buf(size_t off_, size_t size_) : off(off_), size(size_)
  {
    if (posix_memalign((void**)&base, 256, off + size)) abort();
    memset(base, 0xC3, off);
    p = base + off;
  }
  ~Buf() { free(base); }
  bool front_intact() const { for (size_t i = 0; i < off; ++i) if (base[i] != 0xC3) return false; return true; }
};

std::vector<uint8_t> blob(FILE* f, size_t n)
{
  std::vector<uint8_t> v(n);
  if (n && fread(v.data(), 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
  return v;
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: video444_host CASE_FILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t h[9];
  size_t cases = 0, bad = 0;
  while (fread(h, sizeof(uint32_t), 9, f) == 9) {
    const int format = (int)h[0], container = (int)h[4];
    const uint32_t width = h[1], height = h[2], depth = h[3], pitch = h[5];
    const std::vector<uint8_t> vin = blob(f, h[7]), want_planes = blob(f, h[8]), src_planes = blob(f, h[8]), want_v = blob(f, h[7]);
    ++cases;
    std::string why;
    {
      Buf v(h[6], h[7]), planes(0, h[8]);
      memcpy(v.p, vin.data(), h[7]); memset(planes.p, 0x5A, h[8]);
      if (ojphgpu_unpack_video444(nullptr, format, v.p, pitch, planes.p, width, height, depth, container) != OJPHGPU_OK) why += " unpack refused";
      else if (memcmp(planes.p, want_planes.data(), h[8])) why += " unpack differs";
    }
    {
      Buf v(h[6], h[7]), planes(0, h[8]);
      memset(v.p, 0x5A, h[7]); memcpy(planes.p, src_planes.data(), h[8]);
      if (ojphgpu_pack_video444(nullptr, format, planes.p, v.p, pitch, width, height, container, depth) != OJPHGPU_OK) why += " pack refused";
      else if (memcmp(v.p, want_v.data(), h[7])) why += " pack differs";
      if (!v.front_intact()) why += " pack wrote in front of the buffer";
    }
    if (!why.empty()) {
      ++bad;
      fprintf(stderr, "format 0x%x %u x %u depth %u container %d pitch %u offset %u:%s\n", format, width, height, depth, container, pitch, h[6], why.c_str());
    }
  }
  fclose(f);
  printf("%zu cases, %zu failed\n", cases, bad);
  return bad || !cases ? 1 : 0;
}
