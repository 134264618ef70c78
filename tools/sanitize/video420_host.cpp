// tools/sanitize/video420_host.cpp -- the text of kernels_video420.hip compiled for the HOST (hip_shim/ stands in for the
// HIP headers and runs a launch lane by lane) and run over the cases of video420_cases.py, built with
// -fsanitize=address,undefined: every access of the kernels inside its buffer and aligned to its width, readfirstlane only
// of wave-uniform values, and the results byte for byte those of the numpy statement.  Every buffer is an allocation of its
// exact size at the case's offset from a 256-byte boundary, so one byte beyond a plane is an error.  CPU only.
//     video420_host CASE_FILE
#include "../../openjph_amd/csrc/kernels_video420.hip"

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
  if (argc != 2) { fprintf(stderr, "usage: video420_host CASE_FILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t h[12];
  size_t cases = 0, bad = 0;
  while (fread(h, sizeof(uint32_t), 12, f) == 12) {
    const int format = (int)h[0], container = (int)h[4];
    const uint32_t width = h[1], height = h[2], depth = h[3], lp = h[5], cp = h[6];
    const std::vector<uint8_t> vin_l = blob(f, h[9]), vin_c = blob(f, h[10]), want_planes = blob(f, h[11]), src_planes = blob(f, h[11]),
                               want_l = blob(f, h[9]), want_c = blob(f, h[10]);
    ++cases;
    std::string why;
    {
      Buf l(h[7], h[9]), c(h[8], h[10]), planes(0, h[11]);
      memcpy(l.p, vin_l.data(), h[9]); memcpy(c.p, vin_c.data(), h[10]); memset(planes.p, 0x5A, h[11]);
      if (ojphgpu_unpack_video420(nullptr, format, l.p, lp, c.p, cp, planes.p, width, height, depth, container) != OJPHGPU_OK) why += " unpack refused";
      else if (memcmp(planes.p, want_planes.data(), h[11])) why += " unpack differs";
    }
    {
      Buf l(h[7], h[9]), c(h[8], h[10]), planes(0, h[11]);
      memset(l.p, 0x5A, h[9]); memset(c.p, 0x5A, h[10]); memcpy(planes.p, src_planes.data(), h[11]);
      if (ojphgpu_pack_video420(nullptr, format, planes.p, l.p, lp, c.p, cp, width, height, container, depth) != OJPHGPU_OK) why += " pack refused";
      else if (memcmp(l.p, want_l.data(), h[9]) || memcmp(c.p, want_c.data(), h[10])) why += " pack differs";
      if (!l.front_intact() || !c.front_intact()) why += " pack wrote in front of a plane";
    }
    if (!why.empty()) {
      ++bad;
      fprintf(stderr, "format 0x%x %u x %u depth %u container %d pitches %u %u offsets %u %u:%s\n", format, width, height, depth, container, lp, cp,
              h[7], h[8], why.c_str());
    }
  }
  fclose(f);
  printf("%zu cases, %zu failed\n", cases, bad);
  return bad || !cases ? 1 : 0;
}
