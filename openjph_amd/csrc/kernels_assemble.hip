// openjph_amd/csrc/kernels_assemble.hip -- codestream assembly on the device.
//
// In the reference the packet writer copies every code-block's bytes from the elastic allocator's
// chunks into the output file behind its packet header (precinct::write, ojph_precinct.cpp:281-324:
// `file->write(cb->next_coded->buf ...)` per block).  Here the block coder leaves the blocks in HBM in
// the order their wavefronts finished; the host codes the packet headers from the block LENGTHS alone
// (ojph_t2.cpp, a layout: blob + placement jobs), and this kernel lays the codestream out in HBM --
// markers / headers from the blob, code-block bytes from the coder's output -- so that ONE device-to-host
// copy delivers the finished codestream and no coded byte passes through a host memcpy.
//
// One wavefront per placement job (a code-block is 1-4 KB: 64 lanes x 16 bytes cover 1 KB per step).
// Source and destination are byte-aligned arbitrarily: the destination is brought to 16-byte alignment
// with a bytewise head, then every lane stores 16 aligned bytes assembled from five aligned source
// dwords with v_alignbyte_b32; a bytewise tail finishes.  HBM traffic = 2 x codestream bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "ojph_plan.h"

namespace {

constexpr int WAVES = 4;

__global__ __launch_bounds__(WAVES * 64) void assemble_codestream(const ojphgpu::T2Job* __restrict__ jobs, uint32_t njobs,
                                                                   const uint8_t* __restrict__ blob, const uint8_t* __restrict__ data,
                                                                   uint8_t* __restrict__ out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t j = blockIdx.x * WAVES + wave;
  if (j >= njobs) return;
  const ojphgpu::T2Job job = jobs[j];
  const uint8_t* src = (job.blob ? blob : data) + job.src;
  uint8_t* dst = out + job.dst;
  uint32_t n = job.n;
  // head: up to 15 bytes until dst is 16-byte aligned
  uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
  if (head > n) head = n;
  if (lane < head) dst[lane] = src[lane];
  src += head; dst += head; n -= head;
  // body: 16 bytes per lane and step
  const uint32_t sh = (uint32_t)((uintptr_t)src & 3u);
  const uint32_t* s4 = (const uint32_t*)(src - sh);               // aligned dword holding src[0]
  uint4* d16 = (uint4*)dst;
  const uint32_t n16 = n >> 4;
  for (uint32_t i = lane; i < n16; i += 64) {
    const uint32_t* q = s4 + 4 * i;
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    uint4 v;
    if (sh == 0) { v.x = w0; v.y = w1; v.z = w2; v.w = w3; }
    else {
      const uint32_t w4 = q[4];                                   // within the source: src + 16 i + 16 <= end, and sh > 0
      v.x = __builtin_amdgcn_alignbyte(w1, w0, sh); v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
      v.z = __builtin_amdgcn_alignbyte(w3, w2, sh); v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
    }
    d16[i] = v;
  }
  // tail: up to 15 bytes
  const uint32_t done = n16 << 4, tail = n - done;
  if (lane < tail) dst[done + lane] = src[done + lane];
}

// Device -> pinned host memory by a kernel instead of hipMemcpyAsync: on this platform the runtime puts
// host-to-device and device-to-host copies of different streams on the SAME SDMA engine, one after the
// other (measured, profiles/r02_c_pipeline_timeline.txt: the next frame's 3.5 ms upload waited for the
// previous frame's 1.3 ms download), which cost the encode pipeline a third of its frame rate (5.6 -> 3.95 ms
// per 8K frame).  Stores from a kernel go over PCIe as posted writes beside the SDMA upload.  The grid is
// small: the copy is PCIe-bound (55 GB/s alone, ~47 GB/s beside an upload) and 8 workgroups walking
// contiguous segments were the fastest of 8 / 16 / 32 / 64 / 128 / 512 (profiles/r02_d_copy_modes.txt);
// the CUs stay with the next frame's kernels.
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void copy_to_host_kernel(v4u* __restrict__ dst, const v4u* __restrict__ src, size_t n16, size_t seg,
                                                            uint8_t* __restrict__ dst_tail, const uint8_t* __restrict__ src_tail, uint32_t tail)
{
  // every workgroup walks ONE contiguous segment front to back, 16 KB (4 x 16 bytes per lane) per step: the
  // host sees a few sequential write streams of full-size PCIe payloads
  const size_t lo = (size_t)blockIdx.x * seg, hi = lo + seg < n16 ? lo + seg : n16;
  size_t i = lo + threadIdx.x;
  for (; i + 768 < hi; i += 1024) {
    const v4u a = src[i], b = src[i + 256], c = src[i + 512], d = src[i + 768];
    __builtin_nontemporal_store(a, &dst[i]); __builtin_nontemporal_store(b, &dst[i + 256]);
    __builtin_nontemporal_store(c, &dst[i + 512]); __builtin_nontemporal_store(d, &dst[i + 768]);
  }
  for (; i < hi; i += 256) { const v4u a = src[i]; __builtin_nontemporal_store(a, &dst[i]); }
  if (blockIdx.x == 0 && threadIdx.x < tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}

// The upload of a VIEW (reduced resolution, a window): the bytes a frame's decoder needs are runs of code-blocks scattered
// over a codestream that lies in mapped pinned memory; this kernel reads them across PCIe and lays the staged bytes out in
// HBM -- run i at dst_i (64-byte aligned, 64 zero bytes either side), zeros everywhere else -- so that no host pass gathers
// them and only the view's bytes cross the link.  The work is split over the DESTINATION as in copy_to_host_kernel: a few
// workgroups, each walking one contiguous segment in steps of 16 KB, a lane writing four aligned 16-byte pieces per step.
// A piece meets at most one run (runs start on 64-byte boundaries, 64 bytes apart at least): the last one that starts at or
// before it, found
//   * in the table (device memory in the pipes, which copy it there first: a workgroup reads a window of up to 6 KB of it
//     per 16 KB step, too much to fetch across PCIe beside the payload) once per workgroup by a binary search, then carried from step to step: every thread loads one entry of the window [cur, cur + 256) -- a step holds 129 run
//     starts at the most -- and the count of those starting up to the step's end moves `cur`; the next step's window is
//     requested before this step's data, so both are in flight together;
//   * per piece among the step's entries, in LDS (no trip at all when the step lies in one run).
// The source is arbitrary in alignment: a lane loads the four aligned dwords that hold its first byte (one dwordx4, so that
// every source byte crosses the link once), takes the fifth from its neighbour's load -- or from a load of its own where
// the neighbour does not continue it; the other lanes aim that load at one common dword -- and shifts with v_alignbyte.
// Loads are issued unconditionally from addresses clamped into [0, src_cap): bytes behind a run's end, and the whole
// piece where there is none, are selected to zero when the registers are consumed.  Whatever the table holds, nothing
// outside the source is read and nothing outside [0, staged_len) is written.
struct GatherRun { uint64_t src, dst, n; };        // = ojphgpu_run
typedef v4u v4u_a4 __attribute__((aligned(4)));

__global__ __launch_bounds__(256) void gather_runs_kernel(const GatherRun* __restrict__ runs, uint32_t nruns, const uint32_t* __restrict__ src,
                                                          uint32_t ndw, v4u* __restrict__ dst, size_t n16, size_t seg)
{
  __shared__ uint64_t s_src[2][256], s_dst[2][256], s_n[2][256];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const size_t lo = (size_t)blockIdx.x * seg, hi = lo + seg < n16 ? lo + seg : n16;
  if (lo >= hi) return;
  uint32_t cur = 0;                                               // the last run starting at or before the segment (0: none does)
  for (uint32_t cnt = nruns; cnt > 1;) {
    const uint32_t half = cnt >> 1;
    if (runs[cur + half].dst <= (uint64_t)lo * 16u) cur += half;
    cnt -= half;
  }
  auto entry = [&](uint32_t first, bool& ok) { const uint32_t i = first + tid; ok = i < nruns; return runs[ok ? i : nruns - 1u]; };
  bool ok; GatherRun e = entry(cur, ok);
  uint32_t sel = 0;
  for (size_t base = lo; base < hi; base += 1024, sel ^= 1u) {
    s_src[sel][tid] = e.src; s_dst[sel][tid] = ok ? e.dst : ~0ull; s_n[sel][tid] = e.n;
    const uint32_t c = (uint32_t)__syncthreads_count(ok && e.dst <= (uint64_t)(base + 1024) * 16u);   // starts up to the step's end
    cur += (c ? c : 1u) - 1u;
    e = entry(cur, ok);                                           // the next step's window
    v4u L[4]; uint32_t W[4], sh[4], d[4], m[4]; bool own[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t i = base + tid + 256u * j;
      const uint64_t p = (uint64_t)(i < hi ? i : hi - 1) * 16u;
      uint32_t k = 0;
      for (uint32_t cnt = c; cnt > 1;) {                          // (c is the workgroup's: no divergence)
        const uint32_t half = cnt >> 1;
        if (s_dst[sel][k + half] <= p) k += half;
        cnt -= half;
      }
      const uint64_t rs = s_src[sel][k], rd = s_dst[sel][k], rn = s_n[sel][k];
      const uint64_t off = p - rd;                                // (p < rd, before the first run: wraps, >= rn)
      m[j] = off < rn ? (uint32_t)(rn - off < 16u ? rn - off : 16u) : 0u;
      const uint64_t a = rs + (off < rn ? off : 0u);
      const uint32_t q = (uint32_t)((a >> 2) < ndw ? (a >> 2) : ndw);          // the dword holding the piece's first byte
      const uint32_t b = q < ndw - 4u ? q : ndw - 4u;             // where the four dwords are loaded from
      sh[j] = (uint32_t)a & 3u; d[j] = q - b;
      own[j] = lane == 63u || (uint32_t)__shfl_down((int)b, 1) != q + 4u;
      const uint32_t xi = own[j] ? (q + 4u < ndw ? q + 4u : ndw - 1u) : (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
      L[j] = *(const v4u_a4*)(src + b);
      W[j] = src[xi];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t i = base + tid + 256u * j;
      uint32_t x0 = L[j].x, x1 = L[j].y, x2 = L[j].z, x3 = L[j].w;
      const uint32_t nb = (uint32_t)__shfl_down((int)x0, 1);
      uint32_t x4 = own[j] ? W[j] : nb;
      if (d[j]) {                                                 // the last dwords of the source: the load was moved down
        x4 = 0;
        if (d[j] & 1u) { x0 = x1; x1 = x2; x2 = x3; x3 = 0; }
        if (d[j] & 2u) { x0 = x2; x1 = x3; x2 = 0; x3 = 0; }
        if (d[j] & 4u) { x0 = 0; x1 = 0; x2 = 0; x3 = 0; }
      }
      const uint32_t w[4] = { __builtin_amdgcn_alignbyte(x1, x0, sh[j]), __builtin_amdgcn_alignbyte(x2, x1, sh[j]),
                              __builtin_amdgcn_alignbyte(x3, x2, sh[j]), __builtin_amdgcn_alignbyte(x4, x3, sh[j]) };
      v4u v;
#pragma unroll
      for (int t = 0; t < 4; ++t) {                               // bytes at and behind the run's end are zeros
        const uint32_t have = m[j] > 4u * t ? m[j] - 4u * t : 0u;
        v[t] = have >= 4u ? w[t] : (w[t] & ((1u << (8u * have)) - 1u));
      }
      if (i < hi) dst[i] = v;
    }
  }
}

// byte counter + overflow flag of the block coder (device words) -> two words of pinned host memory
__global__ void publish_words_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n)
{
  if (threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
}

}  // namespace

namespace ojphgpu {

// workgroups of the kernels that move bytes across PCIe (see copy_to_host_kernel)
static unsigned copy_workgroups()
{
  static const unsigned n = [] { const char* e = getenv("OJPHGPU_COPY_WGS"); const long v = e ? atol(e) : 0; return v > 0 && v <= 4096 ? (unsigned)v : 8u; }();
  return n;
}

// src: device memory, 16-byte aligned; d_dst: the DEVICE address of pinned host memory (hipHostGetDevicePointer), 16-byte aligned
int copy_to_host_launch(void* stream, void* d_dst, const void* src, size_t bytes)
{
  if (bytes == 0) return OJPHGPU_OK;
  if (!d_dst || !src || (((uintptr_t)d_dst | (uintptr_t)src) & 15u)) return OJPHGPU_E_INVALID;
  const size_t n16 = bytes >> 4; const uint32_t tail = (uint32_t)(bytes & 15u);
  const unsigned max_blocks = copy_workgroups();
  size_t seg = (n16 + max_blocks - 1) / max_blocks;
  seg = std::max<size_t>((seg + 1023) & ~(size_t)1023, 1024);   // whole 16 KB steps (fewer than 16 bytes: the tail alone, one workgroup)
  const unsigned blocks = (unsigned)std::max<size_t>(1, (n16 + seg - 1) / seg);
  hipLaunchKernelGGL(copy_to_host_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (v4u*)d_dst, (const v4u*)src, n16, seg,
                     (uint8_t*)d_dst + (n16 << 4), (const uint8_t*)src + (n16 << 4), tail);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

// d_src: the device address of the source (pinned host memory, or device memory), 16-byte aligned, src_cap bytes of it
// readable (a multiple of 4, from 16 to below 2^34: the kernel counts the source in 32-bit dword indices); d_runs: the table where the kernel can read it; d_dst: 16-byte aligned
int gather_runs_launch(void* stream, const void* d_src, size_t src_cap, const void* d_runs, uint32_t nruns, void* d_dst, uint64_t staged_len)
{
  if (staged_len == 0) return OJPHGPU_OK;
  if (!d_src || !d_dst || (nruns && !d_runs) || (((uintptr_t)d_src | (uintptr_t)d_dst) & 15u) || ((uintptr_t)d_runs & 7u) || (staged_len & 63u) ||
      (src_cap & 3u) || src_cap < 16 || src_cap >= ((size_t)1 << 34)) return OJPHGPU_E_INVALID;
  if (nruns == 0) return hipMemsetAsync(d_dst, 0, (size_t)staged_len, (hipStream_t)stream) == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
  const size_t n16 = (size_t)(staged_len >> 4);
  const unsigned max_blocks = copy_workgroups();
  size_t seg = (n16 + max_blocks - 1) / max_blocks;
  seg = (seg + 1023) & ~(size_t)1023;                        // whole 16 KB steps
  const unsigned blocks = (unsigned)((n16 + seg - 1) / seg);
  hipLaunchKernelGGL(gather_runs_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const GatherRun*)d_runs, nruns, (const uint32_t*)d_src,
                     (uint32_t)(src_cap >> 2), (v4u*)d_dst, n16, seg);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

int publish_words_launch(void* stream, uint32_t* d_dst, const uint32_t* src, uint32_t n)
{
  if (!d_dst || !src || n > 64) return OJPHGPU_E_INVALID;
  hipLaunchKernelGGL(publish_words_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_dst, src, n);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

int assemble_launch(void* stream, const T2Job* d_jobs, uint32_t njobs, const uint8_t* d_blob, const uint8_t* d_data, uint8_t* d_out)
{
  if (njobs == 0) return OJPHGPU_OK;
  if (!d_jobs || !d_blob || !d_out) return OJPHGPU_E_INVALID;
  hipLaunchKernelGGL(assemble_codestream, dim3((njobs + WAVES - 1) / WAVES), dim3(WAVES * 64), 0, (hipStream_t)stream,
                     d_jobs, njobs, d_blob, d_data, d_out);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

}  // namespace ojphgpu

static_assert(sizeof(ojphgpu_run) == sizeof(GatherRun), "ojphgpu_run is the kernel's table entry");

extern "C" int ojphgpu_gather_runs(void* stream, const void* d_src, size_t src_cap, const ojphgpu_run* d_runs, uint32_t n, void* d_dst, uint64_t staged_len)
{
  return ojphgpu::gather_runs_launch(stream, d_src, src_cap, d_runs, n, d_dst, staged_len);
}

static_assert(sizeof(ojphgpu_t2_job) == sizeof(ojphgpu::T2Job) && offsetof(ojphgpu_t2_job, dst) == offsetof(ojphgpu::T2Job, dst) &&
              offsetof(ojphgpu_t2_job, src) == offsetof(ojphgpu::T2Job, src) && offsetof(ojphgpu_t2_job, n) == offsetof(ojphgpu::T2Job, n) &&
              offsetof(ojphgpu_t2_job, blob) == offsetof(ojphgpu::T2Job, blob), "ojphgpu_t2_job is the kernel's placement job");

extern "C" int ojphgpu_assemble(void* stream, const ojphgpu_t2_job* d_jobs, uint32_t n_jobs, const uint8_t* d_blob, const uint8_t* d_data, uint8_t* d_out)
{
  return ojphgpu::assemble_launch(stream, reinterpret_cast<const ojphgpu::T2Job*>(d_jobs), n_jobs, d_blob, d_data, d_out);
}

extern "C" int ojphgpu_copy_to_host(void* stream, void* d_dst, const void* d_src, size_t bytes)
{
  return ojphgpu::copy_to_host_launch(stream, d_dst, d_src, bytes);
}
