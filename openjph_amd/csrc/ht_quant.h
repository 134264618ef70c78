// openjph_amd/csrc/ht_quant.h -- the quantise / de-quantise transfers of one sample, shared by the block encoder
// (kernels_ht_enc.hip), the block decoder (kernels_ht_dec.hip) and the quality search's requantise pass
// (kernels_quality.hip), which restates what the first two do to a coefficient between them: one definition, so that the
// three cannot drift apart.
#ifndef OJPHGPU_HT_QUANT_H
#define OJPHGPU_HT_QUANT_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ojphgpu {

// quantise transfer of one raw coefficient: sign | magnitude, MSB aligned.  A coefficient with more than K_max magnitude
// bits (Part-2 kernels whose gain outruns the guard bits) leaves the reference's transfer the way its 32-bit arithmetic
// has it: reversible, |v| << shift drops what does not fit and bit K_max of |v| lands on the sign position
// (ojph_codestream_gen.cpp:70-76); irreversible, the float -> int conversion of a product beyond 2^31 gives INT_MIN (what
// cvttss2si and its vector forms return for every out-of-range input, NaN included), i.e. the word 0x80000000: a zero.
// Either way that bit counts in max_val, and codeblock::encode (ojph_codeblock.cpp:142-175) codes a block whose max_val
// is not zero even when no sample of it is significant: `over` collects it.
__device__ __forceinline__ uint32_t to_sign_mag(uint32_t raw, bool reversible, uint32_t shift, float delta_inv, uint32_t& over)
{
  if (reversible) {
    const int v = (int)raw;
    const uint32_t m = (v >= 0 ? (uint32_t)v : 0u - (uint32_t)v) << shift;
    over |= m >> 31;
    return (v >= 0 ? 0u : 0x80000000u) | m;
  }
  const float f = __fmul_rn(__uint_as_float(raw), delta_inv);            // :113-118, C truncation
  const bool out = !(fabsf(f) < 2147483648.0f);
  const int t = out ? (int)0x80000000u : (int)f;
  const uint32_t m = t >= 0 ? (uint32_t)t : 0u - (uint32_t)t;
  over |= m >> 31;
  return (t >= 0 ? 0u : 0x80000000u) | m;
}

// What the cleanup pass carries of a sign-magnitude word, as the decoder hands it back: the top K_max magnitude bits
// (p = 31 - K_max, 1 <= p) and the half bit below them (ojph_block_decoder32.cpp: "2 * m + 1" placed at p - 1); a sample
// whose kept bits are all zero is not significant and comes back as the zero word, sign dropped.
__device__ __forceinline__ uint32_t coded_word(uint32_t sm, uint32_t p)
{
  const uint32_t m = (sm & 0x7FFFFFFFu) >> p;
  return m ? (sm & 0x80000000u) | (m << p) | (1u << (p - 1u)) : 0u;
}

// de-quantise transfer of one sign-magnitude word (ojph_codestream_gen.cpp:124-168)
__device__ __forceinline__ uint32_t dequantise(uint32_t val, bool rev, uint32_t shift, float delta)
{
  const uint32_t mag = val & 0x7FFFFFFFu;
  if (rev) { const uint32_t iv = mag >> shift, sg = (uint32_t)((int)val >> 31); return (iv ^ sg) - sg; }   // -iv for a set sign
  // (the product of two non-negative floats has a clear sign bit: OR-ing the sample's sign in negates it, -0.0f for a zero
  // magnitude included -- as "-fv" does)
  return __float_as_uint(__fmul_rn((float)mag, delta)) | (val & 0x80000000u);
}

}  // namespace ojphgpu
#endif
