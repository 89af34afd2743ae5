/*
 * pt_rgbe.h -- one texel rounded to the RGBE texel a Radiance file would hold (PT_ENV_RGBE of
 * pt_update_env, pt_abi.h): the same function in the HIP kernel (pt_envupdate.hip) and on the host
 * (tests/native/env_quantise_check.cpp). tests/env_update_ref.py restates it in float32 numpy.
 *
 *   c     -> c > 0 ? min(c, 255 * 2^119) : 0   per channel: negative values, -0 and NaN become 0,
 *                                              +inf the largest RGBE value
 *   mx     = the largest channel; mx < 1e-32f gives a black texel (Radiance's writer threshold)
 *   E      = exponent(mx) + 128, mx = f * 2^exponent with f in [0.5, 1): 22 .. 255
 *   c     -> floor(c * 2^(136 - E)) * 2^(E - 136)
 *   ... and black again if that leaves the largest channel below 1e-32f: 1e-32f lies between the RGBE
 *   values 207 and 208 * 2^-114, so the threshold holds for what is stored -- the smallest texel kept
 *   is 208 * 2^-114 -- and quantising twice changes nothing
 *
 * Both scalings are by normal powers of two (2^-119 .. 2^114 and back) and every product is exact: the
 * result is what pt_device.h decodeHdr8 decodes from the bytes (m_r, m_g, m_b, E), so a quantised
 * texel passes envCompactKernel's round-trip test, and quantising twice changes nothing. Only IEEE
 * compares, multiplies and floorf: the CPU and the GPU give the same bits.
 *
 * Usable from C++ and HIP device code.
 */
#ifndef PT_RGBE_H
#define PT_RGBE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PT_RGBE_FN static inline __host__ __device__ __attribute__((always_inline))
#else
#define PT_RGBE_FN static inline
#endif

#define PT_RGBE_MAX 0x1.fep+126f /* 255 * 2^119: E = 255, mantissa 255 */
#define PT_RGBE_MIN 1e-32f

PT_RGBE_FN float pt_rgbe_pow2(int e) { /* 2^e, e in -126 .. 127 */
  const uint32_t u = (uint32_t)(e + 127) << 23;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

PT_RGBE_FN void pt_rgbe_quantise(float* r, float* g, float* b) {
  float c0 = *r > 0.0f ? (*r < PT_RGBE_MAX ? *r : PT_RGBE_MAX) : 0.0f;
  float c1 = *g > 0.0f ? (*g < PT_RGBE_MAX ? *g : PT_RGBE_MAX) : 0.0f;
  float c2 = *b > 0.0f ? (*b < PT_RGBE_MAX ? *b : PT_RGBE_MAX) : 0.0f;
  float mx = c0 > c1 ? c0 : c1;
  mx = mx > c2 ? mx : c2;
  if (mx < PT_RGBE_MIN) {
    *r = *g = *b = 0.0f;
    return;
  }
  uint32_t u;
  __builtin_memcpy(&u, &mx, 4);
  const int E = (int)(u >> 23) + 2; /* mx is a normal float: frexp's exponent is the biased one - 126 */
  const float up = pt_rgbe_pow2(136 - E), down = pt_rgbe_pow2(E - 136);
  if (floorf(mx * up) * down < PT_RGBE_MIN) { /* 1e-32f itself is no RGBE value: see above */
    *r = *g = *b = 0.0f;
    return;
  }
  *r = floorf(c0 * up) * down;
  *g = floorf(c1 * up) * down;
  *b = floorf(c2 * up) * down;
}

#endif
