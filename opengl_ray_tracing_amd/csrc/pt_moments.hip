// pt_moments.hip -- the running-mean update of a PT_FLAG_MOMENTS context (pt_abi.h): mixKernel
// (pt_kernels.hip) plus the running means of the sample luminance l and of l * l, kept per pixel in
// a float2 plane (m1, m2). Same loop over the batch's frames, one pixel per lane, the same weights
// and the same mixf as the colour, so the accumulation equals a plain context's bit for bit.
// tests/variance_ref.py (moments_update) is the specification: l = (0.3 r + 0.6 g) + 0.1 b is
// tonemapPixel's luminance, one f32 operation each (no fused multiply-add).
//
// Per pixel and launch: 32 B of accumulation and 16 B of moments (read + written once each, streaming
// like the accumulation) and 12 B per frame of sample colour.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

__global__ void mixMomentsKernel(PackParams p, float4* accum, float2* moments, const float* col, size_t colStride,
                                 int nFrames, uint32_t frameCounter) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  if (!packedPixel(p, k, px, py)) return;
  const size_t i = (size_t)py * p.width + px;
  float4 a = ldStream(accum + i);
  float2 m = ldStream(moments + i);
  for (int f = 0; f < nFrames; f++) {
    const float3 c = ldCol(col + ((size_t)f * colStride + k) * COL_F);  // slot k of the share (shareIndex)
    const float w = 1.0f / (float)(frameCounter + (uint32_t)f + 1u);
    a = make_float4(mixf(a.x, c.x, w), mixf(a.y, c.y, w), mixf(a.z, c.z, w), 1.0f);
    const float l = (0.3f * c.x + 0.6f * c.y) + 0.1f * c.z;
    m = make_float2(mixf(m.x, l, w), mixf(m.y, l * l, w));
  }
  stStream(accum + i, a);
  stStream(moments + i, m);
}

hipError_t launchMixMoments(const PackParams& p, float4* accum, float2* moments, const float* col, size_t colStride,
                            int nFrames, uint32_t frameCounter, hipStream_t s) {
  if (p.count <= 0 || nFrames <= 0) return hipSuccess;
  hipLaunchKernelGGL(mixMomentsKernel, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, moments, col,
                     colStride, nFrames, frameCounter);
  return hipGetLastError();
}

}  // namespace pt
