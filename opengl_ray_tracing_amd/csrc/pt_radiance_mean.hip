// pt_radiance_mean.hip -- many samples of the radiance query per call, folded on the GPU (pt_abi.h
// pt_radiance_mean_device, pt_radiance_mean). A lane owns ray k for all nSamples samples: sample j is
// pt_radiance.hip radianceKernel's out[k].rgb for sample index firstSample + j (the same hit search, the
// same pathSample of pt_paths.h from the same seed, so the same bits), and the lane folds it into the
// ray's running mean -- and, when asked, the luminance moments -- in registers, with the floats of
// pt_display.hip mixFrames: w = 1 / (float)(s + 1u), mixf per channel, l = (0.3 r + 0.6 g) + 0.1 b. No
// n x nSamples colour buffer: per ray one float4 and one float2 are read (firstSample != 0) and stored.
//
// Without PT_RADIANCE_RAYS_PER_SAMPLE the ray is the same for every sample: its closest hit (tri, t) is
// searched once and every sample starts from it (pathSample's finishHit), and a ray that leaves the scene
// folds its one sky colour nSamples times without a walk -- the fold still runs, mixf(c, c, w) is not
// always c. With the flag sample j's ray is rays[j * n + k], indexed in size_t.
//
// This is radianceKernel with a sample loop around pathSample: the launch shape, the stack and the tree
// are its (one lane per ray in a grid-stride loop, no LDS copy of the top of the tree, the queries'
// overflow area), and a wave is lock-step per sample. A per-lane path state machine in the manner of
// pt_regen.hip (one traversal call site, a lane starting its next sample as soon as its path ends) was
// built and measured beside it and not kept: faster where long paths fill the machine (c4), slower than
// 16 single calls on c2's per-sample rays. Both forms' figures: DESIGN.md 4i-2.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_frame.h"
#include "pt_kernels.h"
#include "pt_paths.h"
#include "pt_trace.h"

namespace pt {

// waves per SIMD: radianceKernel's, per integrator (the fold's five registers make the Lambert variant
// spill 3 VGPRs at its 128)
constexpr int radianceMeanWaves(int integ) {
  return integ == 0 ? PT_RADIANCE_WAVES_LAMBERT : integ == 1 ? PT_RADIANCE_WAVES_DISNEY : PT_RADIANCE_WAVES_MIS;
}

// A ray's running mean and moments, and mixFrames' update of them with sample s
struct MeanAcc {
  float r, g, b, m1, m2;
};
__device__ __forceinline__ void foldSample(MeanAcc& a, V3 c, uint32_t s, bool moments) {
  const float w = 1.0f / (float)(s + 1u);
  a.r = mixf(a.r, c.x, w);
  a.g = mixf(a.g, c.y, w);
  a.b = mixf(a.b, c.z, w);
  if (moments) {
    const float l = (0.3f * c.x + 0.6f * c.y) + 0.1f * c.z;
    a.m1 = mixf(a.m1, l, w);
    a.m2 = mixf(a.m2, l * l, w);
  }
}

template <int INTEG, bool CULL>
__global__ __launch_bounds__(BLOCK, radianceMeanWaves(INTEG)) void radianceMeanKernel(RadianceMeanParams p) {
  __shared__ int s_stack[LDS_STACK * BLOCK];
  Stack st;
  st.init(s_stack, p.ovf, p.ovfDepth);
  st.reset();
  const size_t gtid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  Counters C = {0, 0, 0, 0, 0};
  const SceneView S = noTopView(p.scene);  // as radianceKernel
  Tracer<CULL, false, true> tr{S, st, C, nullptr, p.originLimit};  // as radianceKernel
  for (size_t k = gtid; k < (size_t)p.n; k += (size_t)gridDim.x * BLOCK) {
    const int px = p.ids ? p.ids[2 * k] : (int)(k & 4095);
    const int py = p.ids ? p.ids[2 * k + 1] : (int)(k >> 12);
    MeanAcc a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (p.firstSample != 0u) {  // the picture goes on; a first sample does not read the buffers
      const float4 m = p.mean[k];
      a.r = m.x;
      a.g = m.y;
      a.b = m.z;
      if (p.moments) {
        const float2 mm = p.moments[k];
        a.m1 = mm.x;
        a.m2 = mm.y;
      }
    }
    V3 o = v3(0, 0, 0), d = v3(0, 0, 0), sky = v3(0, 0, 0);
    float t = PT_INF;
    int tri = -1;
    for (int j = 0; j < p.nSamples; j++) {
      const uint32_t s = p.firstSample + (uint32_t)j;
      if (j == 0 || p.perSample) {  // the sample's ray and its closest hit (a fixed ray's: once)
        const float* r = p.rays + 6 * ((p.perSample ? (size_t)j * (size_t)p.n : (size_t)0) + k);
        o = v3(r[0], r[1], r[2]);
        d = v3(r[3], r[4], r[5]);
        tri = tr.traceFrom(o, d, t);
        if (tri < 0) {
          sky = sampleHdr(p.env, d);
          t = PT_INF;
        }
      }
      V3 c = sky;
      if (tri >= 0) {
        uint32_t seed = pathSeed(px, py, s);
        c = pathSample<INTEG>(tr, p.env, tri, o, d, t, p.maxBounce, seed, px, py, s, C, false);
      }
      foldSample(a, c, s, p.moments != nullptr);
    }
    p.mean[k] = make_float4(a.r, a.g, a.b, t);
    if (p.moments) p.moments[k] = make_float2(a.m1, a.m2);
  }
}

template <int I>
static void launchRadianceMeanI(const RadianceMeanParams& p, int grid, hipStream_t s, bool cull) {
  if (cull) hipLaunchKernelGGL((radianceMeanKernel<I, true>), dim3(grid), dim3(BLOCK), 0, s, p);
  else hipLaunchKernelGGL((radianceMeanKernel<I, false>), dim3(grid), dim3(BLOCK), 0, s, p);
}

hipError_t launchRadianceMean(const RadianceMeanParams& p, int integrator, int grid, hipStream_t s, bool cull) {
  if (integrator == 0) launchRadianceMeanI<0>(p, grid, s, cull);
  else if (integrator == 1) launchRadianceMeanI<1>(p, grid, s, cull);
  else if (integrator == 2) launchRadianceMeanI<2>(p, grid, s, cull);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace pt
