// pt_radiance.hip -- radiance along caller-supplied rays (pt_abi.h pt_radiance_device, pt_radiance) and the
// frame kernels' camera rays as such rays (pt_camera_rays_device). Ray k = (o, d) with id (px, py) is
// taken as the camera ray of pixel (px, py) of sample sampleIndex: the ray queries' hit search
// (Tracer::trace, pt_trace_closest's result), a miss finished with the sky along d, a hit with
// finishHit and the context's integrator (pt_paths.h, the megakernel's text) from the RNG state that
// pixel holds once its camera ray exists (pt_frame.h pathSeed). out = (Le(first hit) + Li, t). So a ray
// that is bit for bit a frame's camera ray yields that frame's sample of the pixel bit for bit, in any
// order and any batch: nothing in a path depends on the image size or on the other rays. Nothing is
// counted: pt_frame_stats stays as it was.
//
// One lane per ray in a grid-stride loop, as the ray queries (pt_query.hip): no LDS copy of the top of
// the tree, the LDS stack and the queries' overflow area. What was measured, and the waves per SIMD of
// each integrator's variant: DESIGN.md 4i.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_frame.h"
#include "pt_kernels.h"
#include "pt_paths.h"
#include "pt_trace.h"

namespace pt {

constexpr int radianceWaves(int integ) {
  return integ == 0 ? PT_RADIANCE_WAVES_LAMBERT : integ == 1 ? PT_RADIANCE_WAVES_DISNEY : PT_RADIANCE_WAVES_MIS;
}

template <int INTEG, bool CULL>
__global__ __launch_bounds__(BLOCK, radianceWaves(INTEG)) void radianceKernel(RadianceParams p) {
  __shared__ int s_stack[LDS_STACK * BLOCK];
  Stack st;
  st.init(s_stack, p.ovf, p.ovfDepth);
  st.reset();
  const size_t gtid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  Counters C = {0, 0, 0, 0, 0};
  const SceneView S = noTopView(p.scene);  // no LDS copy of the top of the tree (as the ray queries, pt_query.hip)
  // (GUARD: the caller's ray is checked against the runtime tree's origin domain, traceFrom; the path's own
  // rays start on the scene)
  Tracer<CULL, false, true> tr{S, st, C, nullptr, p.originLimit};
  for (size_t k = gtid; k < (size_t)p.n; k += (size_t)gridDim.x * BLOCK) {
    const float* r = p.rays + 6 * k;
    const V3 o = v3(r[0], r[1], r[2]);
    const V3 d = v3(r[3], r[4], r[5]);
    const int px = p.ids ? p.ids[2 * k] : (int)(k & 4095);
    const int py = p.ids ? p.ids[2 * k + 1] : (int)(k >> 12);
    float t;
    const int tri = tr.traceFrom(o, d, t);
    V3 color;
    if (tri < 0) {
      color = sampleHdr(p.env, d);
      t = PT_INF;
    } else {
      uint32_t seed = pathSeed(px, py, p.sampleIndex);
      color = pathSample<INTEG>(tr, p.env, tri, o, d, t, p.maxBounce, seed, px, py, p.sampleIndex, C, false);
    }
    p.out[k] = make_float4(color.x, color.y, color.z, t);
  }
}

template <int I>
static void launchRadianceI(const RadianceParams& p, int grid, hipStream_t s, bool cull) {
  if (cull) hipLaunchKernelGGL((radianceKernel<I, true>), dim3(grid), dim3(BLOCK), 0, s, p);
  else hipLaunchKernelGGL((radianceKernel<I, false>), dim3(grid), dim3(BLOCK), 0, s, p);
}

hipError_t launchRadiance(const RadianceParams& p, int integrator, int grid, hipStream_t s, bool cull) {
  if (integrator == 0) launchRadianceI<0>(p, grid, s, cull);
  else if (integrator == 1) launchRadianceI<1>(p, grid, s, cull);
  else if (integrator == 2) launchRadianceI<2>(p, grid, s, cull);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// one lane per pixel, row-major
__global__ __launch_bounds__(BLOCK) void cameraRaysKernel(CameraRaysParams p) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (size_t)p.width * p.height) return;
  const int py = (int)(i / p.width), px = (int)(i - (size_t)py * p.width);
  uint32_t seed;
  const V3 d = cameraRay(p.cam, p.width, p.height, p.sampleIndex, px, py, seed);
  float* r = p.rays + 6 * i;
  r[0] = p.eye[0];
  r[1] = p.eye[1];
  r[2] = p.eye[2];
  r[3] = d.x;
  r[4] = d.y;
  r[5] = d.z;
  if (p.ids) {
    p.ids[2 * i] = px;
    p.ids[2 * i + 1] = py;
  }
}

hipError_t launchCameraRays(const CameraRaysParams& p, hipStream_t s) {
  const size_t n = (size_t)p.width * p.height;
  hipLaunchKernelGGL(cameraRaysKernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace pt
