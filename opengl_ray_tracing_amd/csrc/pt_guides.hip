// pt_guides.hip -- guide buffers of the camera's first hit (pt_abi.h pt_render_guides): for every
// pixel of the frame the camera ray through the pixel centre (pt_frame.h cameraDir, the frame
// kernels' ray with the jitter terms 0), the ray queries' hit search (Tracer::trace: the runtime's tree,
// results checked against the reference's, reference tie rules) and the integrators' hit record
// (finishHit). One lane per pixel, one wave per 8x8 tile; the waves of a resident grid walk the
// tiles in a grid-stride loop, so the traversal stack's overflow area is bounded by the grid.
// Nothing is counted: pt_frame_stats stays as it was. tests/denoise_ref.py restates the ray and
// the hit record operation by operation.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_frame.h"
#include "pt_kernels.h"
#include "pt_trace.h"

namespace pt {

template <bool CULL>
__global__ __launch_bounds__(BLOCK) void guidesKernel(GuideParams p) {
  __shared__ int s_stack[LDS_STACK * BLOCK];
  Stack st;
  st.init(s_stack, p.ovf, p.ovfDepth);
  Counters C = {0, 0, 0, 0, 0};
  const SceneView S = noTopView(p.scene);  // no LDS copy of the top of the tree (as the ray queries, pt_query.hip)
  Tracer<CULL, false> tr{S, st, C, nullptr};
  const int W = p.width, H = p.height;
  const int tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
  const int numTiles = tilesX * tilesY;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WAVES = BLOCK / 64;
  const V3 o = v3(p.eye[0], p.eye[1], p.eye[2]);
  for (int tile = blockIdx.x * WAVES + wave; tile < numTiles; tile += gridDim.x * WAVES) {
    const int ty = tile / tilesX, tx = tile - ty * tilesX;
    const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
    if (px >= W || py >= H) continue;
    const V3 d = cameraDir(p.cam, W, H, px, py, 0.0f, 0.0f);  // IS:846-850 with ax = ay = 0
    float t;
    const int tri = tr.trace(o, d, t);
    float4 a = make_float4(0.0f, 0.0f, 0.0f, PT_INF);
    float4 b = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tri >= 0) {
      Hit h;
      finishHit(S, tri, o, d, t, h);
      a = make_float4(h.P.x, h.P.y, h.P.z, t);
      b = make_float4(h.N.x, h.N.y, h.N.z, __int_as_float(tri));
      c = make_float4(h.m.baseColor.x, h.m.baseColor.y, h.m.baseColor.z, 1.0f);
    }
    const size_t i = (size_t)py * W + px;
    p.posT[i] = a;
    p.nrmTri[i] = b;
    p.albedo[i] = c;
  }
}

hipError_t launchGuides(const GuideParams& p, int grid, hipStream_t s, bool cull) {
  if (cull) hipLaunchKernelGGL((guidesKernel<true>), dim3(grid), dim3(BLOCK), 0, s, p);
  else hipLaunchKernelGGL((guidesKernel<false>), dim3(grid), dim3(BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace pt
