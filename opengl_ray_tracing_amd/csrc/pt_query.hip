// pt_query.hip -- the ray queries (pt_abi.h pt_trace_closest, pt_trace_closest_device,
// pt_trace_occluded_device and their host forms): for ray k with bound b = tmax[k] (none: PT_INF) the
// closest hit below b, or whether there is one. With (t*, tri*) the unbounded query's result for the ray
// (pt_trace_closest: the reference traversal's winner under the reference tie rules), the answer is
// (t*, tri*) / 1 when tri* >= 0 && t* < b and the miss values / 0 otherwise (tests/query_ref.py). A
// walk whose closest-hit bound starts at b gives exactly that -- a triangle at or beyond b cannot win,
// and among the others the same least-t, first-in-order one does -- so the kernel runs the frames'
// hit search (Tracer) with the walks' BOUNDED switch: the runtime's tree checked against the
// reference's (refReachable), or the uploaded tree alone -- per ray for an origin outside the runtime
// tree's origin domain (Tracer's GUARD; pt_kernels.h originInDomain). A ray with !(b > 0.0005f) -- hitTriangle's
// own lower bound, and a NaN -- is a miss without a walk. Nothing is counted: pt_frame_stats stays as it was.
//
// One lane per ray in a grid-stride loop. A loop that refills a wave's finished lanes with
// the next rays (the resumable 4-wide walk, walk4Run, a claim of 512 rays per wave and atomic) was tried
// for the any-hit and short-range rays, which finish at very different times, and measured about half
// the plain loop's rate on every case: not kept (profiles/r14/queries.json).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_trace.h"

namespace pt {

// ray k's bound: a bound past PT_INF admits nothing more (the unbounded query accepts only t < PT_INF); a
// NaN stays one (no fminf, which would drop it), and fails the callers' b > 0.0005f
__device__ __forceinline__ float loadBound(const QueryParams& p, size_t k) {
  const float b = p.tmax ? p.tmax[k] : PT_INF;
  return b > PT_INF ? PT_INF : b;
}
__device__ __forceinline__ void loadRay(const QueryParams& p, size_t k, V3& o, V3& d, float& b) {
  const float* r = p.rays + 6 * k;
  o = v3(r[0], r[1], r[2]);
  d = v3(r[3], r[4], r[5]);
  b = loadBound(p, k);
}
template <bool OCCLUDED>
__device__ __forceinline__ void storeResult(const QueryParams& p, size_t k, int tri, float t) {
  if (OCCLUDED) {
    p.occ[k] = tri >= 0 ? 1 : 0;
  } else {
    p.t[k] = tri >= 0 ? t : PT_INF;
    p.tri[k] = tri >= 0 ? tri : -1;
  }
}

template <bool OCCLUDED, bool CULL>
__global__ __launch_bounds__(BLOCK) void queryKernel(QueryParams p) {
  __shared__ int s_stack[LDS_STACK * BLOCK];
  Stack st;
  st.init(s_stack, p.ovf, p.ovfDepth);
  const size_t gtid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  Counters C = {0, 0, 0, 0, 0};
  const SceneView S = noTopView(p.scene);
  // (GUARD: a ray from outside the runtime tree's origin domain walks the uploaded tree alone)
  Tracer<CULL, false, true> tr{S, st, C, nullptr, p.originLimit};
  for (size_t k = gtid; k < (size_t)p.n; k += (size_t)gridDim.x * BLOCK) {
    V3 o, d;
    float b;
    loadRay(p, k, o, d, b);
    float t = PT_INF;
    int tri = -1;
    if (b > 0.0005f) {
      if (OCCLUDED) tri = tr.occludedBounded(o, d, b) ? 0 : -1;
      else tri = tr.traceBounded(o, d, b, t);
    }
    storeResult<OCCLUDED>(p, k, tri, t);
  }
}

template <bool OCCLUDED>
static void launchQueryT(const QueryParams& p, int grid, hipStream_t s, bool cull) {
  if (cull) hipLaunchKernelGGL((queryKernel<OCCLUDED, true>), dim3(grid), dim3(BLOCK), 0, s, p);
  else hipLaunchKernelGGL((queryKernel<OCCLUDED, false>), dim3(grid), dim3(BLOCK), 0, s, p);
}

hipError_t launchQuery(const QueryParams& p, int grid, hipStream_t s, bool occluded, bool cull) {
  if (occluded) launchQueryT<true>(p, grid, s, cull);
  else launchQueryT<false>(p, grid, s, cull);
  return hipGetLastError();
}

}  // namespace pt
