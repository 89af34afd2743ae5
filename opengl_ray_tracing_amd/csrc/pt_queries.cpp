// pt_queries.cpp -- the ray queries of the C-ABI in include/pt_abi.h: closest hit and occlusion, with or
// without a bound per ray, on device memory in stream order or on host arrays. One kernel
// (pt_query.hip queryKernel) and one host path (queryHost) serve every entry point.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_runtime.h"

using namespace pt;

// The largest grid a query launches: its stack overflow area is sized for it once, whatever n is
static int queryGridCap(const pt_ctx* ctx) { return ctx->numCU * 8; }

// A query's own resources before its first launch, and again after a scene upload deepened the trees:
// the completion event and the stack overflow area. In the steady state this
// allocates nothing and waits for nothing.
static int ensureQuery(pt_ctx* ctx, int* ovfDepth) {
  if (!ctx->queryDone) CK(hipEventCreateWithFlags(&ctx->queryDone, hipEventDisableTiming));
  *ovfDepth = ctx->maxStack > LDS_STACK ? ctx->maxStack - LDS_STACK / 2 : 0;  // pt_trace.h StackT
  const size_t need = (size_t)queryGridCap(ctx) * BLOCK * (size_t)*ovfDepth;
  if (need > ctx->queryOvfInts) {
    if (ctx->queryIssued) CK(hipEventSynchronize(ctx->queryDone));  // an earlier query may still use the old area
    dfree(ctx->d_queryOvf);
    ctx->queryOvfInts = 0;
    CK(hipMalloc(&ctx->d_queryOvf, need * sizeof(int)));
    ctx->queryOvfInts = need;
  }
  return PT_OK;
}

// One query of n > 0 rays in device memory, enqueued on the context's stream
static int queryOne(pt_ctx* ctx, const void* d_rays, const void* d_tmax, int n, void* d_t, void* d_tri, void* d_occ) {
  CK(hipSetDevice(ctx->cfg.device_id));
  int ovfDepth = 0;
  if (int rc = ensureQuery(ctx, &ovfDepth)) return rc;
  // the overflow area is one query's at a time: behind the last one on another stream
  if (ctx->queryIssued && ctx->queryStream != ctx->stream) CK(hipStreamWaitEvent(ctx->stream, ctx->queryDone, 0));
  QueryParams p;
  p.scene = sceneView(ctx);
  // the runtime's own tree, results reference-exact (pt_trace.h refReachable)
  p.scene.fast = ctx->fastReady && !(ctx->cfg.flags & (PT_FLAG_REFERENCE_TREE | PT_FLAG_COUNT_FETCHES)) ? 1 : 0;
  p.rays = static_cast<const float*>(d_rays);
  p.tmax = static_cast<const float*>(d_tmax);
  p.n = n;
  p.t = static_cast<float*>(d_t);
  p.tri = static_cast<int*>(d_tri);
  p.occ = static_cast<uint8_t*>(d_occ);
  p.ovf = ovfDepth ? ctx->d_queryOvf : nullptr;
  p.ovfDepth = ovfDepth;
  const bool cull = !(ctx->cfg.flags & (PT_FLAG_NO_CULL | PT_FLAG_COUNT_FETCHES));
  const int grid = (int)std::min<long>(((long)n + BLOCK - 1) / BLOCK, (long)queryGridCap(ctx));
  CK(launchQuery(p, grid, ctx->stream, d_occ != nullptr, cull));
  CK(hipEventRecord(ctx->queryDone, ctx->stream));
  ctx->queryStream = ctx->stream;
  ctx->queryIssued = true;
  return PT_OK;
}

// the argument checks the entry points share: PT_OK with *run = false when there is nothing to do
static int queryArgs(pt_ctx* ctx, int n, bool pointers, bool* run) {
  *run = false;
  if (!ctx || n < 0 || (n > 0 && !pointers)) return PT_E_INVALID;
  if (!ctx->d_bvh) return fail(ctx, PT_E_NOSCENE, "no scene");
  *run = n > 0;
  return PT_OK;
}

int pt_trace_closest_device(pt_ctx* ctx, const void* d_rays, const void* d_tmax, int n, void* d_t, void* d_tri) {
  bool run;
  if (int rc = queryArgs(ctx, n, d_rays && d_t && d_tri, &run)) return rc;
  return run ? queryOne(ctx, d_rays, d_tmax, n, d_t, d_tri, nullptr) : PT_OK;
}

int pt_trace_occluded_device(pt_ctx* ctx, const void* d_rays, const void* d_tmax, int n, void* d_occ) {
  bool run;
  if (int rc = queryArgs(ctx, n, d_rays && d_occ, &run)) return rc;
  return run ? queryOne(ctx, d_rays, d_tmax, n, nullptr, nullptr, d_occ) : PT_OK;
}

// The host forms: the rays (and bounds) staged in, the device query, the results staged out, all on the
// context's stream, which is synchronised on return -- the staging is never in flight between calls.
// Staging per ray: 6 floats of ray, the bound, t, the triangle (the occlusion bytes take t's place).
static int queryHost(pt_ctx* ctx, const float* rays, const float* tmax, int n, float* t_out, int* tri_out,
                     uint8_t* occ_out) {
  CK(hipSetDevice(ctx->cfg.device_id));
  if ((size_t)n > ctx->queryStageRays) {
    dfree(ctx->d_queryStage);
    ctx->queryStageRays = 0;
    CK(hipMalloc(&ctx->d_queryStage, (size_t)n * 9 * sizeof(float)));
    ctx->queryStageRays = (size_t)n;
  }
  float* dRays = ctx->d_queryStage;
  float* dTmax = dRays + (size_t)n * 6;
  float* dT = dTmax + n;
  int* dTri = reinterpret_cast<int*>(dT + n);
  CK(hipMemcpyAsync(dRays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (tmax) CK(hipMemcpyAsync(dTmax, tmax, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = queryOne(ctx, dRays, tmax ? dTmax : nullptr, n, occ_out ? nullptr : dT, occ_out ? nullptr : dTri,
                        occ_out ? dT : nullptr))
    return rc;
  if (occ_out) {
    CK(hipMemcpyAsync(occ_out, dT, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    CK(hipMemcpyAsync(t_out, dT, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(tri_out, dTri, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  }
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

// The unbounded closest hit of host rays, as BVH/main.cpp:571 asks it. Unlike the ranged forms it runs
// after every frame issued before it (it always has: callers rely on the drain).
int pt_trace_closest(pt_ctx* ctx, const float* rays, int n, float* t_out, int* tri_out) {
  bool run;
  if (int rc = queryArgs(ctx, n, rays && t_out && tri_out, &run)) return rc;
  if (!run) return PT_OK;
  if (int rc = syncStreams(ctx)) return rc;
  return queryHost(ctx, rays, nullptr, n, t_out, tri_out, nullptr);
}

int pt_trace_closest_range(pt_ctx* ctx, const float* rays, const float* tmax, int n, float* t_out, int* tri_out) {
  bool run;
  if (int rc = queryArgs(ctx, n, rays && t_out && tri_out, &run)) return rc;
  return run ? queryHost(ctx, rays, tmax, n, t_out, tri_out, nullptr) : PT_OK;
}

int pt_trace_occluded(pt_ctx* ctx, const float* rays, const float* tmax, int n, uint8_t* occ_out) {
  bool run;
  if (int rc = queryArgs(ctx, n, rays && occ_out, &run)) return rc;
  return run ? queryHost(ctx, rays, tmax, n, nullptr, nullptr, occ_out) : PT_OK;
}
