// pt_queries.cpp -- the ray queries of the C-ABI in include/pt_abi.h: closest hit and occlusion, with or
// without a bound per ray, on device memory in stream order or on host arrays. One kernel
// (pt_query.hip queryKernel) and one host path (queryHost) serve every entry point. And the radiance
// query (pt_radiance_device, pt_radiance: pt_radiance.hip radianceKernel), which shares the queries'
// overflow area and their one-at-a-time ordering, with its many-sample form folded on the GPU
// (pt_radiance_mean_device, pt_radiance_mean: pt_radiance_mean.hip) and the camera rays it is specified
// against (pt_camera_rays_device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_plan.h"
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

// What every launch of a query does before its kernel: the device, the overflow area (*ovfDepth entries per
// thread, 0: none), and its turn -- the area is one query's at a time, so behind the last one on another stream
static int beginQuery(pt_ctx* ctx, int* ovfDepth) {
  CK(hipSetDevice(ctx->cfg.device_id));
  if (int rc = ensureQuery(ctx, ovfDepth)) return rc;
  if (ctx->queryIssued && ctx->queryStream != ctx->stream) CK(hipStreamWaitEvent(ctx->stream, ctx->queryDone, 0));
  return PT_OK;
}
// ... and after it
static int endQuery(pt_ctx* ctx) {
  CK(hipEventRecord(ctx->queryDone, ctx->stream));
  ctx->queryStream = ctx->stream;
  ctx->queryIssued = true;
  return PT_OK;
}
// the scene as a query walks it: the runtime's own tree, results reference-exact (pt_trace.h refReachable);
// the kernels keep each ray from outside the tree's origin domain off it (QueryParams::originLimit)
static SceneView queryScene(const pt_ctx* ctx) {
  SceneView s = sceneView(ctx);
  s.fast = ctx->fastReady && !(ctx->cfg.flags & (PT_FLAG_REFERENCE_TREE | PT_FLAG_COUNT_FETCHES)) ? 1 : 0;
  return s;
}
static bool queryCull(const pt_ctx* ctx) { return !(ctx->cfg.flags & (PT_FLAG_NO_CULL | PT_FLAG_COUNT_FETCHES)); }
static int queryGrid(const pt_ctx* ctx, int n) {
  return (int)std::min<long>(((long)n + BLOCK - 1) / BLOCK, (long)queryGridCap(ctx));
}

// One query of n > 0 rays in device memory, enqueued on the context's stream
static int queryOne(pt_ctx* ctx, const void* d_rays, const void* d_tmax, int n, void* d_t, void* d_tri, void* d_occ) {
  int ovfDepth = 0;
  if (int rc = beginQuery(ctx, &ovfDepth)) return rc;
  QueryParams p;
  p.scene = queryScene(ctx);
  p.rays = static_cast<const float*>(d_rays);
  p.tmax = static_cast<const float*>(d_tmax);
  p.n = n;
  p.t = static_cast<float*>(d_t);
  p.tri = static_cast<int*>(d_tri);
  p.occ = static_cast<uint8_t*>(d_occ);
  p.ovf = ovfDepth ? ctx->d_queryOvf : nullptr;
  p.ovfDepth = ovfDepth;
  p.originLimit = ctx->originLimit;
  CK(launchQuery(p, queryGrid(ctx, n), ctx->stream, d_occ != nullptr, queryCull(ctx)));
  return endQuery(ctx);
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

// the host forms' staging of at least `floats` floats; the stream is synchronised when a host form returns,
// so a staging that grows is not in use
static int ensureStage(pt_ctx* ctx, size_t floats) {
  if (floats > ctx->queryStageFloats) {
    dfree(ctx->d_queryStage);
    ctx->queryStageFloats = 0;
    CK(hipMalloc(&ctx->d_queryStage, floats * sizeof(float)));
    ctx->queryStageFloats = floats;
  }
  return PT_OK;
}

// The host forms: the rays (and bounds) staged in, the device query, the results staged out, all on the
// context's stream, which is synchronised on return -- the staging is never in flight between calls.
// Staging per ray: 6 floats of ray, the bound, t, the triangle (the occlusion bytes take t's place).
static int queryHost(pt_ctx* ctx, const float* rays, const float* tmax, int n, float* t_out, int* tri_out,
                     uint8_t* occ_out) {
  CK(hipSetDevice(ctx->cfg.device_id));
  if (int rc = ensureStage(ctx, (size_t)n * 9)) return rc;
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

// ------------------------------------------------------------ radiance along caller-supplied rays
// One sample of the context's integrator along n > 0 rays in device memory, enqueued on the context's stream
static int radianceOne(pt_ctx* ctx, const void* d_rays, const void* d_ids, int n, uint32_t sampleIndex, void* d_out) {
  int ovfDepth = 0;
  if (int rc = beginQuery(ctx, &ovfDepth)) return rc;
  RadianceParams p;
  p.scene = queryScene(ctx);
  p.env = envView(ctx, rowTable(ctx, false), largeScene(ctx) ? 1 : 0);  // as a megakernel frame reads it
  p.rays = static_cast<const float*>(d_rays);
  p.ids = static_cast<const int*>(d_ids);
  p.n = n;
  p.sampleIndex = sampleIndex;
  p.maxBounce = maxBounce(ctx->cfg);
  p.out = static_cast<float4*>(d_out);
  p.ovf = ovfDepth ? ctx->d_queryOvf : nullptr;
  p.ovfDepth = ovfDepth;
  p.originLimit = ctx->originLimit;
  CK(launchRadiance(p, ctx->cfg.integrator, queryGrid(ctx, n), ctx->stream, queryCull(ctx)));
  return endQuery(ctx);
}

int pt_radiance_device(pt_ctx* ctx, const void* d_rays, const void* d_ids, int n, uint32_t sampleIndex, void* d_out) {
  bool run;
  if (int rc = queryArgs(ctx, n, d_rays && d_out, &run)) return rc;
  return run ? radianceOne(ctx, d_rays, d_ids, n, sampleIndex, d_out) : PT_OK;
}

// The host form, staged like queryHost: per ray 6 floats of ray, 2 ints of id and 4 floats of result
int pt_radiance(pt_ctx* ctx, const float* rays, const int* ids, int n, uint32_t sampleIndex, float* out) {
  bool run;
  if (int rc = queryArgs(ctx, n, rays && out, &run)) return rc;
  if (!run) return PT_OK;
  CK(hipSetDevice(ctx->cfg.device_id));
  if (int rc = ensureStage(ctx, (size_t)n * 12)) return rc;
  float* dRays = ctx->d_queryStage;
  int* dIds = reinterpret_cast<int*>(dRays + (size_t)n * 6);
  float* dOut = dRays + (size_t)n * 8;
  CK(hipMemcpyAsync(dRays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (ids) CK(hipMemcpyAsync(dIds, ids, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = radianceOne(ctx, dRays, ids ? dIds : nullptr, n, sampleIndex, dOut)) return rc;
  CK(hipMemcpyAsync(out, dOut, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

// nSamples samples (firstSample ...) along n > 0 rays in device memory, folded into d_mean (and d_moments,
// nullable) by pt_radiance_mean.hip; otherwise as radianceOne
static int radianceMeanOne(pt_ctx* ctx, const void* d_rays, const void* d_ids, int n, uint32_t firstSample,
                           int nSamples, uint32_t flags, void* d_mean, void* d_moments) {
  int ovfDepth = 0;
  if (int rc = beginQuery(ctx, &ovfDepth)) return rc;
  RadianceMeanParams p;
  p.scene = queryScene(ctx);
  p.env = envView(ctx, rowTable(ctx, false), largeScene(ctx) ? 1 : 0);  // as radianceOne
  p.rays = static_cast<const float*>(d_rays);
  p.ids = static_cast<const int*>(d_ids);
  p.n = n;
  p.firstSample = firstSample;
  p.nSamples = nSamples;
  p.perSample = (flags & PT_RADIANCE_RAYS_PER_SAMPLE) ? 1 : 0;
  p.maxBounce = maxBounce(ctx->cfg);
  p.mean = static_cast<float4*>(d_mean);
  p.moments = static_cast<float2*>(d_moments);
  p.ovf = ovfDepth ? ctx->d_queryOvf : nullptr;
  p.ovfDepth = ovfDepth;
  p.originLimit = ctx->originLimit;
  CK(launchRadianceMean(p, ctx->cfg.integrator, queryGrid(ctx, n), ctx->stream, queryCull(ctx)));
  return endQuery(ctx);
}

// the checks of the two forms: the sample range and the flags first, then queryArgs
static int radianceMeanArgs(pt_ctx* ctx, int n, uint32_t firstSample, int nSamples, uint32_t flags, bool pointers,
                            bool* run) {
  *run = false;
  if (nSamples < 1 || (uint64_t)firstSample + (uint64_t)nSamples > 0xFFFFFFFFull) return PT_E_INVALID;  // s + 1u must not wrap
  if (flags & ~(uint32_t)PT_RADIANCE_RAYS_PER_SAMPLE) return PT_E_INVALID;
  return queryArgs(ctx, n, pointers, run);
}

int pt_radiance_mean_device(pt_ctx* ctx, const void* d_rays, const void* d_ids, int n, uint32_t firstSample,
                            int nSamples, uint32_t flags, void* d_mean, void* d_moments) {
  bool run;
  if (int rc = radianceMeanArgs(ctx, n, firstSample, nSamples, flags, d_rays && d_mean, &run)) return rc;
  return run ? radianceMeanOne(ctx, d_rays, d_ids, n, firstSample, nSamples, flags, d_mean, d_moments) : PT_OK;
}

// The host form, staged like pt_radiance: per ray 4 floats of mean and 2 of moments (in when the picture
// goes on, and out), 2 ints of id, and 6 floats per ray the caller gave (n, or nSamples x n)
int pt_radiance_mean(pt_ctx* ctx, const float* rays, const int* ids, int n, uint32_t firstSample, int nSamples,
                     uint32_t flags, float* mean, float* moments) {
  bool run;
  if (int rc = radianceMeanArgs(ctx, n, firstSample, nSamples, flags, rays && mean, &run)) return rc;
  if (!run) return PT_OK;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t nRays = (flags & PT_RADIANCE_RAYS_PER_SAMPLE) ? (size_t)nSamples * (size_t)n : (size_t)n;
  if (int rc = ensureStage(ctx, (size_t)n * 8 + nRays * 6)) return rc;
  float* dMean = ctx->d_queryStage;  // first: 16-byte aligned
  float* dMoments = dMean + (size_t)n * 4;
  int* dIds = reinterpret_cast<int*>(dMoments + (size_t)n * 2);
  float* dRays = dMoments + (size_t)n * 4;
  CK(hipMemcpyAsync(dRays, rays, nRays * 6 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (ids) CK(hipMemcpyAsync(dIds, ids, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (firstSample != 0u) {
    CK(hipMemcpyAsync(dMean, mean, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (moments) CK(hipMemcpyAsync(dMoments, moments, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  if (int rc = radianceMeanOne(ctx, dRays, ids ? dIds : nullptr, n, firstSample, nSamples, flags, dMean,
                               moments ? dMoments : nullptr))
    return rc;
  CK(hipMemcpyAsync(mean, dMean, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (moments) CK(hipMemcpyAsync(moments, dMoments, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

int pt_camera_rays_device(pt_ctx* ctx, const float eye[3], const float cameraRotate[16], uint32_t sampleIndex,
                          void* d_rays, void* d_ids) {
  if (!ctx || !eye || !cameraRotate || !d_rays) return PT_E_INVALID;
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT) return fail(ctx, PT_E_INVALID, "not a GL integrator's context");
  CK(hipSetDevice(ctx->cfg.device_id));
  CameraRaysParams p;
  p.width = ctx->cfg.width;
  p.height = ctx->cfg.height;
  p.sampleIndex = sampleIndex;
  std::memcpy(p.eye, eye, sizeof(p.eye));
  std::memcpy(p.cam, cameraRotate, sizeof(p.cam));
  p.rays = static_cast<float*>(d_rays);
  p.ids = static_cast<int*>(d_ids);
  CK(launchCameraRays(p, ctx->stream));
  return PT_OK;
}
