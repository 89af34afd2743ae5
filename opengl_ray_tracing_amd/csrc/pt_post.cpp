// pt_post.cpp -- the display post-processing of the C-ABI in include/pt_abi.h: the guide buffers,
// the two a-trous denoisers, the sample moments' accessors and the temporal resolve. None of it is
// on the frame path: it reads the accumulation the frames leave (pt_runtime.cpp) and shares with
// it only what pt_runtime.h declares.
#include <algorithm>
#include <cstring>

#include "pt_plan.h"
#include "pt_runtime.h"

// an H x W plane of T the context allocates when it is first needed
template <class T>
static int ensure(pt_ctx* ctx, T*& plane) {
  if (!plane) CK(hipMalloc(&plane, (size_t)ctx->cfg.width * ctx->cfg.height * sizeof(T)));
  return PT_OK;
}

// an H x W plane of elem-byte pixels to the caller's memory, host or device; returns when it is there
static int copyPlane(pt_ctx* ctx, void* dst, const void* plane, size_t elem) {
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(hipMemcpyAsync(dst, plane, (size_t)ctx->cfg.width * ctx->cfg.height * elem, hipMemcpyDefault, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

// a whole-frame image (every pixel: one rank of one) tone-mapped to the caller's RGBA8 image
static int displayImage(pt_ctx* ctx, const float4* img, float limit, float gamma, void* dimage) {
  CK(hipSetDevice(ctx->cfg.device_id));
  PackParams p = packParams(ctx, 0, 1);
  CK(launchDisplayOwn(p, img, limit, gamma, reinterpret_cast<uchar4*>(dimage), ctx->stream));
  return PT_OK;
}

// a context that can hold guides: a GL integrator with a scene
static int guideContext(pt_ctx* ctx, const char* what) {
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT)
    return fail(ctx, PT_E_INVALID, std::string(what) + ": not for PT_BASIC_CPU_COMPAT contexts");
  if (!ctx->d_bvh) return fail(ctx, PT_E_NOSCENE, std::string(what) + ": no scene");
  return PT_OK;
}
static int guidesReady(pt_ctx* ctx, const char* what) {
  if (int rc = guideContext(ctx, what)) return rc;
  if (!ctx->guidesValid || ctx->guideVersion != ctx->sceneVersion)
    return fail(ctx, PT_E_INVALID, std::string(what) + ": no guides of this scene (pt_render_guides first)");
  return PT_OK;
}

// the parameters pt_denoise_params and pt_denoise_var_params share
template <class Prm>
static int checkFilter(pt_ctx* ctx, const std::string& what, const Prm& P) {
  if (P.passes < 1 || P.passes > 8) return fail(ctx, PT_E_INVALID, what + ": passes must be 1..8");
  if (P.normal_log2 < -1 || P.normal_log2 > 10) return fail(ctx, PT_E_INVALID, what + ": normal_log2 must be -1..10");
  if (!(P.limit > 0.0f)) return fail(ctx, PT_E_INVALID, what + ": limit must be > 0");
  return PT_OK;
}

// A filter call after its parameter checks: the input (the caller's, else the accumulation as the
// frames rendered so far leave it), then first(in, npix) for what the filter launches before its
// passes, then the passes, ping-pong through the context's two planes, the last one into the
// caller's buffer if there is one. `a` is the filter's kernel parameters: the AtrousCommon fields
// are filled here, pass(i, last) sets the filter's own and launches pass i.
template <class Prm, class Params, class First, class Pass>
static int runFilter(pt_ctx* ctx, const std::string& what, const Prm& P, Params& a, const void* d_in_rgba,
                     void* d_out_rgba, First first, Pass pass) {
  // an input that is one of the two planes, or the output, would be overwritten while it is read
  if (d_in_rgba && (d_in_rgba == d_out_rgba || d_in_rgba == ctx->d_dn[0] || d_in_rgba == ctx->d_dn[1]))
    return fail(ctx, PT_E_INVALID, what + ": the input must not be the output or the context's denoised buffer");
  if (int rc = joinGather(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  for (auto& plane : ctx->d_dn)
    if (int rc = ensure(ctx, plane)) return rc;
  const float4* in = d_in_rgba ? reinterpret_cast<const float4*>(d_in_rgba) : ctx->d_accum;
  if (int rc = first(in, (size_t)ctx->cfg.width * ctx->cfg.height)) return rc;
  a.width = ctx->cfg.width;
  a.height = ctx->cfg.height;
  a.posT = ctx->d_guide[0];
  a.nrmTri = ctx->d_guide[1];
  a.albedo = ctx->d_guide[2];
  a.sigmaZ = P.sigma_z;
  a.albDen = P.sigma_a * P.sigma_a;
  a.albOn = P.sigma_a > 0.0f;
  a.normalLog2 = P.normal_log2;
  a.limit = P.limit;
  for (int i = 0; i < P.passes; i++) {
    const bool last = i == P.passes - 1;
    a.stride = 1 << i;
    a.in = in;
    a.out = last && d_out_rgba ? reinterpret_cast<float4*>(d_out_rgba) : ctx->d_dn[i & 1];
    if (int rc = pass(i, last)) return rc;
    in = a.out;
  }
  ctx->denoised = in;
  return PT_OK;
}

extern "C" {

// ------------------------------------------------------------ guide buffers and the denoised display
static_assert(sizeof(pt_denoise_params) == PT_DENOISE_PARAMS_SIZE, "pt_denoise_params layout");

void pt_denoise_defaults(pt_denoise_params* prm) {
  if (!prm) return;
  prm->passes = 5;
  prm->sigma_c = 2.0f;
  prm->sigma_z = 0.02f;
  prm->sigma_a = 0.2f;
  prm->normal_log2 = 6;
  prm->limit = 1.5f;
}

int pt_denoise_params_size(void) { return (int)sizeof(pt_denoise_params); }

int pt_render_guides(pt_ctx* ctx, const float eye[3], const float cameraRotate[16]) {
  if (!ctx || !eye || !cameraRotate) return PT_E_INVALID;
  if (int rc = guideContext(ctx, "pt_render_guides")) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const int W = ctx->cfg.width, H = ctx->cfg.height;
  // the set that is not the history's
  const int set = ctx->histValid ? 1 - ctx->histSet : ctx->guideSet;
  for (auto& g : ctx->d_guidePN[set])
    if (int rc = ensure(ctx, g)) return rc;
  if (int rc = ensure(ctx, ctx->d_guide[2])) return rc;
  ctx->guideSet = set;
  ctx->d_guide[0] = ctx->d_guidePN[set][0];
  ctx->d_guide[1] = ctx->d_guidePN[set][1];
  ctx->resolvedFresh = false;  // a resolve of the previous guides is not committed with these
  const long tiles = (long)((W + 7) / 8) * ((H + 7) / 8);
  const int grid = (int)std::min<long>((tiles + BLOCK / 64 - 1) / (BLOCK / 64), (long)ctx->numCU * 8);
  // the kernel's own overflow area: frames in flight keep using d_ovf meanwhile
  const int ovfDepth = ctx->maxStack > LDS_STACK ? ctx->maxStack - LDS_STACK / 2 : 0;
  const size_t need = (size_t)grid * BLOCK * (size_t)ovfDepth;
  if (need > ctx->guideOvfInts) {
    CK(hipStreamSynchronize(ctx->stream));  // an earlier guide launch may still use the old area
    dfree(ctx->d_guideOvf);
    ctx->guideOvfInts = 0;
    CK(hipMalloc(&ctx->d_guideOvf, need * sizeof(int)));
    ctx->guideOvfInts = need;
  }
  GuideParams p;
  p.scene = sceneView(ctx);
  // the hit search of pt_trace_closest: the runtime's own tree, results reference-exact -- for an eye in
  // its origin domain (pt_plan.h eyeInDomain), else the uploaded tree alone
  p.scene.fast = ctx->fastReady && eyeInDomain(ctx, eye) &&
                         !(ctx->cfg.flags & (PT_FLAG_REFERENCE_TREE | PT_FLAG_COUNT_FETCHES))
                     ? 1
                     : 0;
  p.width = W;
  p.height = H;
  std::memcpy(p.eye, eye, sizeof(p.eye));
  std::memcpy(p.cam, cameraRotate, sizeof(p.cam));
  p.posT = ctx->d_guide[0];
  p.nrmTri = ctx->d_guide[1];
  p.albedo = ctx->d_guide[2];
  p.ovf = ovfDepth ? ctx->d_guideOvf : nullptr;
  p.ovfDepth = ovfDepth;
  const bool cull = !(ctx->cfg.flags & (PT_FLAG_NO_CULL | PT_FLAG_COUNT_FETCHES));
  CK(launchGuides(p, grid, ctx->stream, cull));
  ctx->guidesValid = true;
  ctx->guideVersion = ctx->sceneVersion;
  std::memcpy(ctx->guideEye, eye, sizeof(ctx->guideEye));
  std::memcpy(ctx->guideCam, cameraRotate, sizeof(ctx->guideCam));
  return PT_OK;
}

int pt_download_guides(pt_ctx* ctx, float* pos_t, float* nrm_tri, float* albedo) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = guidesReady(ctx, "pt_download_guides")) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t bytes = (size_t)ctx->cfg.width * ctx->cfg.height * sizeof(float4);
  float* dst[3] = {pos_t, nrm_tri, albedo};
  for (int k = 0; k < 3; k++)  // up to three planes, then one wait: not copyPlane
    if (dst[k]) CK(hipMemcpyAsync(dst[k], ctx->d_guide[k], bytes, hipMemcpyDefault, ctx->stream));  // host or device
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

int pt_guides_device_ptr(pt_ctx* ctx, void** pos_t, void** nrm_tri, void** albedo) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = guidesReady(ctx, "pt_guides_device_ptr")) return rc;
  if (pos_t) *pos_t = ctx->d_guide[0];
  if (nrm_tri) *nrm_tri = ctx->d_guide[1];
  if (albedo) *albedo = ctx->d_guide[2];
  return PT_OK;
}

int pt_denoise(pt_ctx* ctx, const pt_denoise_params* prm, void* d_out_rgba) {
  return pt_denoise_from(ctx, prm, nullptr, d_out_rgba);
}

int pt_denoise_from(pt_ctx* ctx, const pt_denoise_params* prm, const void* d_in_rgba, void* d_out_rgba) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = guidesReady(ctx, "pt_denoise")) return rc;
  pt_denoise_params P;
  pt_denoise_defaults(&P);
  if (prm) P = *prm;
  if (int rc = checkFilter(ctx, "pt_denoise", P)) return rc;
  AtrousParams a;
  return runFilter(
      ctx, "pt_denoise_from", P, a, d_in_rgba, d_out_rgba,
      [&](const float4* in, size_t npix) {
        for (auto& plane : ctx->d_dnTm)
          if (int rc = ensure(ctx, plane)) return rc;
        CK(launchAtrousTm(in, ctx->d_dnTm[0], (int)npix, P.limit, ctx->stream));
        return PT_OK;
      },
      [&](int i, bool last) {
        const float sc = P.sigma_c * (1.0f / (float)(1 << i));  // halved every pass
        a.colDen = sc * sc;
        a.colOn = sc > 0.0f;
        a.tmIn = ctx->d_dnTm[i & 1];
        a.tmOut = last ? nullptr : ctx->d_dnTm[(i + 1) & 1];
        CK(launchAtrous(a, ctx->stream));
        return PT_OK;
      });
}

int pt_denoised_device_ptr(pt_ctx* ctx, void** dptr) {
  if (!ctx || !dptr) return PT_E_INVALID;
  if (!ctx->denoised) return fail(ctx, PT_E_INVALID, "pt_denoised_device_ptr: no pt_denoise yet");
  *dptr = const_cast<float4*>(ctx->denoised);
  return PT_OK;
}

int pt_download_denoised(pt_ctx* ctx, float* rgba) {
  if (!ctx || !rgba) return PT_E_INVALID;
  if (!ctx->denoised) return fail(ctx, PT_E_INVALID, "pt_download_denoised: no pt_denoise yet");
  return copyPlane(ctx, rgba, ctx->denoised, sizeof(float4));
}

int pt_display_denoised(pt_ctx* ctx, float limit, float gamma, void* dimage) {
  if (!ctx || !dimage || !(limit > 0.0f)) return PT_E_INVALID;
  if (!ctx->denoised) return fail(ctx, PT_E_INVALID, "pt_display_denoised: no pt_denoise yet");
  return displayImage(ctx, ctx->denoised, limit, gamma, dimage);
}

// ------------------------------------------------------------ sample moments and the variance-guided filter
static_assert(sizeof(pt_denoise_var_params) == PT_DENOISE_VAR_PARAMS_SIZE, "pt_denoise_var_params layout");

int pt_moments_frames(pt_ctx* ctx, uint32_t* frames) {
  if (!ctx || !frames) return PT_E_INVALID;
  *frames = ctx->d_mom ? ctx->momFrames : 0u;
  return PT_OK;
}

int pt_download_moments(pt_ctx* ctx, float* m) {
  if (!ctx || !m) return PT_E_INVALID;
  if (!ctx->d_mom) return fail(ctx, PT_E_INVALID, "pt_download_moments: not a PT_FLAG_MOMENTS context");
  if (int rc = joinPipe(ctx)) return rc;
  return copyPlane(ctx, m, ctx->d_mom, sizeof(float2));
}

int pt_moments_device_ptr(pt_ctx* ctx, void** dptr) {
  if (!ctx || !dptr) return PT_E_INVALID;
  if (!ctx->d_mom) return fail(ctx, PT_E_INVALID, "pt_moments_device_ptr: not a PT_FLAG_MOMENTS context");
  *dptr = ctx->d_mom;
  return PT_OK;
}

void pt_denoise_var_defaults(pt_denoise_var_params* prm) {
  if (!prm) return;
  prm->passes = 5;
  prm->sigma_l = 4.0f;
  prm->sigma_z = 0.02f;
  prm->sigma_a = 0.2f;
  prm->normal_log2 = 6;
  prm->limit = 1.5f;
  prm->min_temporal = 8;
}

int pt_denoise_var_params_size(void) { return (int)sizeof(pt_denoise_var_params); }

int pt_denoise_var(pt_ctx* ctx, const pt_denoise_var_params* prm, const void* d_in_rgba, void* d_out_rgba) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = guidesReady(ctx, "pt_denoise_var")) return rc;
  pt_denoise_var_params P;
  pt_denoise_var_defaults(&P);
  if (prm) P = *prm;
  if (int rc = checkFilter(ctx, "pt_denoise_var", P)) return rc;
  if (P.min_temporal < 2) return fail(ctx, PT_E_INVALID, "pt_denoise_var: min_temporal must be >= 2");
  AtrousVarParams a;
  a.sigmaL = P.sigma_l;
  return runFilter(
      ctx, "pt_denoise_var", P, a, d_in_rgba, d_out_rgba,
      [&](const float4* in, size_t npix) {
        for (auto& plane : ctx->d_lv)
          if (int rc = ensure(ctx, plane)) return rc;
        if (int rc = ensure(ctx, ctx->d_lum)) return rc;
        if (int rc = ensure(ctx, ctx->d_var0)) return rc;
        CK(launchVarLum(in, ctx->d_lum, (int)npix, P.limit, ctx->stream));
        // step A: from the moments once they hold min_temporal frames, else (or without them) spatial
        const float kf = ctx->d_mom ? (float)ctx->momFrames : 0.0f;
        VarInitParams v;
        v.width = ctx->cfg.width;
        v.height = ctx->cfg.height;
        v.in = in;
        v.nrmTri = ctx->d_guide[1];
        v.moments = ctx->d_mom && kf >= (float)P.min_temporal ? ctx->d_mom : nullptr;
        v.lum = ctx->d_lum;
        v.var0 = ctx->d_var0;
        v.lv = ctx->d_lv[0];
        v.kf = kf;
        v.limit = P.limit;
        CK(launchVarInit(v, ctx->stream));
        ctx->varianceValid = true;
        return PT_OK;
      },
      [&](int i, bool last) {
        a.lvIn = ctx->d_lv[i & 1];
        a.lvOut = last ? nullptr : ctx->d_lv[(i + 1) & 1];
        CK(launchAtrousVar(a, ctx->stream));
        return PT_OK;
      });
}

int pt_download_variance(pt_ctx* ctx, float* v) {
  if (!ctx || !v) return PT_E_INVALID;
  if (!ctx->varianceValid) return fail(ctx, PT_E_INVALID, "pt_download_variance: no pt_denoise_var yet");
  return copyPlane(ctx, v, ctx->d_var0, sizeof(float));
}

// ------------------------------------------------------------ the temporal resolve
static_assert(sizeof(pt_temporal_params) == PT_TEMPORAL_PARAMS_SIZE, "pt_temporal_params layout");

void pt_temporal_defaults(pt_temporal_params* prm) {
  if (!prm) return;
  prm->sigma_z = 0.02f;
  prm->normal_cos = 0.9f;
  prm->max_history = 32.0f;
}

int pt_temporal_params_size(void) { return (int)sizeof(pt_temporal_params); }

int pt_temporal_resolve(pt_ctx* ctx, const pt_temporal_params* prm, uint32_t frames, void* d_out_rgba) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = guidesReady(ctx, "pt_temporal_resolve")) return rc;
  pt_temporal_params P;
  pt_temporal_defaults(&P);
  if (prm) P = *prm;
  if (frames == 0) return fail(ctx, PT_E_INVALID, "pt_temporal_resolve: frames must be >= 1 (frameCounter + 1)");
  if (!(P.sigma_z >= 0.0f)) return fail(ctx, PT_E_INVALID, "pt_temporal_resolve: sigma_z must be >= 0");
  if (!(P.normal_cos >= -1.0f && P.normal_cos <= 1.0f))
    return fail(ctx, PT_E_INVALID, "pt_temporal_resolve: normal_cos must be in [-1, 1]");
  if (!(P.max_history >= 1.0f)) return fail(ctx, PT_E_INVALID, "pt_temporal_resolve: max_history must be >= 1");
  // the accumulation as the frames rendered so far leave it
  if (int rc = joinGather(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  float4* out = reinterpret_cast<float4*>(d_out_rgba);
  if (!out) {
    // never the history's plane: a second resolve recomputes from the same history
    const int k = ctx->histValid ? 1 - ctx->histRes : ctx->resCur;
    if (int rc = ensure(ctx, ctx->d_res[k])) return rc;
    ctx->resCur = k;
    out = ctx->d_res[k];
  }
  TemporalParams t;
  t.width = ctx->cfg.width;
  t.height = ctx->cfg.height;
  t.accum = ctx->d_accum;
  t.posT = ctx->d_guide[0];
  t.nrmTri = ctx->d_guide[1];
  t.hist = t.histPosT = t.histNrmTri = nullptr;
  if (ctx->histValid) {
    t.hist = ctx->d_res[ctx->histRes];
    t.histPosT = ctx->d_guidePN[ctx->histSet][0];
    t.histNrmTri = ctx->d_guidePN[ctx->histSet][1];
  }
  t.out = out;
  for (int k = 0; k < 3; k++) {
    t.eye[k] = ctx->histEye[k];
    t.c0[k] = ctx->histCam[k];
    t.c1[k] = ctx->histCam[4 + k];
    t.c2[k] = ctx->histCam[8 + k];
  }
  t.sigmaZ = P.sigma_z;
  t.normalCos = P.normal_cos;
  t.maxHistory = P.max_history;
  t.frames = (float)frames;
  CK(launchTemporal(t, ctx->stream));
  ctx->resolved = out;
  ctx->resolvedFresh = true;
  return PT_OK;
}

int pt_temporal_commit(pt_ctx* ctx) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = guidesReady(ctx, "pt_temporal_commit")) return rc;
  if (!ctx->resolvedFresh)
    return fail(ctx, PT_E_INVALID, "pt_temporal_commit: no pt_temporal_resolve since the last commit, reset or pt_render_guides");
  if (ctx->resolved != ctx->d_res[ctx->resCur])
    return fail(ctx, PT_E_INVALID, "pt_temporal_commit: the last resolve went to a caller's buffer (resolve with NULL to commit)");
  ctx->histRes = ctx->resCur;
  ctx->histSet = ctx->guideSet;
  std::memcpy(ctx->histEye, ctx->guideEye, sizeof(ctx->histEye));
  std::memcpy(ctx->histCam, ctx->guideCam, sizeof(ctx->histCam));
  ctx->histValid = true;
  ctx->resolvedFresh = false;
  return PT_OK;
}

int pt_temporal_reset(pt_ctx* ctx) {
  if (!ctx) return PT_E_INVALID;
  dropHistory(ctx);
  return PT_OK;
}

int pt_resolved_device_ptr(pt_ctx* ctx, void** dptr) {
  if (!ctx || !dptr) return PT_E_INVALID;
  if (!ctx->resolved) return fail(ctx, PT_E_INVALID, "pt_resolved_device_ptr: no pt_temporal_resolve yet");
  *dptr = const_cast<float4*>(ctx->resolved);
  return PT_OK;
}

int pt_download_resolved(pt_ctx* ctx, float* rgba) {
  if (!ctx || !rgba) return PT_E_INVALID;
  if (!ctx->resolved) return fail(ctx, PT_E_INVALID, "pt_download_resolved: no pt_temporal_resolve yet");
  return copyPlane(ctx, rgba, ctx->resolved, sizeof(float4));
}

int pt_display_resolved(pt_ctx* ctx, float limit, float gamma, void* dimage) {
  if (!ctx || !dimage || !(limit > 0.0f)) return PT_E_INVALID;
  if (!ctx->resolved) return fail(ctx, PT_E_INVALID, "pt_display_resolved: no pt_temporal_resolve yet");
  return displayImage(ctx, ctx->resolved, limit, gamma, dimage);
}

}  // extern "C"
