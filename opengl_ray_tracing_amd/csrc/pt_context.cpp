// pt_context.cpp -- the context of the C-ABI in include/pt_abi.h: device selection, creation and
// release, the caller's stream, synchronisation, the frame statistics, and the small device probes
// (pt_fmath_*, pt_sph_texel_device). The other subjects have files of their own: see pt_runtime.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_fmath.h"
#include "pt_kernels.h"
#include "pt_plan.h"
#include "pt_runtime.h"

using namespace pt;

static std::string g_create_err;

int pt_device_count(int* n) {
  if (!n) return PT_E_INVALID;
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  *n = c;
  return PT_OK;
}

const char* pt_last_error(pt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

static int createOne(pt_ctx** out, const pt_config* cfg) {
  if (!out || !cfg) return PT_E_INVALID;
  *out = nullptr;
  // width, height < 65536: the megakernel packs a pixel as (px | py << 16)
  if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 65535 || cfg->height > 65535 || cfg->integrator < 0 ||
      cfg->integrator > PT_BASIC_CPU_COMPAT ||
      cfg->tile_world < 1 || cfg->tile_rank < 0 || cfg->tile_rank >= cfg->tile_world || cfg->sample_world < 0 ||
      cfg->sample_rank < 0 || cfg->sample_rank >= (cfg->sample_world > 0 ? cfg->sample_world : 1)) {
    g_create_err = "pt_create: invalid config";
    return PT_E_INVALID;
  }
  if (cfg->flags & PT_FLAG_WAVEFRONT) {  // retired in round 5; git history keeps it
    g_create_err = "pt_create: invalid config: PT_FLAG_WAVEFRONT (the staged wavefront pipeline) was retired";
    return PT_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_err = "pt_create: no HIP device";
    return PT_E_NODEVICE;
  }
  if (cfg->device_id < 0 || cfg->device_id >= ndev) {
    g_create_err = "pt_create: device_id out of range";
    return PT_E_INVALID;
  }
  pt_ctx* ctx = new (std::nothrow) pt_ctx();
  if (!ctx) return PT_E_NOMEM;
  ctx->cfg = *cfg;
  if (ctx->cfg.basic_samples <= 0) ctx->cfg.basic_samples = 128;
  int ss = cfg->tile_size > 0 ? cfg->tile_size : 32;
  if (ss % 8 != 0) {
    delete ctx;
    g_create_err = "pt_create: tile_size must be a multiple of 8";
    return PT_E_INVALID;
  }
  ctx->shardSize = ss;
  auto bail = [&](int code) {
    g_create_err = ctx->err;
    pt_destroy(ctx);
    return code;
  };
#define CKC(expr)                                                     \
  do {                                                                \
    hipError_t e_ = (expr);                                           \
    if (e_ != hipSuccess) {                                           \
      ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);   \
      return bail(PT_E_HIP);                                          \
    }                                                                 \
  } while (0)
  CKC(hipSetDevice(cfg->device_id));
  hipDeviceProp_t prop;
  CKC(hipGetDeviceProperties(&prop, cfg->device_id));
  ctx->numCU = prop.multiProcessorCount;
  CKC(hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking));
  ctx->stream = ctx->own;
  const size_t npix = (size_t)cfg->width * cfg->height;
  CKC(hipMalloc(&ctx->d_accum, npix * sizeof(float4)));
  CKC(hipMemset(ctx->d_accum, 0, npix * sizeof(float4)));
  if (cfg->flags & PT_FLAG_MOMENTS) {
    CKC(hipMalloc(&ctx->d_mom, npix * sizeof(float2)));
    CKC(hipMemset(ctx->d_mom, 0, npix * sizeof(float2)));
  }
  if (cfg->flags & PT_FLAG_ADAPTIVE) {
    ctx->adaptTilesX = (cfg->width + 7) / 8;
    ctx->adaptTiles = ctx->adaptTilesX * ((cfg->height + 7) / 8);
    CKC(hipMalloc(&ctx->d_err2, (size_t)ctx->adaptTiles * sizeof(float)));
    CKC(hipMemset(ctx->d_err2, 0, (size_t)ctx->adaptTiles * sizeof(float)));
    CKC(hipMalloc(&ctx->d_retiredAt, (size_t)ctx->adaptTiles * sizeof(uint32_t)));
    CKC(hipMemset(ctx->d_retiredAt, 0, (size_t)ctx->adaptTiles * sizeof(uint32_t)));
    CKC(hipEventCreateWithFlags(&ctx->adaptDone, hipEventDisableTiming));
  }
  CKC(hipMalloc(&ctx->d_ctl, CTL_BYTES));
  CKC(hipMemset(ctx->d_ctl, 0, CTL_BYTES));
  const Share share = shareOf(ctx, cfg->tile_rank, cfg->tile_world);
  ctx->shardsX = share.shardsX;
  ctx->shardsY = shardsY(share);
  ctx->numItems = waveTiles(share);
  ctx->perQueue = (ctx->numItems + NUM_QUEUES - 1) / NUM_QUEUES;
  // the path-regeneration kernel with the 4-wide walk for every integrator on any scene
  // (PT_REGEN_WIDE = 1; 0: never; unset: Lambert frames and large Disney/MIS scenes)
  if (const char* e = std::getenv("PT_REGEN_WIDE")) ctx->regenWide = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("PT_SOLO")) ctx->solo = std::atoi(e) != 0;
  ctx->pipe = pipelines(*cfg);
  if (ctx->pipe) {
    // the hardware queues of the process (GPU_MAX_HW_QUEUES, HIP's default 4; the Python package asks
    // for 12 when it is unset and HIP not yet initialised, and passes what is in effect as
    // pt_config.hw_queues)
    int hwq = cfg->hw_queues;
    if (hwq <= 0) {
      const char* q = std::getenv("GPU_MAX_HW_QUEUES");
      hwq = q && std::atoi(q) > 0 ? std::atoi(q) : 4;
    }
    ctx->pipeDepth = pipeDepthFor(*cfg, ctx->regenWide, hwq);
    if (const char* e = std::getenv("PT_PIPE_DEPTH")) {
      ctx->pipeDepth = std::min(PIPE, std::max(1, std::atoi(e)));
      ctx->pipeDepthFixed = true;
    }
    ctx->pipeDepthBase = ctx->pipeDepth;
    ctx->batchCap = batchFor(ctx, false);
    // slot streams are created as a depth first uses them (ensureSlots). (Created here instead,
    // before the context's own stream and the caller's, they take hardware queues of their own even
    // at GPU_MAX_HW_QUEUES = 4 -- created later they share one -- but c2's shares measured slower
    // that way in the 20-frame window, N = 2 / 4 / 8: 0.1091 / 0.0638 / 0.0439 -> 0.1164 / 0.0701 /
    // 0.0478 ms: the next launch's camera-ray pass then competes with the running launch's tail.)
    for (int k = 0; k < COLS; k++) CKC(hipEventCreateWithFlags(&ctx->mixDone[k], hipEventDisableTiming));
    CKC(hipEventCreateWithFlags(&ctx->binsBuilt, hipEventDisableTiming));
  }
#undef CKC
  *out = ctx;
  return PT_OK;
}

int pt_create(pt_ctx** out, const pt_config* cfg) {
  if (!out || !cfg) return PT_E_INVALID;
  *out = nullptr;
  const int n = cfg->n_devices;
  if (n < 0 || n > PT_MAX_DEVICES || cfg->gather < PT_GATHER_AUTO || cfg->gather > PT_GATHER_RCCL) {
    g_create_err = "pt_create: n_devices must be 0..8 and gather a PT_GATHER_* value";
    return PT_E_INVALID;
  }
  if (cfg->flags & PT_FLAG_MOMENTS) {
    // the moments are collected from the pipelined frames' colour buffer, which these do not have,
    // and are this context's own: a screen-tile share keeps them only when it says how they are
    // gathered (PT_FLAG_SHARE_MOMENTS: pt_pack_owned_stats / pt_unpack_ranks_stats)
    const bool shared = (cfg->flags & PT_FLAG_SHARE_MOMENTS) != 0;
    const char* why = nullptr;
    if (cfg->integrator == PT_BASIC_CPU_COMPAT) why = "PT_BASIC_CPU_COMPAT";
    else if (cfg->flags & PT_FLAG_COUNT_FETCHES) why = "PT_FLAG_COUNT_FETCHES";
    else if (cfg->flags & PT_FLAG_SERIAL_FRAMES) why = "PT_FLAG_SERIAL_FRAMES";
    else if (cfg->tile_world > 1 && !shared) why = "tile_world > 1 (without PT_FLAG_SHARE_MOMENTS)";
    else if (n > 1) why = "n_devices > 1";
    // (each sample rank's moments are of its own samples: merging them is not the gather's bit-exact copy)
    else if (shared && cfg->sample_world > 1) why = "PT_FLAG_SHARE_MOMENTS and sample_world > 1";
    if (why) {
      g_create_err = std::string("pt_create: PT_FLAG_MOMENTS cannot be combined with ") + why;
      return PT_E_INVALID;
    }
  }
  if ((cfg->flags & PT_FLAG_SHARE_MOMENTS) && !(cfg->flags & PT_FLAG_MOMENTS)) {
    g_create_err = "pt_create: PT_FLAG_SHARE_MOMENTS needs PT_FLAG_MOMENTS";
    return PT_E_INVALID;
  }
  if (cfg->flags & PT_FLAG_ADAPTIVE) {
    // tiles retire from the moments, in the camera-ray pass, which needs the camera-ray bins
    const char* why = nullptr;
    if (!(cfg->flags & PT_FLAG_MOMENTS)) why = "needs PT_FLAG_MOMENTS";
    else if (cfg->flags & PT_FLAG_NO_BINS) why = "cannot be combined with PT_FLAG_NO_BINS";
    if (why) {
      g_create_err = std::string("pt_create: PT_FLAG_ADAPTIVE ") + why;
      return PT_E_INVALID;
    }
  }
  if (n <= 1) return createOne(out, cfg);
  if (cfg->tile_world > 1 || cfg->sample_world > 1 || cfg->integrator == PT_BASIC_CPU_COMPAT) {
    g_create_err = "pt_create: n_devices > 1 renders screen tiles of the GL integrators itself "
                   "(tile_world and sample_world must be <= 1)";
    return PT_E_INVALID;
  }
  // rank k: device_ids[k], screen tiles t % n == k
  pt_config c = *cfg;
  c.n_devices = 0;
  c.tile_world = n;
  c.tile_rank = 0;
  c.device_id = cfg->device_ids[0];
  int rc = createOne(out, &c);
  if (rc) return rc;
  pt_ctx* ctx = *out;
  ctx->cfg.n_devices = n;
  for (int k = 1; k < n; k++) {
    c.tile_rank = k;
    c.device_id = cfg->device_ids[k];
    pt_ctx* p = nullptr;
    if ((rc = createOne(&p, &c)) != PT_OK) {
      pt_destroy(ctx);
      *out = nullptr;
      return rc;
    }
    ctx->peers.push_back(p);
  }
  if ((rc = createGroup(ctx)) != PT_OK) {
    g_create_err = ctx->err;
    pt_destroy(ctx);
    *out = nullptr;
    return rc;
  }
  return PT_OK;
}

void pt_destroy(pt_ctx* ctx) {
  if (!ctx) return;
  destroyGroup(ctx);
  (void)hipSetDevice(ctx->cfg.device_id);
  if (ctx->own) (void)hipStreamSynchronize(ctx->own);
  dfree(ctx->d_geo); dfree(ctx->d_hit); dfree(ctx->d_mats); dfree(ctx->d_bvh); dfree(ctx->d_pairs);
  dfree(ctx->d_fbvh); dfree(ctx->d_fbvh4); dfree(ctx->d_fpairs); dfree(ctx->d_fastTri);
  dfree(ctx->d_refParent); dfree(ctx->d_refBox); dfree(ctx->d_leafBox);
  freeRefit(ctx);
  freeMaterialTables(ctx);
  releaseEnv(ctx);
  dfree(ctx->d_shapes); dfree(ctx->d_basicImg); dfree(ctx->d_stream); dfree(ctx->d_offsets); dfree(ctx->d_overruns);
  dfree(ctx->d_accum); dfree(ctx->d_ctl); dfree(ctx->d_ovf); dfree(ctx->d_cost); dfree(ctx->d_order);
  dfree(ctx->d_rgb);
  dfree(ctx->d_guide[2]);
  for (auto& set : ctx->d_guidePN) for (auto& g : set) dfree(g);
  dfree(ctx->d_res[0]); dfree(ctx->d_res[1]);
  dfree(ctx->d_mom); dfree(ctx->d_lum); dfree(ctx->d_var0); dfree(ctx->d_lv[0]); dfree(ctx->d_lv[1]);
  dfree(ctx->d_guideOvf); dfree(ctx->d_dn[0]); dfree(ctx->d_dn[1]); dfree(ctx->d_dnTm[0]); dfree(ctx->d_dnTm[1]);
  freePrimaryBins(ctx->bins);
  for (int k = 0; k < PIPE; k++) {
    if (ctx->slotStream[k]) (void)hipStreamSynchronize(ctx->slotStream[k]);
    dfree(ctx->d_prim[k]);
    dfree(ctx->d_live[k]);
    if (ctx->kernelDone[k]) (void)hipEventDestroy(ctx->kernelDone[k]);
    if (ctx->slotStream[k]) (void)hipStreamDestroy(ctx->slotStream[k]);
  }
  for (int k = 0; k < COLS; k++) {
    dfree(ctx->d_col[k]);
    if (ctx->mixDone[k]) (void)hipEventDestroy(ctx->mixDone[k]);
  }
  if (ctx->binsBuilt) (void)hipEventDestroy(ctx->binsBuilt);
  dfree(ctx->d_err2); dfree(ctx->d_retiredAt);
  if (ctx->adaptDone) (void)hipEventDestroy(ctx->adaptDone);
  if (ctx->queryDone) (void)hipEventSynchronize(ctx->queryDone);  // a query on a caller's stream
  dfree(ctx->d_queryOvf); dfree(ctx->d_queryStage);
  if (ctx->queryDone) (void)hipEventDestroy(ctx->queryDone);
  for (hipEvent_t e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->own) (void)hipStreamDestroy(ctx->own);
  delete ctx;
}

int pt_set_stream(pt_ctx* ctx, void* s) {
  if (!ctx) return PT_E_INVALID;
  ctx->stream = s ? reinterpret_cast<hipStream_t>(s) : ctx->own;
  return PT_OK;
}

int pt_synchronize(pt_ctx* ctx) {
  if (!ctx) return PT_E_INVALID;
  return ctx->peers.empty() ? syncStreams(ctx) : syncGroup(ctx);
}

static int statsOne(pt_ctx* ctx, pt_frame_stats* st) {
  if (int rc = syncStreams(ctx)) return rc;
  unsigned long long h[5];
  std::vector<unsigned long long> shards((size_t)RAY_SHARDS * RAY_SHARD_STRIDE);
  CK(hipMemcpy(h, ctx->d_ctl + CTL_STATS, sizeof(h), hipMemcpyDeviceToHost));
  CK(hipMemcpy(shards.data(), ctx->d_ctl + CTL_RAYS, shards.size() * sizeof(unsigned long long),
               hipMemcpyDeviceToHost));
  std::memset(st, 0, sizeof(*st));
  st->rays = h[0];
  for (int k = 0; k < RAY_SHARDS; k++) st->rays += shards[(size_t)k * RAY_SHARD_STRIDE];
  st->node_fetch = h[1];
  st->tri_fetch = h[2];
  st->mat_fetch = h[3];
  st->tex_fetch = h[4];
  foldLaunches(ctx);
  st->kernel_ms = ctx->launches > 0 ? ctx->msLast : 0.0f;
  st->kernel_ms_total = (float)ctx->msTotal;
  st->launches = ctx->launches;
  st->frames = ctx->frames;
  st->frame_batch = ctx->batchCap;
  st->env_compact = compactLevel(ctx->env);
  st->tree4_nodes = ctx->fast4Ready ? ctx->f4nDev : 0;
  st->max_stack = ctx->maxStack;
  st->split_items = 0;
  st->runtime_tree = ctx->lastFast ? 1 : 0;
  st->waves_per_simd = ctx->lastWaves;
  st->regen = ctx->lastRegen ? 1 : 0;
  st->devices = 1;
  st->gather = 0;
  st->frames_in_flight = ctx->pipe ? ctx->pipeDepth : 1;
  st->upload_ms = ctx->uploadMs;
  st->accel_build_ms = ctx->accelMs;
  st->accel_device = ctx->accelDevice;
  st->accel_nodes = ctx->accelNodes;
  st->accel_depth = ctx->accelDepth;
  const int ls = ctx->pipe && ctx->frameNo > 0 ? ctx->lastSlot : 0;  // the last frame's slot
  if (ctx->d_order && ctx->orderValid[ls]) {
    int counts[NUM_QUEUES];
    const int* ord = ctx->d_order + (size_t)ls * ((size_t)NUM_QUEUES * ctx->orderCap + NUM_QUEUES);
    CK(hipMemcpy(counts, ord + (size_t)NUM_QUEUES * ctx->orderCap, sizeof(counts), hipMemcpyDeviceToHost));
    long items = 0;
    for (int q = 0; q < NUM_QUEUES; q++) items += counts[q];
    st->split_items = (int)std::max(0L, items - (long)ctx->numItems);
  }
  return PT_OK;
}

// A group: rays and fetches summed over the devices, kernel times the slowest device's,
// launches / policies rank 0's.
int pt_get_stats(pt_ctx* ctx, pt_frame_stats* st) {
  if (!ctx || !st) return PT_E_INVALID;
  if (ctx->peers.empty()) return statsOne(ctx, st);
  if (int rc = syncGroup(ctx)) return rc;
  if (int rc = statsOne(ctx, st)) return rc;
  for (pt_ctx* p : ctx->peers) {
    pt_frame_stats q;
    if (int rc = statsOne(p, &q)) return fromPeer(ctx, p, rc);
    st->rays += q.rays;
    st->node_fetch += q.node_fetch;
    st->tri_fetch += q.tri_fetch;
    st->mat_fetch += q.mat_fetch;
    st->tex_fetch += q.tex_fetch;
    st->kernel_ms = std::max(st->kernel_ms, q.kernel_ms);
    st->kernel_ms_total = std::max(st->kernel_ms_total, q.kernel_ms_total);
    st->max_stack = std::max(st->max_stack, q.max_stack);
    st->split_items += q.split_items;
  }
  st->devices = 1 + (int)ctx->peers.size();
  st->gather = ctx->gather ? ctx->gather->mode : 0;
  return PT_OK;
}

static int resetOne(pt_ctx* ctx) {
  if (int rc = syncStreams(ctx)) return rc;
  CK(hipMemset(ctx->d_ctl + CTL_STATS, 0, CTL_BYTES - CTL_STATS));
  foldLaunches(ctx);
  ctx->launches = 0;
  ctx->frames = 0;
  ctx->msTotal = 0.0;
  ctx->msLast = 0.0f;
  return PT_OK;
}

int pt_reset_stats(pt_ctx* ctx) {
  if (!ctx) return PT_E_INVALID;
  for (pt_ctx* p : ctx->peers)
    if (int rc = resetOne(p)) return fromPeer(ctx, p, rc);
  return resetOne(ctx);
}

static float fmathHost(int fn, float x, float y) {
  switch (fn) {
    case 0: return ptm_sinf(x);
    case 1: return ptm_cosf(x);
    case 2: return ptm_atan2f(x, y);
    case 3: return ptm_asinf(x);
    case 4: return ptm_logf(x);
    case 5: return ptm_expf(x);
    case 6: return ptm_powf(x, y);
    case 7: return ptm_atan2f_fast(x, y);
    case 8: return ptm_asinf_fast(x);
    default: {  // 9, 10: the sine and the cosine of ptm_sincosf
      float s, c;
      ptm_sincosf(x, &s, &c);
      return fn == 9 ? s : c;
    }
  }
}

int pt_fmath_host(int fn, const float* x, const float* y, int n, float* out) {
  if (fn < 0 || fn > 10 || n < 0 || (n > 0 && (!x || !out))) return PT_E_INVALID;
  for (int i = 0; i < n; i++) out[i] = fmathHost(fn, x[i], y ? y[i] : 0.0f);
  return PT_OK;
}

int pt_fmath_device(pt_ctx* ctx, int fn, const float* x, const float* y, int n, float* out) {
  if (!ctx || fn < 0 || fn > 10 || n < 0 || (n > 0 && (!x || !out))) return PT_E_INVALID;
  if (n == 0) return PT_OK;
  CK(hipSetDevice(ctx->cfg.device_id));
  float *dx = nullptr, *dy = nullptr, *dout = nullptr;
  const size_t b = (size_t)n * sizeof(float);
  CK(hipMalloc(&dx, b));
  CK(hipMalloc(&dy, b));
  CK(hipMalloc(&dout, b));
  CK(hipMemcpy(dx, x, b, hipMemcpyHostToDevice));
  if (y) CK(hipMemcpy(dy, y, b, hipMemcpyHostToDevice));
  else CK(hipMemset(dy, 0, b));
  CK(launchFmath(fn, dx, dy, n, dout, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  CK(hipMemcpy(out, dout, b, hipMemcpyDeviceToHost));
  CK(hipFree(dx));
  CK(hipFree(dy));
  CK(hipFree(dout));
  return PT_OK;
}

int pt_sph_texel_device(pt_ctx* ctx, int W, int H, const float* dirs, int n, int* texel, int* texel_exact) {
  if (!ctx || W < 1 || H < 1 || (int64_t)W * H > INT32_MAX || n < 0 || (n > 0 && (!dirs || !texel || !texel_exact)))
    return PT_E_INVALID;
  if (n == 0) return PT_OK;
  CK(hipSetDevice(ctx->cfg.device_id));
  float* dd = nullptr;
  int* dt = nullptr;  // texel, then texel_exact
  const size_t bt = (size_t)n * sizeof(int);
  CK(hipMalloc(&dd, (size_t)n * 3 * sizeof(float)));
  CK(hipMalloc(&dt, 2 * bt));
  CK(hipMemcpy(dd, dirs, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  CK(launchSphTexel(W, H, dd, n, dt, dt + n, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  CK(hipMemcpy(texel, dt, bt, hipMemcpyDeviceToHost));
  CK(hipMemcpy(texel_exact, dt + n, bt, hipMemcpyDeviceToHost));
  CK(hipFree(dd));
  CK(hipFree(dt));
  return PT_OK;
}

int pt_abi_version(void) { return PT_ABI_VERSION; }
