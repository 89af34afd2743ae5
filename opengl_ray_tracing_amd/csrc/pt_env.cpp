// pt_env.cpp -- the environment map of the C-ABI in include/pt_abi.h (pt_upload_env and the forms it
// keeps on the device, pt_hdr_cache_device, pt_update_env and pt_download_env), and the state of the
// BASIC integrator: its shapes, its replayed random stream and its double image.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_runtime.h"
#include "pt_scene.h"

using namespace pt;

// calculateHdrCache of host image hdr (w*h*3) into the device table out (w*h float4)
static int deviceHdrCache(pt_ctx* ctx, const float* hdr, int w, int h, float4* out) {
  const size_t n = (size_t)w * h;
  float* d3 = nullptr;
  float* scratch = nullptr;
  CK(hipMalloc(&d3, n * 3 * sizeof(float)));
  if (hipMalloc(&scratch, (2 * n + 2 * (size_t)w + 1) * sizeof(float)) != hipSuccess) {
    (void)hipFree(d3);
    return fail(ctx, PT_E_NOMEM, "hdr cache scratch");
  }
  hipError_t e = hipMemcpyAsync(d3, hdr, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = launchHdrCache(d3, w, h, out, scratch, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d3);
  (void)hipFree(scratch);
  if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("hdr cache: ") + hipGetErrorString(e));
  return PT_OK;
}

static int envOne(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = syncStreams(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  releaseEnvStore(ctx);  // an env pt_update_env made: its buffers go, and the pointers below are null
  dfree(ctx->d_hdr);
  dfree(ctx->d_cache);
  dfree(ctx->d_hdr8);
  dfree(ctx->d_cache4);
  dfree(ctx->d_cacheRow);
  dfree(ctx->d_cacheY);
  dfree(ctx->d_trig);
  dfree(ctx->d_light);
  ctx->hdrW = ctx->hdrH = 0;
  if (!hdr) return PT_OK;
  if (w <= 0 || h <= 0) return PT_E_INVALID;
  const size_t n = (size_t)w * h;
  // render layout (pt_kernels.h Env): (r, g, b, pdf) texels + (x, y) sample table
  std::vector<float4> a(n);
  for (size_t k = 0; k < n; k++)
    a[k] = make_float4(hdr[3 * k], hdr[3 * k + 1], hdr[3 * k + 2], cache ? cache[3 * k + 2] : 0.0f);
  CK(hipMalloc(&ctx->d_hdr, n * sizeof(float4)));
  CK(hipMalloc(&ctx->d_cache, n * sizeof(float2)));
  CK(hipMemcpy(ctx->d_hdr, a.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  if (cache) {
    std::vector<float2> b(n);
    for (size_t k = 0; k < n; k++) b[k] = make_float2(cache[3 * k], cache[3 * k + 1]);
    CK(hipMemcpy(ctx->d_cache, b.data(), n * sizeof(float2), hipMemcpyHostToDevice));
  } else {
    float4* full = nullptr;  // calculateHdrCache on the GPU, then packed into the render layout
    CK(hipMalloc(&full, n * sizeof(float4)));
    int rc = deviceHdrCache(ctx, hdr, w, h, full);
    if (!rc) {
      hipError_t e = launchEnvPack(ctx->d_hdr, full, ctx->d_cache, (int)n, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) rc = fail(ctx, PT_E_HIP, std::string("env pack: ") + hipGetErrorString(e));
    }
    (void)hipFree(full);
    if (rc) return rc;
  }
  // The compact texels (8 + 4 bytes instead of 16 + 8 per texel; pt_kernels.h Env), kept when every
  // texel decodes back to its float bits: a Radiance map's RGBE values and calculateHdrCache's
  // table always do. c4's MIS light samples read the sample table at uniformly random (xi1, xi2):
  // half the bytes per texel, twice the texels per cached line. PT_ENV_COMPACT=0: the float texels.
  static const bool compact = [] {
    const char* e = std::getenv("PT_ENV_COMPACT");
    return !e || std::atoi(e) != 0;
  }();
  // (built into locals and handed to the context only once verified: a failure part-way leaves the
  // float texels serving, never a half-built compact form)
  if (compact && w <= 65535 && h <= 65535) {
    uint2* hdr8 = nullptr;
    uint32_t* cache4 = nullptr;
    int* d_bad = nullptr;
    hipError_t e = hipMalloc(&hdr8, n * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&cache4, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d_bad, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream);
    if (e == hipSuccess) e = launchEnvCompact(ctx->d_hdr, ctx->d_cache, w, h, hdr8, cache4, d_bad, ctx->stream);
    int bad = 1;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dfree(d_bad);
    if (e != hipSuccess || bad) {  // not exact (or failed): the float texels serve
      dfree(hdr8);
      dfree(cache4);
      if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("env compact: ") + hipGetErrorString(e));
    } else {
      ctx->d_hdr8 = hdr8;
      ctx->d_cache4 = cache4;
    }
  }
  if (ctx->d_cache4) {  // SampleHdr's sines and cosines of the compact table's integers (Env::trig)
    float2* trig = nullptr;
    hipError_t e2 = hipMalloc(&trig, (size_t)(w + h + 2) * sizeof(float2));
    if (e2 == hipSuccess) e2 = launchEnvTrig(trig, w, h, ctx->stream);
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(ctx->stream);
    if (e2 != hipSuccess) {
      dfree(trig);
      return fail(ctx, PT_E_HIP, std::string("env trig: ") + hipGetErrorString(e2));
    }
    ctx->d_trig = trig;
    // ... and every entry's light-sample color and pdf (Env::light)
    Env e;
    std::memset(&e, 0, sizeof(e));
    e.hdr = ctx->d_hdr;
    e.hdr8 = ctx->d_hdr8;
    e.trig = ctx->d_trig;
    e.w = e.res = w;
    e.h = h;
    uint2* light = nullptr;
    e2 = hipMalloc(&light, (size_t)(w + 1) * (h + 1) * sizeof(uint2));
    if (e2 == hipSuccess) e2 = launchEnvLight(e, light, ctx->stream);
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(ctx->stream);
    if (e2 != hipSuccess) {
      dfree(light);
      return fail(ctx, PT_E_HIP, std::string("env light: ") + hipGetErrorString(e2));
    }
    ctx->d_light = light;
  }
  if (ctx->d_cache4) {
    // the sample table by rows (pt_kernels.h Env::cacheRow), kept when every entry of every row equals
    // its row form: each row's x is one value, and the rows of one x hold the same y's
    std::vector<uint32_t> c4(n);
    CK(hipMemcpy(c4.data(), ctx->d_cache4, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint32_t> rows(h);
    std::vector<unsigned short> ys;
    std::vector<int> idOf(65536, -1);
    bool ok = true;
    for (int i = 0; i < h && ok; i++) {
      const uint32_t* row = c4.data() + (size_t)i * w;
      const uint32_t x = row[0] & 0xffffu;
      int id = idOf[x];
      if (id < 0) {
        id = idOf[x] = (int)(ys.size() / (size_t)w);
        for (int j = 0; j < w; j++) ys.push_back((unsigned short)(row[j] >> 16));
      }
      const unsigned short* yr = ys.data() + (size_t)id * w;
      for (int j = 0; j < w && ok; j++) ok = (row[j] & 0xffffu) == x && (row[j] >> 16) == yr[j];
      rows[i] = x | (uint32_t)id << 16;
    }
    if (ok) {  // both or neither (Env::cacheRow reads cacheY)
      uint32_t* cr = nullptr;
      unsigned short* cy = nullptr;
      hipError_t e = hipMalloc(&cr, rows.size() * sizeof(uint32_t));
      if (e == hipSuccess) e = hipMalloc(&cy, ys.size() * sizeof(unsigned short));
      if (e == hipSuccess) e = hipMemcpy(cr, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMemcpy(cy, ys.data(), ys.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        dfree(cr);
        dfree(cy);
        return fail(ctx, PT_E_HIP, std::string("env rows: ") + hipGetErrorString(e));
      }
      ctx->d_cacheRow = cr;
      ctx->d_cacheY = cy;
    }
  }
  ctx->policyKey++;
  ctx->hdrW = w;
  ctx->hdrH = h;
  return PT_OK;
}

int pt_hdr_cache_device(pt_ctx* ctx, const float* hdr, int w, int h, float* cache_out) {
  if (!ctx || !hdr || !cache_out || w <= 0 || h <= 0) return PT_E_INVALID;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t n = (size_t)w * h;
  float4* d = nullptr;
  CK(hipMalloc(&d, n * sizeof(float4)));
  int rc = deviceHdrCache(ctx, hdr, w, h, d);
  std::vector<float4> b(rc ? 0 : n);
  if (!rc && hipMemcpy(b.data(), d, n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(ctx, PT_E_HIP, "pt_hdr_cache_device: copy");
  (void)hipFree(d);
  if (rc) return rc;
  for (size_t k = 0; k < n; k++) {
    cache_out[3 * k] = b[k].x;
    cache_out[3 * k + 1] = b[k].y;
    cache_out[3 * k + 2] = b[k].z;
  }
  return PT_OK;
}

int pt_upload_env(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache) {
  if (!ctx) return PT_E_INVALID;
  dropHistory(ctx);
  if (int rc = dropMoments(ctx)) return rc;
  if (ctx->peers.empty()) return envOne(ctx, hdr, w, h, cache);
  // a device group computes calculateHdrCache once (on rank 0's GPU) and uploads it everywhere
  std::vector<float> own;
  if (hdr && !cache && w > 0 && h > 0) {
    own.resize((size_t)w * h * 3);
    if (int rc = pt_hdr_cache_device(ctx, hdr, w, h, own.data())) return rc;
    cache = own.data();
  }
  for (pt_ctx* m : members(ctx))
    if (int rc = envOne(m, hdr, w, h, cache)) return fromPeer(ctx, m, rc);
  return PT_OK;
}

// ------------------------------------------------------------ environment update (pt_envupdate.hip)
static void freeStore(EnvStore& s) {
  dfree(s.hdr); dfree(s.cache); dfree(s.hdr8); dfree(s.cache4); dfree(s.cacheRow); dfree(s.cacheY); dfree(s.rowTmp);
  dfree(s.trig); dfree(s.light); dfree(s.flags); dfree(s.full); dfree(s.scratch); dfree(s.quant); dfree(s.stageHdr);
  dfree(s.stageCache);
  s = EnvStore{};
}

void releaseEnvStore(pt_ctx* ctx) {
  if (!ctx->envStore.w) return;
  freeStore(ctx->envStore);
  ctx->d_hdr = nullptr;
  ctx->d_cache = nullptr;
  ctx->d_hdr8 = nullptr;
  ctx->d_cache4 = nullptr;
  ctx->d_cacheRow = nullptr;
  ctx->d_cacheY = nullptr;
  ctx->d_trig = nullptr;
  ctx->d_light = nullptr;
}

static int envCompactLevel(const pt_ctx* ctx) { return ctx->d_hdr8 ? (ctx->d_cacheRow ? 2 : 1) : 0; }  // pt_frame_stats.env_compact

template <class T>
static bool tryAlloc(T** p, size_t count) {  // an optional table: false, and no error left behind, when it does not fit
  if (hipMalloc(p, count * sizeof(T)) == hipSuccess) return true;
  *p = nullptr;
  (void)hipGetLastError();
  return false;
}

// The buffers of a w x h map, every form's: the compact forms are allocated whether or not the first map
// is compact, so that a later one of the same size allocates nothing. The float texels, the float table
// and the flag words are required; every other table falls back when it cannot be allocated (the compact
// forms to the float ones, trig and light to the kernels' own arithmetic, the rows to the compact table).
static int makeStore(pt_ctx* ctx, int w, int h, EnvStore& s) {
  const size_t n = (size_t)w * h;
  if (!tryAlloc(&s.hdr, n) || !tryAlloc(&s.cache, n) || !tryAlloc(&s.flags, (size_t)ENV_FLAGS)) {
    freeStore(s);
    return fail(ctx, PT_E_NOMEM, "pt_update_env: texels");
  }
  s.w = w;
  s.h = h;
  const char* c = std::getenv("PT_ENV_COMPACT");  // as pt_upload_env: 0 keeps the float texels
  if ((c && std::atoi(c) == 0) || w > 65535 || h > 65535) return PT_OK;
  if (!tryAlloc(&s.hdr8, n) || !tryAlloc(&s.cache4, n)) {
    dfree(s.hdr8);
    dfree(s.cache4);
    return PT_OK;
  }
  if (!tryAlloc(&s.cacheRow, (size_t)h) || !tryAlloc(&s.cacheY, n) || !tryAlloc(&s.rowTmp, (size_t)ENV_X_SLOTS + h)) {
    dfree(s.cacheRow);
    dfree(s.cacheY);
    dfree(s.rowTmp);
  }
  if (tryAlloc(&s.trig, (size_t)(w + h + 2))) tryAlloc(&s.light, (size_t)(w + 1) * (h + 1));
  return PT_OK;
}

// One context's update. The map is w*h*3 floats in host memory (hdr, cache: staged here) or in the
// context's device memory (d_hdr, d_cache), read in stream order on its stream; the caller has waited
// for the frames and queries in flight. A map of the current store's size is written into the store's
// buffers; any other size gets a new store, and the old environment -- the previous store, or
// pt_upload_env's allocations -- is released only once the new one is complete.
static int updateEnvOne(pt_ctx* ctx, const float* hdr, const float* cache, const float* d_hdr, const float* d_cache, int w,
                        int h, uint32_t flags) {
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t n = (size_t)w * h;
  const bool rgbe = (flags & PT_ENV_RGBE) != 0, hasTable = hdr ? cache != nullptr : d_cache != nullptr;
  const bool fresh = ctx->envStore.w != w || ctx->envStore.h != h;
  EnvStore made;
  if (fresh)
    if (int rc = makeStore(ctx, w, h, made)) return rc;
  EnvStore& st = fresh ? made : ctx->envStore;
  // what this kind of update needs beside the forms, made at its first use
  bool got = true;
  if (!hasTable) got = (st.full || tryAlloc(&st.full, n)) && (st.scratch || tryAlloc(&st.scratch, 2 * n + 2 * (size_t)w + 1));
  if (got && !hasTable && rgbe) got = st.quant || tryAlloc(&st.quant, 3 * n);
  if (got && hdr) got = st.stageHdr || tryAlloc(&st.stageHdr, 3 * n);
  if (got && hdr && cache) got = st.stageCache || tryAlloc(&st.stageCache, 3 * n);
  if (!got) {
    if (fresh) freeStore(made);
    return fail(ctx, PT_E_NOMEM, "pt_update_env: table scratch or staging");
  }
  // PT_UPDATE_TIMES (environment; tools/env_time.py): the device time of each step, on stderr
  const bool timed = std::getenv("PT_UPDATE_TIMES") != nullptr;
  constexpr int NEV = 6;
  struct StepEvents {  // destroyed on every way out
    hipEvent_t ev[NEV] = {};
    ~StepEvents() {
      for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    }
  } steps;
  hipError_t e = hipSuccess;
  if (timed)
    for (int k = 0; k < NEV && e == hipSuccess; k++) e = hipEventCreate(&steps.ev[k]);
  auto mark = [&](int k) {
    if (timed && e == hipSuccess) e = hipEventRecord(steps.ev[k], ctx->stream);
  };
  hipStream_t s = ctx->stream;
  if (e == hipSuccess && hdr) {
    e = hipMemcpyAsync(st.stageHdr, hdr, 3 * n * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && cache) e = hipMemcpyAsync(st.stageCache, cache, 3 * n * sizeof(float), hipMemcpyHostToDevice, s);
    d_hdr = st.stageHdr;
    d_cache = cache ? st.stageCache : nullptr;
  }
  if (e == hipSuccess) e = hipMemsetAsync(st.flags, 0, ENV_FLAGS * sizeof(int), s);
  mark(0);
  float* quant = rgbe && !hasTable ? st.quant : nullptr;
  if (e == hipSuccess) e = launchEnvTexels(d_hdr, d_cache, rgbe ? 1 : 0, st.hdr, st.cache, quant, (int)n, s);
  mark(1);
  if (e == hipSuccess && !hasTable) {  // calculateHdrCache of the texels as stored, packed into the render layout
    e = launchHdrCache(quant ? quant : d_hdr, w, h, st.full, st.scratch, s);
    if (e == hipSuccess) e = launchEnvPack(st.hdr, st.full, st.cache, (int)n, s);
  }
  mark(2);
  if (e == hipSuccess && st.hdr8) e = launchEnvCompact(st.hdr, st.cache, w, h, st.hdr8, st.cache4, st.flags + ENV_BAD, s);
  mark(3);
  // Env::trig once per (w, h); Env::light and the rows from whatever the compact forms hold -- whether they
  // serve is known only after the one read-back below, and any contents keep both kernels in bounds
  if (e == hipSuccess && st.hdr8 && st.trig && !st.trigReady) {
    e = launchEnvTrig(st.trig, w, h, s);
    st.trigReady = e == hipSuccess;
  }
  if (e == hipSuccess && st.hdr8 && st.trig && st.light) {
    Env v;
    std::memset(&v, 0, sizeof(v));
    v.hdr = st.hdr;
    v.hdr8 = st.hdr8;
    v.trig = st.trig;
    v.w = v.res = w;
    v.h = h;
    e = launchEnvLight(v, st.light, s);
  }
  mark(4);
  if (e == hipSuccess && st.hdr8 && st.cacheRow) e = launchEnvRows(st, s);
  mark(5);
  int f[ENV_FLAGS] = {1, 1, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(f, st.flags, sizeof(f), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the one host synchronisation
  if (e != hipSuccess) {
    if (fresh) freeStore(made);
    return fail(ctx, PT_E_HIP, std::string("pt_update_env: ") + hipGetErrorString(e));
  }
  // the hand-over: the Env the kernels get, chosen from the three ints
  const int wasW = ctx->hdrW, wasH = ctx->hdrH, wasCompact = envCompactLevel(ctx);
  if (fresh) {
    releaseEnvStore(ctx);
    dfree(ctx->d_hdr); dfree(ctx->d_cache); dfree(ctx->d_hdr8); dfree(ctx->d_cache4);
    dfree(ctx->d_cacheRow); dfree(ctx->d_cacheY); dfree(ctx->d_trig); dfree(ctx->d_light);
    ctx->envStore = made;
  }
  const EnvStore& k = ctx->envStore;
  const bool compact = k.hdr8 && !f[ENV_BAD], rows = compact && k.cacheRow && !f[ENV_ROWS_BAD];
  ctx->d_hdr = k.hdr;
  ctx->d_cache = k.cache;
  ctx->d_hdr8 = compact ? k.hdr8 : nullptr;
  ctx->d_cache4 = compact ? k.cache4 : nullptr;
  ctx->d_trig = compact ? k.trig : nullptr;
  ctx->d_light = compact && k.trig ? k.light : nullptr;
  ctx->d_cacheRow = rows ? k.cacheRow : nullptr;
  ctx->d_cacheY = rows ? k.cacheY : nullptr;
  ctx->hdrW = w;
  ctx->hdrH = h;
  // the measured launch policies were measured for a map of this size in this form: they stay while both do
  if (wasW != w || wasH != h || wasCompact != envCompactLevel(ctx)) ctx->policyKey++;
  if (timed) {
    float ms[NEV - 1] = {};
    for (int j = 0; j + 1 < NEV; j++) CK(hipEventElapsedTime(&ms[j], steps.ev[j], steps.ev[j + 1]));
    std::fprintf(stderr, "pt_update_env: texels %.4f table %.4f compact %.4f light %.4f rows %.4f ms, env_compact %d, %d rows\n",
                 ms[0], ms[1], ms[2], ms[3], ms[4], envCompactLevel(ctx), rows ? f[ENV_ROW_IDS] : 0);
  }
  return PT_OK;
}

static int envUpdateArgs(pt_ctx* ctx, const void* hdr, int w, int h, uint32_t flags) {
  if (!ctx) return PT_E_INVALID;
  if (flags & ~(uint32_t)PT_ENV_RGBE) return fail(ctx, PT_E_INVALID, "pt_update_env: unknown flag bits");
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT) return fail(ctx, PT_E_INVALID, "pt_update_env: not on a BASIC context");
  if (!hdr) return PT_OK;
  if (w <= 0 || h <= 0) return fail(ctx, PT_E_INVALID, "pt_update_env: w and h must be positive");
  // every element count of the pipeline as an int: 3 floats per texel, Env::light's (w + 1)(h + 1), the table scratch
  const long long n = (long long)w * h, most = 2147483647LL;
  if (3 * n > most || (long long)(w + 1LL) * (h + 1LL) > most || 2 * n + 2LL * w + 1 > most)
    return fail(ctx, PT_E_INVALID, "pt_update_env: map too large");
  return PT_OK;
}

static int envWait(pt_ctx* ctx) {
  if (int rc = syncStreams(ctx)) return rc;  // no frame in flight reads the buffers rewritten here
  if (ctx->queryIssued) CK(hipEventSynchronize(ctx->queryDone));  // nor a ray query, whichever stream it is on
  return PT_OK;
}

int pt_update_env(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache, uint32_t flags) {
  if (int rc = envUpdateArgs(ctx, hdr, w, h, flags)) return rc;
  if (!hdr) return pt_upload_env(ctx, nullptr, 0, 0, nullptr);
  for (pt_ctx* m : members(ctx)) {
    if (int rc = envWait(m)) return fromPeer(ctx, m, rc);
    dropHistory(m);
    if (int rc = dropMoments(m)) return fromPeer(ctx, m, rc);
    if (int rc = updateEnvOne(m, hdr, cache, nullptr, nullptr, w, h, flags)) return fromPeer(ctx, m, rc);
  }
  return PT_OK;
}

int pt_update_env_device(pt_ctx* ctx, const void* d_hdr, int w, int h, const void* d_cache, uint32_t flags) {
  if (int rc = envUpdateArgs(ctx, d_hdr, w, h, flags)) return rc;
  if (!ctx->peers.empty()) return fail(ctx, PT_E_INVALID, "pt_update_env_device: not on an n_devices > 1 context");
  if (!d_hdr) return pt_upload_env(ctx, nullptr, 0, 0, nullptr);
  if (int rc = envWait(ctx)) return rc;
  dropHistory(ctx);
  if (int rc = dropMoments(ctx)) return rc;
  return updateEnvOne(ctx, nullptr, nullptr, static_cast<const float*>(d_hdr), static_cast<const float*>(d_cache), w, h, flags);
}

int pt_env_size(pt_ctx* ctx, int* w, int* h) {
  if (!ctx || !w || !h) return PT_E_INVALID;
  *w = ctx->d_hdr ? ctx->hdrW : 0;
  *h = ctx->d_hdr ? ctx->hdrH : 0;
  return PT_OK;
}

int pt_download_env(pt_ctx* ctx, int form, float* texels, float* table) {
  if (!ctx || (!texels && !table)) return PT_E_INVALID;
  if (form < 0 || form > 2) return fail(ctx, PT_E_INVALID, "pt_download_env: form must be 0, 1 or 2");
  if (!ctx->d_hdr) return fail(ctx, PT_E_INVALID, "pt_download_env: no environment");
  if (form > envCompactLevel(ctx)) return fail(ctx, PT_E_INVALID, "pt_download_env: the environment is not kept in that form");
  if (form == 2 && texels) return fail(ctx, PT_E_INVALID, "pt_download_env: the row form holds no texels");
  if (int rc = syncStreams(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t n = (size_t)ctx->hdrW * ctx->hdrH;
  if (form == 0) {
    if (texels) CK(hipMemcpy(texels, ctx->d_hdr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (table) CK(hipMemcpy(table, ctx->d_cache, n * sizeof(float2), hipMemcpyDeviceToHost));
    return PT_OK;
  }
  float4* t4 = nullptr;
  float2* t2 = nullptr;
  hipError_t e = hipSuccess;
  if (texels) e = hipMalloc(&t4, n * sizeof(float4));
  if (e == hipSuccess && table) e = hipMalloc(&t2, n * sizeof(float2));
  if (e == hipSuccess) e = launchEnvDecode(envView(ctx, form == 2, 0), form, t4, t2, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && texels) e = hipMemcpy(texels, t4, n * sizeof(float4), hipMemcpyDeviceToHost);
  if (e == hipSuccess && table) e = hipMemcpy(table, t2, n * sizeof(float2), hipMemcpyDeviceToHost);
  dfree(t4);
  dfree(t2);
  if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("pt_download_env: ") + hipGetErrorString(e));
  return PT_OK;
}

// ------------------------------------------------------------ the BASIC integrator's state
int pt_upload_shapes(pt_ctx* ctx, const double* shapes, int n) {
  if (!ctx || (!shapes && n > 0) || n < 0) return PT_E_INVALID;
  if (!ctx->peers.empty()) return fail(ctx, PT_E_INVALID, "BASIC shapes: one device only");
  if (int rc = syncStreams(ctx)) return rc;
  dfree(ctx->d_shapes);
  ctx->nShapes = 0;
  if (n == 0) return PT_OK;
  CK(hipMalloc(&ctx->d_shapes, (size_t)n * PT_SHAPE_DOUBLES * sizeof(double)));
  CK(hipMemcpy(ctx->d_shapes, shapes, (size_t)n * PT_SHAPE_DOUBLES * sizeof(double), hipMemcpyHostToDevice));
  ctx->nShapes = n;
  return PT_OK;
}

int pt_set_basic_stream(pt_ctx* ctx, const double* stream, int64_t n, const int64_t* offsets, int64_t nOffsets) {
  if (!ctx) return PT_E_INVALID;
  if (ctx->cfg.integrator != PT_BASIC_CPU_COMPAT) return fail(ctx, PT_E_INVALID, "not a BASIC context");
  if (int rc = syncStreams(ctx)) return rc;
  dfree(ctx->d_stream);
  dfree(ctx->d_offsets);
  ctx->streamN = ctx->nOffsets = 0;
  if (!stream) return PT_OK;
  if (n < 1 || !offsets || nOffsets < 1) return fail(ctx, PT_E_INVALID, "pt_set_basic_stream: empty stream or offsets");
  for (int64_t k = 0; k < nOffsets; k++)
    if (offsets[k] < 0 || offsets[k] > n || (k > 0 && offsets[k] < offsets[k - 1]))
      return fail(ctx, PT_E_INVALID, "pt_set_basic_stream: offsets must be non-decreasing within [0, n]");
  CK(hipMalloc(&ctx->d_stream, (size_t)n * sizeof(double)));
  CK(hipMalloc(&ctx->d_offsets, (size_t)nOffsets * sizeof(long long)));
  CK(hipMemcpy(ctx->d_stream, stream, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemcpy(ctx->d_offsets, offsets, (size_t)nOffsets * sizeof(long long), hipMemcpyHostToDevice));
  ctx->streamN = n;
  ctx->nOffsets = nOffsets;
  return PT_OK;
}

int pt_basic_replay_overruns(pt_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return PT_E_INVALID;
  if (int rc = syncStreams(ctx)) return rc;
  unsigned long long v = 0;
  if (ctx->d_overruns) CK(hipMemcpy(&v, ctx->d_overruns, sizeof(v), hipMemcpyDeviceToHost));
  *count = (int64_t)v;
  return PT_OK;
}

// the BASIC double image (basicKernel adds each sample to it), allocated and zeroed on first use
int ensureBasicImage(pt_ctx* ctx) {
  if (ctx->d_basicImg) return PT_OK;
  const size_t n = (size_t)ctx->cfg.width * ctx->cfg.height * 3;
  CK(hipMalloc(&ctx->d_basicImg, n * sizeof(double)));
  CK(hipMemsetAsync(ctx->d_basicImg, 0, n * sizeof(double), ctx->stream));
  return PT_OK;
}

int pt_download_basic_image(pt_ctx* ctx, double* rgb) {
  if (!ctx || !rgb) return PT_E_INVALID;
  if (ctx->cfg.integrator != PT_BASIC_CPU_COMPAT) return fail(ctx, PT_E_INVALID, "not a BASIC context");
  if (int rc = syncStreams(ctx)) return rc;
  const size_t n = (size_t)ctx->cfg.width * ctx->cfg.height * 3;
  if (!ctx->d_basicImg) {
    std::memset(rgb, 0, n * sizeof(double));
    return PT_OK;
  }
  CK(hipMemcpy(rgb, ctx->d_basicImg, n * sizeof(double), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_upload_basic_image(pt_ctx* ctx, const double* rgb) {
  if (!ctx || !rgb) return PT_E_INVALID;
  if (ctx->cfg.integrator != PT_BASIC_CPU_COMPAT) return fail(ctx, PT_E_INVALID, "not a BASIC context");
  if (int rc = syncStreams(ctx)) return rc;
  if (int rc = ensureBasicImage(ctx)) return rc;
  const size_t npix = (size_t)ctx->cfg.width * ctx->cfg.height;
  CK(hipMemcpyAsync(ctx->d_basicImg, rgb, npix * 3 * sizeof(double), hipMemcpyDefault, ctx->stream));
  CK(launchBasicNarrow(ctx->d_basicImg, ctx->d_accum, (long)npix, ctx->stream));  // the f32 sums, as a frame leaves them
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}
