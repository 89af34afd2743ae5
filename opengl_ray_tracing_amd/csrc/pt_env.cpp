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
#include "pt_update.h"

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

// ------------------------------------------------------------ the environment's buffers (pt_envupdate.h EnvStore)
static void freeStore(EnvStore& s) {
  dfree(s.hdr); dfree(s.cache); dfree(s.hdr8); dfree(s.cache4); dfree(s.cacheRow); dfree(s.cacheY); dfree(s.rowTmp);
  dfree(s.trig); dfree(s.light); dfree(s.flags); dfree(s.full); dfree(s.scratch); dfree(s.quant); dfree(s.stageHdr);
  dfree(s.stageCache);
  s = EnvStore{};
}

// the one place the context's view changes: the forms, and their size where the launch policy reads it
static void setEnvForms(pt_ctx* ctx, const EnvForms& v) {
  ctx->env = v;
  ctx->hdrW = v.w;
  ctx->hdrH = v.h;
}

void releaseEnv(pt_ctx* ctx) {
  freeStore(ctx->envStore);
  setEnvForms(ctx, EnvForms{});
}

template <class T>
static bool tryAlloc(T** p, size_t count) {  // an optional table: false, and no error left behind, when it does not fit
  if (hipMalloc(p, count * sizeof(T)) == hipSuccess) return true;
  *p = nullptr;
  (void)hipGetLastError();
  return false;
}

// The compact texels (8 + 4 bytes instead of 16 + 8 per texel; pt_kernels.h Env) are kept when every
// texel decodes back to its float bits: a Radiance map's RGBE values and calculateHdrCache's table
// always do. c4's MIS light samples read the sample table at uniformly random (xi1, xi2): half the
// bytes per texel, twice the texels per cached line. PT_ENV_COMPACT=0 (environment): the float texels.
static bool compactWanted(int w, int h) {
  const char* e = std::getenv("PT_ENV_COMPACT");
  return (!e || std::atoi(e) != 0) && w <= 65535 && h <= 65535;
}

// what launchEnvLight reads of an Env: the texels in both forms, Env::trig and the size
static Env lightEnv(const EnvStore& s) {
  Env e{};
  e.hdr = s.hdr;
  e.hdr8 = s.hdr8;
  e.trig = s.trig;
  e.w = e.res = s.w;
  e.h = s.h;
  return e;
}

// ------------------------------------------------------------ pt_upload_env
// The forms that serve a map from host memory, built into s and into nothing else: the float texels and
// table, and -- each only where it is exact, and where its optional buffers fit -- the compact forms,
// trig and light, and the table by rows. The caller frees s on a failure.
static int buildUpload(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache, EnvStore& s) {
  const size_t n = (size_t)w * h;
  s.w = w;
  s.h = h;
  // render layout (pt_kernels.h Env): (r, g, b, pdf) texels + (x, y) sample table
  std::vector<float4> a(n);
  for (size_t k = 0; k < n; k++)
    a[k] = make_float4(hdr[3 * k], hdr[3 * k + 1], hdr[3 * k + 2], cache ? cache[3 * k + 2] : 0.0f);
  CK(hipMalloc(&s.hdr, n * sizeof(float4)));
  CK(hipMalloc(&s.cache, n * sizeof(float2)));
  CK(hipMemcpy(s.hdr, a.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  if (cache) {
    std::vector<float2> b(n);
    for (size_t k = 0; k < n; k++) b[k] = make_float2(cache[3 * k], cache[3 * k + 1]);
    CK(hipMemcpy(s.cache, b.data(), n * sizeof(float2), hipMemcpyHostToDevice));
  } else {
    float4* full = nullptr;  // calculateHdrCache on the GPU, then packed into the render layout
    CK(hipMalloc(&full, n * sizeof(float4)));
    int rc = deviceHdrCache(ctx, hdr, w, h, full);
    if (!rc) {
      hipError_t e = launchEnvPack(s.hdr, full, s.cache, (int)n, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) rc = fail(ctx, PT_E_HIP, std::string("env pack: ") + hipGetErrorString(e));
    }
    (void)hipFree(full);
    if (rc) return rc;
  }
  int* d_bad = nullptr;
  int bad = 1;
  if (compactWanted(w, h) && tryAlloc(&s.hdr8, n) && tryAlloc(&s.cache4, n) && tryAlloc(&d_bad, 1)) {
    hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream);
    if (e == hipSuccess) e = launchEnvCompact(s.hdr, s.cache, w, h, s.hdr8, s.cache4, d_bad, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dfree(d_bad);
    if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("env compact: ") + hipGetErrorString(e));
  }
  if (bad) {  // not exact, not wanted or no room: the float texels serve, and nothing below applies
    dfree(s.hdr8);
    dfree(s.cache4);
    return PT_OK;
  }
  // SampleHdr's sines and cosines of the compact table's integers (Env::trig) ...
  if (tryAlloc(&s.trig, (size_t)(w + h + 2))) {
    hipError_t e = launchEnvTrig(s.trig, w, h, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("env trig: ") + hipGetErrorString(e));
    s.trigReady = true;
    // ... and every entry's light-sample color and pdf (Env::light)
    if (tryAlloc(&s.light, (size_t)(w + 1) * (h + 1))) {
      e = launchEnvLight(lightEnv(s), s.light, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("env light: ") + hipGetErrorString(e));
    }
  }
  // the sample table by rows (pt_kernels.h Env::cacheRow), kept when every entry of every row equals
  // its row form: each row's x is one value, and the rows of one x hold the same y's
  std::vector<uint32_t> c4(n);
  CK(hipMemcpy(c4.data(), s.cache4, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
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
  if (ok && tryAlloc(&s.cacheRow, rows.size()) && tryAlloc(&s.cacheY, ys.size())) {
    hipError_t e = hipMemcpy(s.cacheRow, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s.cacheY, ys.data(), ys.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("env rows: ") + hipGetErrorString(e));
  }
  if (!s.cacheY) dfree(s.cacheRow);  // both or neither (Env::cacheRow reads cacheY)
  return PT_OK;
}

// The old environment is released first, so the peak is one environment's memory; the new one reaches the
// context only when it is complete, and any failure leaves the context with no environment.
static int envOne(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache) {
  if (int rc = waitForReaders(ctx)) return rc;  // of the buffers freed here
  CK(hipSetDevice(ctx->cfg.device_id));
  releaseEnv(ctx);
  if (!hdr) return PT_OK;
  if (w <= 0 || h <= 0) return PT_E_INVALID;
  EnvStore s;
  if (int rc = buildUpload(ctx, hdr, w, h, cache, s)) {
    freeStore(s);
    return rc;
  }
  ctx->envStore = s;
  setEnvForms(ctx, envForms(s, true, true));  // buildUpload kept the exact forms only
  ctx->policyKey++;
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
  s.complete = true;
  if (!compactWanted(w, h)) return PT_OK;
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
// buffers; any other size, and any map after a pt_upload_env (whose store is not complete), gets a new
// store, and the old environment is released only once the new one is complete.
static int updateEnvOne(pt_ctx* ctx, const float* hdr, const float* cache, const float* d_hdr, const float* d_cache, int w,
                        int h, uint32_t flags) {
  dropHistory(ctx);  // the history and the moments saw the old light, as after an upload
  if (int rc = dropMoments(ctx)) return rc;
  const size_t n = (size_t)w * h;
  const bool rgbe = (flags & PT_ENV_RGBE) != 0, hasTable = hdr ? cache != nullptr : d_cache != nullptr;
  const bool fresh = !ctx->envStore.complete || ctx->envStore.w != w || ctx->envStore.h != h;
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
  StepEvents<6> steps;
  hipStream_t s = ctx->stream;
  hipError_t e = steps.create("PT_UPDATE_TIMES");
  auto mark = [&](int k) {
    if (e == hipSuccess) e = steps.mark(k, s);
  };
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
  if (e == hipSuccess && st.hdr8 && st.trig && st.light) e = launchEnvLight(lightEnv(st), st.light, s);
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
  // the hand-over: the forms the kernels get, chosen from the three ints
  const EnvForms was = ctx->env;
  if (fresh) {
    freeStore(ctx->envStore);
    ctx->envStore = made;
  }
  setEnvForms(ctx, envForms(ctx->envStore, !f[ENV_BAD], !f[ENV_ROWS_BAD]));
  // the measured launch policies were measured for a map of this size in this form: they stay while both do
  if (was.w != w || was.h != h || compactLevel(was) != compactLevel(ctx->env)) ctx->policyKey++;
  if (steps.on) {
    float ms[5] = {};
    CK(steps.elapsed(ms));
    std::fprintf(stderr, "pt_update_env: texels %.4f table %.4f compact %.4f light %.4f rows %.4f ms, env_compact %d, %d rows\n",
                 ms[0], ms[1], ms[2], ms[3], ms[4], compactLevel(ctx->env), ctx->env.cacheRow ? f[ENV_ROW_IDS] : 0);
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

int pt_update_env(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache, uint32_t flags) {
  if (int rc = envUpdateArgs(ctx, hdr, w, h, flags)) return rc;
  if (!hdr) return pt_upload_env(ctx, nullptr, 0, 0, nullptr);
  return updateMembers(ctx, nullptr, [&](pt_ctx* m) { return updateEnvOne(m, hdr, cache, nullptr, nullptr, w, h, flags); });
}

int pt_update_env_device(pt_ctx* ctx, const void* d_hdr, int w, int h, const void* d_cache, uint32_t flags) {
  if (int rc = envUpdateArgs(ctx, d_hdr, w, h, flags)) return rc;
  if (!d_hdr && ctx->peers.empty()) return pt_upload_env(ctx, nullptr, 0, 0, nullptr);
  return updateAlone(ctx, "pt_update_env_device", nullptr, [&](pt_ctx* m) {
    return updateEnvOne(m, nullptr, nullptr, static_cast<const float*>(d_hdr), static_cast<const float*>(d_cache), w, h, flags);
  });
}

int pt_env_size(pt_ctx* ctx, int* w, int* h) {
  if (!ctx || !w || !h) return PT_E_INVALID;
  *w = ctx->env.w;
  *h = ctx->env.h;
  return PT_OK;
}

int pt_download_env(pt_ctx* ctx, int form, float* texels, float* table) {
  if (!ctx || (!texels && !table)) return PT_E_INVALID;
  if (form < 0 || form > 2) return fail(ctx, PT_E_INVALID, "pt_download_env: form must be 0, 1 or 2");
  if (!ctx->env.hdr) return fail(ctx, PT_E_INVALID, "pt_download_env: no environment");
  if (form > compactLevel(ctx->env)) return fail(ctx, PT_E_INVALID, "pt_download_env: the environment is not kept in that form");
  if (form == 2 && texels) return fail(ctx, PT_E_INVALID, "pt_download_env: the row form holds no texels");
  if (int rc = syncStreams(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t n = (size_t)ctx->env.w * ctx->env.h;
  if (form == 0) {
    if (texels) CK(hipMemcpy(texels, ctx->env.hdr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (table) CK(hipMemcpy(table, ctx->env.cache, n * sizeof(float2), hipMemcpyDeviceToHost));
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
