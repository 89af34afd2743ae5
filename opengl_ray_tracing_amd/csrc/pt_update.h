// pt_update.h -- what the in-place updates share (pt_scene_upload.cpp pt_update_geometry and
// pt_update_materials, pt_env.cpp pt_update_env; pt_upload_scene and pt_upload_env wait the same way):
// the wait for whatever still reads the buffers, the device time of an update's steps, the staging of
// the host forms' strided records, and the two drivers -- every member of a device group for the host
// forms, this context alone for the device forms. An "update X in place" is an argument check, a
// per-context update that takes device memory, and one call of each driver. Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <string>

#include "pt_runtime.h"

#pragma GCC visibility push(hidden)  // the library exports only pt_abi.h's names
// No frame in flight reads the buffers rewritten or freed after this, nor a ray query, whichever stream it is on
static inline int waitForReaders(pt_ctx* ctx) {
  if (int rc = syncStreams(ctx)) return rc;
  if (ctx->queryIssued) CK(hipEventSynchronize(ctx->queryDone));
  return PT_OK;
}

// The device time of an update's steps: N events around N - 1 steps, made only while the environment
// variable `name` is set (PT_UPDATE_TIMES, PT_MATERIAL_TIMES) and destroyed on every way out.
template <int N>
struct StepEvents {
  hipEvent_t ev[N] = {};
  bool on = false;
  ~StepEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(const char* name) {
    on = std::getenv(name) != nullptr;
    hipError_t e = hipSuccess;
    for (int k = 0; on && k < N && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
    return e;
  }
  hipEvent_t* events() { return on ? ev : nullptr; }  // what launchRefit and launchMaterials record into
  hipError_t mark(int k, hipStream_t s) { return on ? hipEventRecord(ev[k], s) : hipSuccess; }
  hipError_t elapsed(float (&ms)[N - 1]) {  // after the stream's synchronisation
    hipError_t e = hipSuccess;
    for (int k = 0; k + 1 < N && e == hipSuccess; k++) e = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    return e;
  }
};

// n records of `width` floats, `stride` floats apart in host memory, packed into *stage on the context's
// stream; *stage is allocated at its first use (nomem: the message when it cannot be)
static inline int stageRecords(pt_ctx* ctx, float** stage, const float* src, int n, int width, int stride, const char* nomem) {
  if (!*stage && hipMalloc(stage, (size_t)n * width * sizeof(float)) != hipSuccess) return fail(ctx, PT_E_NOMEM, nomem);
  CK(hipMemcpy2DAsync(*stage, width * sizeof(float), src, (size_t)stride * sizeof(float), width * sizeof(float), (size_t)n,
                      hipMemcpyHostToDevice, ctx->stream));
  return PT_OK;
}

static inline int makeCurrent(pt_ctx* ctx) {
  CK(hipSetDevice(ctx->cfg.device_id));
  return PT_OK;
}

// The host forms: one(m) for every member m of the group in turn, once nothing reads m's buffers and with
// m's device current (the per-context updates rely on both). wallMs (nullable) takes the wall-clock time of the whole call (pt_frame_stats upload_ms).
template <class One>
static int updateMembers(pt_ctx* ctx, float* wallMs, One one) {
  const auto t0 = std::chrono::steady_clock::now();
  for (pt_ctx* m : members(ctx)) {
    int rc = waitForReaders(m);
    if (!rc) rc = makeCurrent(m);
    if (!rc) rc = one(m);
    if (rc) return fromPeer(ctx, m, rc);
  }
  if (wallMs) *wallMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PT_OK;
}

// The device forms: the caller's memory is on this context's device, so a device group is refused
template <class One>
static int updateAlone(pt_ctx* ctx, const char* call, float* wallMs, One one) {
  if (!ctx->peers.empty()) return fail(ctx, PT_E_INVALID, std::string(call) + ": not on an n_devices > 1 context");
  return updateMembers(ctx, wallMs, one);
}
#pragma GCC visibility pop
