// pt_accum.cpp -- access to the accumulation of the C-ABI in include/pt_abi.h: download, upload and
// clear, adaptive sampling's update and status (the frames' side of it is pt_runtime.cpp), the tonemap,
// and the pack / unpack / display calls of a screen-tile split across processes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_plan.h"
#include "pt_runtime.h"

using namespace pt;

int pt_download_accum(pt_ctx* ctx, float* accum) {
  if (!ctx || !accum) return PT_E_INVALID;
  if (int rc = joinGather(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t bytes = (size_t)ctx->cfg.width * ctx->cfg.height * sizeof(float4);
  CK(hipMemcpyAsync(accum, ctx->d_accum, bytes, hipMemcpyDefault, ctx->stream));  // host or device
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

static int uploadAccumOne(pt_ctx* ctx, const float* accum) {
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t npix = (size_t)ctx->cfg.width * ctx->cfg.height;
  CK(hipMemcpyAsync(ctx->d_accum, accum, npix * sizeof(float4), hipMemcpyDefault, ctx->stream));  // host or device
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT) {  // basicKernel continues from its double image: the sums, widened
    if (int rc = ensureBasicImage(ctx)) return rc;
    CK(launchBasicWiden(ctx->d_accum, ctx->d_basicImg, (long)npix, ctx->stream));
  }
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

// (every device of a group takes the whole image: each continues the running mean of its own tiles)
int pt_upload_accum(pt_ctx* ctx, const float* accum) {
  if (!ctx || !accum) return PT_E_INVALID;
  if (int rc = joinGather(ctx)) return rc;
  if (int rc = dropMoments(ctx)) return rc;
  for (pt_ctx* m : members(ctx))
    if (int rc = uploadAccumOne(m, accum)) return fromPeer(ctx, m, rc);
  return PT_OK;
}

int pt_clear_accum(pt_ctx* ctx) {
  if (!ctx) return PT_E_INVALID;
  if (int rc = joinGather(ctx)) return rc;
  for (pt_ctx* m : members(ctx)) {
    if (int rc = joinPipe(m)) return fromPeer(ctx, m, rc);
    if (hipSetDevice(m->cfg.device_id) != hipSuccess ||
        hipMemsetAsync(m->d_accum, 0, (size_t)m->cfg.width * m->cfg.height * sizeof(float4), m->stream) != hipSuccess)
      return fail(ctx, PT_E_HIP, "pt_clear_accum on device " + std::to_string(m->cfg.device_id));
    if (m->d_basicImg &&
        hipMemsetAsync(m->d_basicImg, 0, (size_t)m->cfg.width * m->cfg.height * 3 * sizeof(double), m->stream) != hipSuccess)
      return fail(ctx, PT_E_HIP, "pt_clear_accum (BASIC image)");
    if (int rc = dropMoments(m)) return fromPeer(ctx, m, rc);
    if (m->d_mom &&
        hipMemsetAsync(m->d_mom, 0, (size_t)m->cfg.width * m->cfg.height * sizeof(float2), m->stream) != hipSuccess)
      return fail(ctx, PT_E_HIP, "pt_clear_accum (moments)");
  }
  // a group's next gather unpacks into rank 0's accumulation on the gather stream, which
  // is not ordered after rank 0's stream: the clear completes first
  if (ctx->gather) {
    CK(hipSetDevice(ctx->cfg.device_id));
    CK(hipStreamSynchronize(ctx->stream));
  }
  return PT_OK;
}

// ------------------------------------------------------------ adaptive sampling
static_assert(sizeof(pt_adaptive_params) == PT_ADAPTIVE_PARAMS_SIZE, "pt_adaptive_params layout");
static_assert(sizeof(pt_adaptive_state) == PT_ADAPTIVE_STATE_SIZE, "pt_adaptive_state layout");

void pt_adaptive_defaults(pt_adaptive_params* prm) {
  if (!prm) return;
  prm->threshold = 1.0f / 255.0f;
  prm->limit = 1.5f;
  prm->min_frames = 16;
}

int pt_adaptive_params_size(void) { return (int)sizeof(pt_adaptive_params); }
int pt_adaptive_state_size(void) { return (int)sizeof(pt_adaptive_state); }

int pt_adaptive_update(pt_ctx* ctx, const pt_adaptive_params* prm) {
  if (!ctx) return PT_E_INVALID;
  if (!ctx->d_retiredAt) return fail(ctx, PT_E_INVALID, "pt_adaptive_update: not a PT_FLAG_ADAPTIVE context");
  pt_adaptive_params P;
  pt_adaptive_defaults(&P);
  if (prm) P = *prm;
  if (!(P.threshold > 0.0f) || !std::isfinite(P.threshold))
    return fail(ctx, PT_E_INVALID, "pt_adaptive_update: threshold must be > 0 and finite");
  if (!(P.limit > 0.0f)) return fail(ctx, PT_E_INVALID, "pt_adaptive_update: limit must be > 0");
  if (P.min_frames < 2) return fail(ctx, PT_E_INVALID, "pt_adaptive_update: min_frames must be >= 2");
  if (ctx->momFrames == 0)
    return fail(ctx, PT_E_INVALID, "pt_adaptive_update: the moments are not valid (pt_moments_frames is 0: render from frameCounter 0)");
  // tiles retire in the camera-ray pass: a context whose launches cannot run it retires nothing
  if (!planFrame(ctx, false, 2).bins)
    return fail(ctx, PT_E_INVALID, "pt_adaptive_update: this context's frames run no camera-ray pass (no camera-ray bins for its scene)");
  // after every launch so far has updated the running mean -- and so after their passes read the planes.
  // (A share reads its own pixels only: rank 0's update needs no ordering against an unpack of the
  // other ranks' pixels in flight on a communication stream.)
  if (int rc = joinPipe(ctx)) return rc;
  if (int rc = joinAdaptive(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  TileErrorParams t;
  t.share = shareOf(ctx, ctx->cfg.tile_rank, ctx->cfg.tile_world);
  t.shardTiles = shardTiles(t.share);
  t.waveTiles = waveTiles(t.share);
  t.tilesX = ctx->adaptTilesX;
  t.accum = ctx->d_accum;
  t.moments = ctx->d_mom;
  t.err2 = ctx->d_err2;
  t.retiredAt = ctx->d_retiredAt;
  t.kf = (float)ctx->momFrames;
  t.limit = P.limit;
  t.thr2 = P.threshold * P.threshold;
  t.frames = ctx->momFrames;
  t.minFrames = P.min_frames;
  CK(launchTileError(t, ctx->stream));
  CK(hipEventRecord(ctx->adaptDone, ctx->stream));
  ctx->adaptStream = ctx->stream;
  ctx->adaptGen++;
  ctx->adaptDirty = true;
  ctx->adaptFrames = ctx->momFrames;
  return PT_OK;
}

// the two tile planes on the host, after the frames and updates so far
static int adaptivePlanes(pt_ctx* ctx, std::vector<float>& err2, std::vector<uint32_t>& retiredAt) {
  if (int rc = joinPipe(ctx)) return rc;
  if (int rc = joinAdaptive(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  err2.resize(ctx->adaptTiles);
  retiredAt.resize(ctx->adaptTiles);
  CK(hipMemcpyAsync(err2.data(), ctx->d_err2, err2.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(retiredAt.data(), ctx->d_retiredAt, retiredAt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

int pt_adaptive_status(pt_ctx* ctx, pt_adaptive_state* st) {
  if (!ctx) return PT_E_INVALID;
  if (!st) return fail(ctx, PT_E_INVALID, "pt_adaptive_status: null status");
  if (!ctx->d_retiredAt) return fail(ctx, PT_E_INVALID, "pt_adaptive_status: not a PT_FLAG_ADAPTIVE context");
  std::vector<float> err2;
  std::vector<uint32_t> retiredAt;
  if (int rc = adaptivePlanes(ctx, err2, retiredAt)) return rc;
  // over the image tiles of this context's share (every tile with tile_world 1): a shard tile's edge
  // is a multiple of 8, so a tile's first pixel names its owner
  const Share sh = shareOf(ctx, ctx->cfg.tile_rank, ctx->cfg.tile_world);
  st->tiles = 0;
  st->retired = 0;
  st->frames = ctx->adaptFrames;
  st->max_err2 = 0.0f;
  for (int k = 0; k < ctx->adaptTiles; k++) {
    const int ty = k / ctx->adaptTilesX, tx = k - ty * ctx->adaptTilesX;
    const int g = (ty * 8 / sh.shardSize) * sh.shardsX + tx * 8 / sh.shardSize;
    if (g % sh.world != sh.rank) continue;
    st->tiles++;
    if (retiredAt[k] != 0u) st->retired++;
    else st->max_err2 = err2[k] > st->max_err2 ? err2[k] : st->max_err2;
  }
  return PT_OK;
}

int pt_download_tile_error(pt_ctx* ctx, float* err2, uint32_t* retired_at) {
  if (!ctx) return PT_E_INVALID;
  if (!ctx->d_retiredAt) return fail(ctx, PT_E_INVALID, "pt_download_tile_error: not a PT_FLAG_ADAPTIVE context");
  if (int rc = joinPipe(ctx)) return rc;
  if (int rc = joinAdaptive(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const size_t n = (size_t)ctx->adaptTiles;
  if (err2) CK(hipMemcpyAsync(err2, ctx->d_err2, n * sizeof(float), hipMemcpyDefault, ctx->stream));  // host or device
  if (retired_at) CK(hipMemcpyAsync(retired_at, ctx->d_retiredAt, n * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

int pt_accum_device_ptr(pt_ctx* ctx, void** dptr) {
  if (!ctx || !dptr) return PT_E_INVALID;
  *dptr = ctx->d_accum;
  return PT_OK;
}

int pt_tonemap(pt_ctx* ctx, float limit, float gamma, float* rgb_out) {
  if (!ctx || !rgb_out || !(limit > 0.0f)) return PT_E_INVALID;
  if (int rc = joinGather(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  const int n = ctx->cfg.width * ctx->cfg.height;
  if (!ctx->d_rgb) CK(hipMalloc(&ctx->d_rgb, (size_t)n * 3 * sizeof(float)));
  CK(launchTonemap(ctx->d_accum, ctx->d_rgb, n, limit, gamma, ctx->stream));
  CK(hipMemcpyAsync(rgb_out, ctx->d_rgb, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return PT_OK;
}

// ------------------------------------------------------------ pack, unpack and display of a screen-tile split
// an in-process device group packs and unpacks its ranks' tiles itself (pt_group.cpp)
static int notGroup(pt_ctx* ctx) {
  return ctx->peers.empty() ? PT_OK : fail(ctx, PT_E_INVALID, "device groups gather inside pt_render_frame");
}

// rank 0's unpack of ranks 1..world-1's packed buffers in one launch
static RanksUnpack ranksUnpack(const pt_ctx* ctx, int world, const void* const* dpacked) {
  RanksUnpack d;
  std::memset(&d, 0, sizeof(d));
  d.base = packParams(ctx, 0, world);
  for (int k = 1; k < world; k++) {
    d.src[k] = dpacked[k];
    d.count[k] = packParams(ctx, k, world).count;
  }
  return d;
}

int pt_owned_pixel_count(pt_ctx* ctx, int rank, int world, int64_t* count) {
  if (!ctx || !count || world < 1 || rank < 0 || rank >= world) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  *count = packParams(ctx, rank, world).count;
  return PT_OK;
}

int pt_pack_owned(pt_ctx* ctx, void* dpacked) {
  if (!ctx || !dpacked) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  PackParams p = packParams(ctx, ctx->cfg.tile_rank, ctx->cfg.tile_world);
  CK(launchPack(p, ctx->d_accum, reinterpret_cast<float*>(dpacked), ctx->stream));
  return PT_OK;
}

int pt_display_pack(pt_ctx* ctx, float limit, float gamma, void* dpacked) {
  if (!ctx || !dpacked || !(limit > 0.0f)) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  PackParams p = packParams(ctx, ctx->cfg.tile_rank, ctx->cfg.tile_world);
  CK(launchDisplayPack(p, ctx->d_accum, limit, gamma, reinterpret_cast<uint8_t*>(dpacked), ctx->stream));
  return PT_OK;
}

int pt_display_own(pt_ctx* ctx, float limit, float gamma, void* dimage) {
  if (!ctx || !dimage || !(limit > 0.0f)) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  PackParams p = packParams(ctx, ctx->cfg.tile_rank, ctx->cfg.tile_world);
  CK(launchDisplayOwn(p, ctx->d_accum, limit, gamma, reinterpret_cast<uchar4*>(dimage), ctx->stream));
  return PT_OK;
}

int pt_display_unpack(pt_ctx* ctx, int world, const void* const* dpacked, void* dimage) {
  if (!ctx || !dpacked || !dimage || world < 1 || world > DISPLAY_MAX_WORLD) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(launchDisplayUnpack(ranksUnpack(ctx, world, dpacked), world, reinterpret_cast<uchar4*>(dimage), ctx->stream));
  return PT_OK;
}

// Another rank's pixels were written into the accumulation. A plain context's moments no longer
// describe it (they were this context's own samples of those pixels). A PT_FLAG_SHARE_MOMENTS
// context's moments and tile planes are of its own pixels and tiles only, which an unpack does not
// write: they stay valid -- rank 0 unpacks after every batch
static int unpackedOthers(pt_ctx* ctx) {
  if (ctx->cfg.flags & PT_FLAG_SHARE_MOMENTS) return PT_OK;
  return dropMoments(ctx);
}

int pt_unpack_ranks(pt_ctx* ctx, int world, const void* const* dpacked) {
  if (!ctx || !dpacked || world < 1 || world > DISPLAY_MAX_WORLD) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(launchUnpackRanks(ranksUnpack(ctx, world, dpacked), world, ctx->d_accum, ctx->stream));
  if (int rc = unpackedOthers(ctx)) return rc;
  return PT_OK;
}

int pt_unpack_rank(pt_ctx* ctx, int rank, int world, const void* dpacked) {
  if (!ctx || !dpacked || world < 1 || rank < 0 || rank >= world) return PT_E_INVALID;
  if (int rc = notGroup(ctx)) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  PackParams p = packParams(ctx, rank, world);
  CK(launchUnpack(p, ctx->d_accum, reinterpret_cast<const float*>(dpacked), ctx->stream));
  if (int rc = unpackedOthers(ctx)) return rc;
  return PT_OK;
}

// The gather of a PT_FLAG_SHARE_MOMENTS split: the running means with the moments, 5 f32 per slot
static int shareMomentsOnly(pt_ctx* ctx, const char* what) {
  if (int rc = notGroup(ctx)) return rc;
  if (!(ctx->cfg.flags & PT_FLAG_SHARE_MOMENTS) || !ctx->d_mom)
    return fail(ctx, PT_E_INVALID, std::string(what) + ": not a PT_FLAG_SHARE_MOMENTS context");
  return PT_OK;
}

int pt_pack_owned_stats(pt_ctx* ctx, void* dpacked) {
  if (!ctx) return PT_E_INVALID;
  if (!dpacked) return fail(ctx, PT_E_INVALID, "pt_pack_owned_stats: null buffer");
  if (int rc = shareMomentsOnly(ctx, "pt_pack_owned_stats")) return rc;
  if (int rc = joinPipe(ctx)) return rc;  // after the frames rendered so far, as pt_pack_owned
  CK(hipSetDevice(ctx->cfg.device_id));
  PackParams p = packParams(ctx, ctx->cfg.tile_rank, ctx->cfg.tile_world);
  CK(launchPackStats(p, ctx->d_accum, ctx->d_mom, reinterpret_cast<float*>(dpacked), ctx->stream));
  return PT_OK;
}

// On the caller's stream, which may be a communication stream while the next launch renders: that
// launch's running-mean update writes only this rank's pixels, this only the others'
int pt_unpack_ranks_stats(pt_ctx* ctx, int world, const void* const* dpacked) {
  if (!ctx) return PT_E_INVALID;
  if (!dpacked || world < 1 || world > DISPLAY_MAX_WORLD)
    return fail(ctx, PT_E_INVALID, "pt_unpack_ranks_stats: world must be 1..16 and the buffer list not null");
  if (int rc = shareMomentsOnly(ctx, "pt_unpack_ranks_stats")) return rc;
  if (int rc = joinPipe(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(launchUnpackRanksStats(ranksUnpack(ctx, world, dpacked), world, ctx->d_accum, ctx->d_mom, ctx->stream));
  return PT_OK;
}
