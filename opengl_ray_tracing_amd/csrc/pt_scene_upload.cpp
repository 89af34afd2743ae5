// pt_scene_upload.cpp -- pt_upload_scene, pt_update_geometry and pt_update_materials of the C-ABI in
// include/pt_abi.h: what pt_scene_prep.cpp prepared on the host uploaded to every device of a context, the
// runtime's own tree built there (pt_build.hip), the geometry update that refits the uploaded tree in place
// (pt_refit.hip) and the material update that rebuilds the material table in place (pt_materials.hip);
// with them pt_download_node_boxes, pt_download_materials and pt_build_bvh_device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_plan.h"
#include "pt_runtime.h"
#include "pt_scene_prep.h"
#include "pt_update.h"

using namespace pt;

template <class T>
static int upload(pt_ctx* ctx, T** dst, const std::vector<T>& src) {
  dfree(*dst);
  if (src.empty()) return PT_OK;
  CK(hipMalloc(dst, src.size() * sizeof(T)));
  CK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}

// the temporal history shows another scene or another light after an upload
void dropHistory(pt_ctx* ctx) {
  ctx->histValid = false;
  ctx->resolvedFresh = false;
}

// What new geometry invalidates, for an upload and an update alike: the tree / split policies are
// measured again at the next restart, the temporal history and the sample moments saw the old scene,
// the runtime tree is not in place until it is built again (runtimeTreeReady), and the traversal stack
// starts over from the uploaded tree's depth. (sceneVersion stays with the callers: an update bumps
// it whether it has a runtime tree or not, an upload only with one -- runtimeTreeReady.)
// On success each caller's sequence is what it was. On a failure they differ from before in one way:
// the flags and figures are reset here, ahead of the uploads (uploadScene) and of makeRefit and the
// refit launch (updateOne), where both callers used to reset them after those steps -- so a call that
// fails there no longer leaves the old runtime tree marked ready over geometry half replaced.
static int invalidateScene(pt_ctx* ctx, int depth) {
  ctx->policyKey++;
  dropHistory(ctx);
  if (int rc = dropMoments(ctx)) return rc;
  ctx->maxStack = depth + 1;
  ctx->fastReady = false;
  ctx->fast4Ready = false;
  ctx->originLimit = 0.0f;
  ctx->accelDevice = -1;
  ctx->accelMs = 0.0f;
  ctx->accelNodes = ctx->accelDepth = 0;
  return PT_OK;
}

// The runtime's tree built on the device from the geometry records in d_geo (pt_build.hip) and collapsed
// to 4-wide nodes there: pt_upload_scene's build and pt_update_geometry's rebuild. *built false: the
// tree would have 2^24 nodes or more, and the context stays on the uploaded tree.
static int buildRuntimeTree(pt_ctx* ctx, bool* built) {
  *built = false;
  const auto t0 = std::chrono::steady_clock::now();
  AccelBuild ab;
  hipError_t e = buildAccelDevice(ctx->d_geo, ctx->nTri, PT_ACCEL_LEAF, 1e-5f, 3e-5f, ab, ctx->stream);
  if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("device tree build: ") + hipGetErrorString(e));
  if (ab.nNodes + 1 >= (1 << 24)) {  // as the host path: no runtime tree of 2^24 nodes or more
    freeAccelBuild(ab);
    return PT_OK;
  }
  // the 4-wide collapse, on the device too (the large-scene regen kernel's and the megakernel's tree)
  // ... which hands back the scale both encodings widened by, this build's root box's: the origin domain
  // is the domain of the tree in place, after an update's rebuild as after an upload (never a stale scale)
  float4* w4 = nullptr;
  float scale = 0.0f;
  e = collapseWide4Device(ab.nodes, ab.nNodes, PT_ACCEL_LEAF, 1e-5f, 3e-5f, &w4, &ctx->f4Root, &ctx->f4nDev,
                          &ctx->f4Depth, &scale, ctx->stream);
  dfree(ab.nodes);
  if (e != hipSuccess) {
    freeAccelBuild(ab);
    return fail(ctx, PT_E_HIP, std::string("device 4-wide collapse: ") + hipGetErrorString(e));
  }
  dfree(ctx->d_fbvh4);
  ctx->d_fbvh4 = w4;
  dfree(ctx->d_fbvh);
  dfree(ctx->d_fpairs);
  dfree(ctx->d_fastTri);
  ctx->d_fbvh = ab.bvh;
  ctx->d_fpairs = ab.pairs;
  ctx->d_fastTri = ab.order;
  ctx->fRoot = ab.rootRef;
  ctx->fnDev = ab.nDev;
  ctx->fDepth = ab.depth;
  ctx->accelMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ctx->accelDevice = 1;
  ctx->accelNodes = ab.nNodes;
  ctx->originLimit = PT_ORIGIN_K * scale;
  *built = true;
  return PT_OK;
}

// the runtime tree and its 4-wide collapse are in place: the frames may walk them
static void runtimeTreeReady(pt_ctx* ctx) {
  ctx->fast4Ready = true;
  // a visit pushes up to three children: the traversal stack needs 3 entries per wide level
  ctx->maxStack = std::max(ctx->maxStack, 3 * ctx->f4Depth + 2);
  ctx->sceneVersion++;  // camera-ray bins are rebuilt for the new triangles
  ctx->maxStack = std::max(ctx->maxStack, ctx->fDepth + 1);
  ctx->fastReady = true;
}

// pt_update_geometry's device tables and staging belong to one upload
void freeRefit(pt_ctx* ctx) {
  dfree(ctx->refit.topo);
  dfree(ctx->refit.byHeight);
  dfree(ctx->refit.heightStart);
  dfree(ctx->refit.devKids);
  ctx->refit = RefitTables{};
  ctx->refitStart.clear();
  dfree(ctx->d_updVerts);
}

static int uploadScene(pt_ctx* ctx, const float* tris, const SceneHost& h) {
  if (int rc = waitForReaders(ctx)) return rc;  // of the buffers replaced here
  if (int rc = invalidateScene(ctx, h.ref.depth)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  int rc;
  if ((rc = upload(ctx, &ctx->d_pairs, h.pairs)) || (rc = upload(ctx, &ctx->d_geo, h.geo)) ||
      (rc = upload(ctx, &ctx->d_bvh, h.ref.bvh)))
    return rc;
  if ((rc = upload(ctx, &ctx->d_hit, h.hit)) || (rc = upload(ctx, &ctx->d_mats, h.mats))) return rc;
  ctx->nMats = (int)(h.mats.size() / MAT_F4);
  ctx->nTri = h.nTri;
  ctx->nNodes = h.nNodes;
  ctx->nDevNodes = h.ref.nDev;
  ctx->sceneBytes = sceneBytes(ctx->nTri, ctx->nDevNodes);
  // Large Disney/MIS scenes (the regen kernel's, pt_plan.h wideScene) run 4 frames in flight:
  // c5's frames last ~6 ms, and 8 in flight spend more on the pipeline's fill and drain than
  // they gain (bench line, 20 frames from idle: 5.60-5.66 ms per frame at 4 vs 5.88 at 8, 6.00 at 6)
  if (ctx->pipe && !ctx->pipeDepthFixed) ctx->pipeDepth = wideScene(ctx) ? std::min(ctx->pipeDepthBase, 4) : ctx->pipeDepthBase;
  // (the batch's large-scene guard, unlike wideScene, holds under PT_FLAG_NO_CULL too)
  if (ctx->pipe) ctx->batchCap = batchFor(ctx, ctx->cfg.integrator != 0 && largeScene(ctx));
  ctx->rootRef = h.ref.rootRef;
  ctx->depth = h.ref.depth;
  // what pt_update_geometry starts from: the boxes on the device, the topology on the host
  freeRefit(ctx);
  freeMaterialTables(ctx);  // d_mats is the upload's exact table again
  ctx->refTopo = h.topo;
  ctx->refOrder = h.ref.ids;
  ctx->sceneFast = h.fast;
  if ((rc = upload(ctx, &ctx->d_refBox, h.refBox))) return rc;
  if (!h.fast) return PT_OK;
  if ((rc = upload(ctx, &ctx->d_refParent, h.parent)) || (rc = upload(ctx, &ctx->d_leafBox, h.leafBox))) return rc;
  if (h.deviceBuild) {
    bool built = false;
    if ((rc = buildRuntimeTree(ctx, &built)) || !built) return rc;
  } else {
    if ((rc = upload(ctx, &ctx->d_fbvh, h.fastTree.bvh)) || (rc = upload(ctx, &ctx->d_fpairs, h.fpairs)) ||
        (rc = upload(ctx, &ctx->d_fastTri, h.order)))
      return rc;
    ctx->fRoot = h.fastTree.rootRef;
    ctx->fnDev = h.fastTree.nDev;
    ctx->fDepth = h.fastTree.depth;
    ctx->accelMs = h.accelMs;
    ctx->accelDevice = 0;
    ctx->accelNodes = h.accelNodes;
    ctx->originLimit = PT_ORIGIN_K * h.sceneScale;
  }
  ctx->accelDepth = ctx->fDepth;
  // the host-built tree's 4-wide collapse (the device build collapsed on the device above)
  if (!h.deviceBuild) {
    const std::vector<float>& an = h.accelRef;
    const int nn = (int)(an.size() / 12);
    // (the scale of prepareAccel's widening: the root box bounds every vertex, so its largest coordinate
    // magnitude is the triangles')
    std::vector<float4> w4;
    encodeWide4(an.data(), nn, h.nTri, 1e-5f, 3e-5f * h.sceneScale, w4, ctx->f4Root, ctx->f4nDev, ctx->f4Depth);
    if ((rc = upload(ctx, &ctx->d_fbvh4, w4))) return rc;
  }
  runtimeTreeReady(ctx);
  return PT_OK;
}

int pt_upload_scene(pt_ctx* ctx, const float* tris, int nTri, const float* nodes, int nNodes) {
  if (!ctx || !tris || !nodes) return PT_E_INVALID;
  if (nTri < 1 || nNodes < 2) return fail(ctx, PT_E_BADSCENE, "need >= 1 triangle and >= 2 nodes (dummy 0, root 1)");
  if (nTri > MAX_TRIS) return fail(ctx, PT_E_BADSCENE, "too many triangles for the leaf encoding");
  const auto t0 = std::chrono::steady_clock::now();
  SceneHost h;
  std::string bad = prepareScene(tris, nTri, nodes, nNodes, h, (ctx->cfg.flags & PT_FLAG_HOST_ACCEL) != 0);
  if (!bad.empty()) return fail(ctx, PT_E_BADSCENE, bad);
  for (pt_ctx* m : members(ctx))
    if (int rc = uploadScene(m, tris, h)) return fromPeer(ctx, m, rc);
  ctx->uploadMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PT_OK;
}

// ------------------------------------------------------------ geometry update (pt_refit.hip)
// The device tables of the uploaded tree's topology, made at the scene's first update
// (pt_scene_prep.cpp refitTables computes them on the host).
static int makeRefit(pt_ctx* ctx) {
  if (ctx->refit.ready) return PT_OK;
  const RefitHost r = refitTables(ctx->refTopo, ctx->refOrder);
  ctx->refitStart = r.heightStart;
  RefitTables& t = ctx->refit;
  int rc;
  if ((rc = upload(ctx, &t.topo, ctx->refTopo)) || (rc = upload(ctx, &t.byHeight, r.byHeight)) ||
      (rc = upload(ctx, &t.heightStart, r.heightStart)) || (rc = upload(ctx, &t.devKids, r.devKids)))
    return rc;
  t.heights = r.heights;
  t.tailFrom = r.tailFrom;
  t.ready = true;
  return PT_OK;
}

// One context's update from nTri vertex records in its device memory; the caller has waited for the
// frames and queries in flight. What uploadScene invalidates is invalidated here (invalidateScene).
static int updateOne(pt_ctx* ctx, const float* d_verts, int stride) {
  if (int rc = invalidateScene(ctx, ctx->depth)) return rc;
  if (int rc = makeRefit(ctx)) return rc;
  RefitParams p;
  p.verts = d_verts;
  p.stride = stride;
  p.nTri = ctx->nTri;
  p.nDevNodes = ctx->nDevNodes;
  p.geo = ctx->d_geo;
  p.pairs = ctx->d_pairs;
  p.hitRec = ctx->d_hit;
  p.bvh = ctx->d_bvh;
  p.refBox = ctx->d_refBox;
  p.leafBox = ctx->sceneFast ? ctx->d_leafBox : nullptr;
  // PT_UPDATE_TIMES (environment; tools/update_time.py): the device time of each step, on stderr
  StepEvents<4> steps;
  CK(steps.create("PT_UPDATE_TIMES"));
  CK(launchRefit(p, ctx->refit, ctx->refitStart.data(), steps.events(), ctx->stream));
  ctx->sceneVersion++;  // guides and camera-ray bins of the old positions are stale, runtime tree or not
  bool built = false;
  if (ctx->sceneFast) {
    if (int rc = buildRuntimeTree(ctx, &built)) return rc;
  }
  CK(hipStreamSynchronize(ctx->stream));
  if (built) {
    ctx->accelDepth = ctx->fDepth;
    runtimeTreeReady(ctx);
  }
  if (steps.on) {
    float ms[3] = {};
    CK(steps.elapsed(ms));
    std::fprintf(stderr, "pt_update_geometry: records %.4f refit %.4f reencode %.4f build %.4f ms, %d heights, tail from %d\n",
                 ms[0], ms[1], ms[2], ctx->accelMs, ctx->refit.heights, ctx->refit.tailFrom);
  }
  return PT_OK;
}

static int updateArgs(pt_ctx* ctx, const void* verts, int nTri, int stride) {
  if (!ctx || !verts) return PT_E_INVALID;
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT || !ctx->d_bvh) return fail(ctx, PT_E_NOSCENE, "no scene");
  if (nTri != ctx->nTri) return fail(ctx, PT_E_INVALID, "pt_update_geometry: nTriangles differs from the uploaded scene's");
  if (stride < 18) return fail(ctx, PT_E_INVALID, "pt_update_geometry: stride < 18 floats");
  if (ctx->cfg.flags & PT_FLAG_HOST_ACCEL)
    return fail(ctx, PT_E_INVALID, "pt_update_geometry: not on a PT_FLAG_HOST_ACCEL context (the update builds on the GPU)");
  return PT_OK;
}

int pt_update_geometry(pt_ctx* ctx, const float* verts, int nTri, int stride) {
  if (int rc = updateArgs(ctx, verts, nTri, stride)) return rc;
  return updateMembers(ctx, &ctx->uploadMs, [&](pt_ctx* m) {
    if (int rc = stageRecords(m, &m->d_updVerts, verts, nTri, 18, stride, "pt_update_geometry: vertex staging")) return rc;
    return updateOne(m, m->d_updVerts, 18);
  });
}

int pt_update_geometry_device(pt_ctx* ctx, const void* d_verts, int nTri, int stride) {
  if (int rc = updateArgs(ctx, d_verts, nTri, stride)) return rc;
  return updateAlone(ctx, "pt_update_geometry_device", &ctx->uploadMs,
                     [&](pt_ctx* m) { return updateOne(m, static_cast<const float*>(d_verts), stride); });
}

// ------------------------------------------------------------ material update (pt_materials.hip)
void freeMaterialTables(pt_ctx* ctx) {
  MaterialTables& t = ctx->matTab;
  dfree(t.slots);
  dfree(t.slotOf);
  dfree(t.flag);
  dfree(t.rank);
  dfree(t.count);
  dfree(t.scanTmp);
  t = MaterialTables{};
  dfree(ctx->d_updMats);
}

// The update's device tables and a material table with room for one material per triangle, made at the
// scene's first material update. The upload's table stays in place until all of them exist.
static int makeMaterialTables(pt_ctx* ctx) {
  if (ctx->matTab.ready) return PT_OK;
  MaterialTables t;
  const size_t n = (size_t)ctx->nTri;
  t.nSlots = materialSlots(ctx->nTri);
  float4* table = nullptr;
  hipError_t e = materialScanBytes(ctx->nTri, &t.scanBytes);
  if (e == hipSuccess) e = hipMalloc(&t.slots, (size_t)t.nSlots * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&t.slotOf, n * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&t.flag, n * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&t.rank, n * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&t.count, sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&t.scanTmp, std::max<size_t>(t.scanBytes, 16));
  if (e == hipSuccess) e = hipMalloc(&table, n * MAT_F4 * sizeof(float4));
  if (e != hipSuccess) {
    dfree(t.slots); dfree(t.slotOf); dfree(t.flag); dfree(t.rank); dfree(t.count); dfree(t.scanTmp); dfree(table);
    return fail(ctx, PT_E_NOMEM, std::string("pt_update_materials: tables: ") + hipGetErrorString(e));
  }
  dfree(ctx->d_mats);  // the update rewrites every entry in use
  ctx->d_mats = table;
  t.ready = true;
  ctx->matTab = t;
  return PT_OK;
}

// One context's update from nTri material records in its device memory; the caller has waited for the
// frames and queries in flight. Invalidated: the temporal history, the moments and adaptive state
// (as an upload does), and the guides -- by guidesValid alone: sceneVersion, which also makes the
// camera-ray bins rebuild, stays, since the bins hold geometry only. The trees, the traversal stack
// bound, the bins and the measured launch policies stay.
static int updateMaterialsOne(pt_ctx* ctx, const float* d_mats, int stride) {
  dropHistory(ctx);
  if (int rc = dropMoments(ctx)) return rc;
  ctx->guidesValid = false;
  if (int rc = makeMaterialTables(ctx)) return rc;
  MaterialParams p;
  p.mats = d_mats;
  p.stride = stride;
  p.nTri = ctx->nTri;
  p.hitRec = ctx->d_hit;
  p.table = ctx->d_mats;
  // PT_MATERIAL_TIMES (environment; tools/material_time.py): the device time of each step, on stderr
  StepEvents<4> steps;
  CK(steps.create("PT_MATERIAL_TIMES"));
  CK(launchMaterials(p, ctx->matTab, steps.events(), ctx->stream));
  int nMats = 0;
  CK(hipMemcpyAsync(&nMats, ctx->matTab.count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  ctx->nMats = nMats;
  if (steps.on) {
    float ms[3] = {};
    CK(steps.elapsed(ms));
    std::fprintf(stderr, "pt_update_materials: insert %.4f scan %.4f scatter %.4f ms, %d materials, %d slots\n", ms[0], ms[1],
                 ms[2], nMats, ctx->matTab.nSlots);
  }
  return PT_OK;
}

static int materialArgs(pt_ctx* ctx, const void* mats, int nTri, int stride) {
  if (!ctx || !mats) return PT_E_INVALID;
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT || !ctx->d_bvh) return fail(ctx, PT_E_NOSCENE, "no scene");
  if (nTri != ctx->nTri) return fail(ctx, PT_E_INVALID, "pt_update_materials: nTriangles differs from the uploaded scene's");
  if (stride < MAT_KEY) return fail(ctx, PT_E_INVALID, "pt_update_materials: stride < 18 floats");
  return PT_OK;
}

int pt_update_materials(pt_ctx* ctx, const float* mats, int nTri, int stride) {
  if (int rc = materialArgs(ctx, mats, nTri, stride)) return rc;
  return updateMembers(ctx, &ctx->uploadMs, [&](pt_ctx* m) {
    if (int rc = stageRecords(m, &m->d_updMats, mats, nTri, MAT_KEY, stride, "pt_update_materials: record staging")) return rc;
    return updateMaterialsOne(m, m->d_updMats, MAT_KEY);
  });
}

int pt_update_materials_device(pt_ctx* ctx, const void* d_mats, int nTri, int stride) {
  if (int rc = materialArgs(ctx, d_mats, nTri, stride)) return rc;
  return updateAlone(ctx, "pt_update_materials_device", &ctx->uploadMs,
                     [&](pt_ctx* m) { return updateMaterialsOne(m, static_cast<const float*>(d_mats), stride); });
}

int pt_material_count(pt_ctx* ctx, int* nMats) {
  if (!ctx || !nMats) return PT_E_INVALID;
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT || !ctx->d_bvh) return fail(ctx, PT_E_NOSCENE, "no scene");
  *nMats = ctx->nMats;
  return PT_OK;
}

int pt_download_materials(pt_ctx* ctx, float* table, int maxMats, int* ids) {
  if (!ctx || (!table && !ids) || maxMats < 0) return PT_E_INVALID;
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT || !ctx->d_bvh) return fail(ctx, PT_E_NOSCENE, "no scene");
  CK(hipSetDevice(ctx->cfg.device_id));
  const int n = table ? std::min(ctx->nMats, maxMats) : 0;
  std::vector<float4> m((size_t)n * MAT_F4), h(ids ? (size_t)ctx->nTri * HIT_F4 : 0);
  if (n) CK(hipMemcpyAsync(m.data(), ctx->d_mats, m.size() * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  if (ids) CK(hipMemcpyAsync(h.data(), ctx->d_hit, h.size() * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n; k++)  // an entry holds Triangle_encoded floats 16..35: the material is its floats 2..19
    std::memcpy(table + (size_t)k * MAT_KEY, reinterpret_cast<const float*>(&m[(size_t)k * MAT_F4]) + 2, MAT_KEY * sizeof(float));
  if (ids)
    for (int i = 0; i < ctx->nTri; i++) std::memcpy(&ids[i], &h[(size_t)i * HIT_F4 + 2].y, sizeof(int));
  return PT_OK;
}

int pt_download_node_boxes(pt_ctx* ctx, float* boxes) {
  if (!ctx || !boxes) return PT_E_INVALID;
  if (ctx->cfg.integrator == PT_BASIC_CPU_COMPAT || !ctx->d_refBox) return fail(ctx, PT_E_NOSCENE, "no scene");
  CK(hipSetDevice(ctx->cfg.device_id));
  std::vector<float4> b((size_t)ctx->nNodes * 2);
  CK(hipMemcpyAsync(b.data(), ctx->d_refBox, b.size() * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < ctx->nNodes; k++) {
    const float4 lo = b[2 * (size_t)k], hi = b[2 * (size_t)k + 1];
    float* o = boxes + 6 * (size_t)k;
    o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = hi.x; o[4] = hi.y; o[5] = hi.z;
  }
  return PT_OK;
}

int pt_build_bvh_device(pt_ctx* ctx, const float* tris, int nTri, int leafSize, float* nodes_out, int maxNodes,
                        int* nNodesOut, int* orderOut) {
  if (!ctx || !tris || !nodes_out || !nNodesOut || !orderOut || nTri < 1 || leafSize < 1 || leafSize > MAX_LEAF)
    return PT_E_INVALID;
  if (nTri > MAX_TRIS) return fail(ctx, PT_E_BADSCENE, "too many triangles for the leaf encoding");
  if (int rc = syncStreams(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  // the builder reads p1..p3 of the geometry records (the normal and plane offset only feed the pair records)
  std::vector<float4> geo((size_t)nTri * 4, make_float4(0, 0, 0, 0));
  for (int i = 0; i < nTri; i++)
    for (int k = 0; k < 3; k++) {
      const float* v = tris + (size_t)i * 36 + 3 * k;
      geo[4 * (size_t)i + k] = make_float4(v[0], v[1], v[2], 0.0f);
    }
  float4* dgeo = nullptr;
  if (int rc = upload(ctx, &dgeo, geo)) return rc;
  AccelBuild ab;
  hipError_t e = buildAccelDevice(dgeo, nTri, leafSize, 0.0f, 0.0f, ab, ctx->stream);
  dfree(dgeo);
  if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("device tree build: ") + hipGetErrorString(e));
  const int M = ab.nNodes;
  *nNodesOut = M + 1;
  std::vector<BuildNode> bn(M);
  e = hipMemcpy(bn.data(), ab.nodes, (size_t)M * sizeof(BuildNode), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(orderOut, ab.order, (size_t)nTri * sizeof(int), hipMemcpyDeviceToHost);
  freeAccelBuild(ab);
  if (e != hipSuccess) return fail(ctx, PT_E_HIP, std::string("device tree download: ") + hipGetErrorString(e));
  if (M + 1 > maxNodes) return fail(ctx, PT_E_INVALID, "nodes_out holds fewer than *nNodes_out nodes");
  const std::vector<float> ref = refNodes(bn, leafSize);
  std::memcpy(nodes_out, ref.data(), ref.size() * sizeof(float));
  return PT_OK;
}
