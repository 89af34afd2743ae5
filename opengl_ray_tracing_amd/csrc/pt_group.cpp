// pt_group.cpp -- the in-process device group of the C-ABI in include/pt_abi.h (pt_config.n_devices >
// 1): its creation and release, the per-frame gather of the ranks' tiles into rank 0's accumulation
// (pt_runtime.h GroupGather) and the waits on it.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_rccl.h"
#include "pt_runtime.h"

using namespace pt;

int createGroup(pt_ctx* ctx) {
  const int n = 1 + (int)ctx->peers.size();
  GroupGather* g = new (std::nothrow) GroupGather();
  if (!g) return fail(ctx, PT_E_NOMEM, "group gather");
  ctx->gather = g;
  g->n = n;
  std::vector<int> devs{ctx->cfg.device_id};
  for (pt_ctx* p : ctx->peers) devs.push_back(p->cfg.device_id);
  bool distinct = true;
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++) distinct = distinct && devs[a] != devs[b];
  const int want = ctx->cfg.gather;
  const Rccl& R = rccl();
  if (want == PT_GATHER_RCCL && (!distinct || !R.ok))
    return fail(ctx, PT_E_INVALID, distinct ? R.err : "PT_GATHER_RCCL needs distinct devices");
  g->mode = (want == PT_GATHER_RCCL || (want == PT_GATHER_AUTO && distinct && R.ok)) ? PT_GATHER_RCCL : PT_GATHER_COPY;
  // peer access lets hipMemcpyPeerAsync go device to device over xGMI (best effort)
  for (int k = 1; k < n; k++)
    if (devs[k] != devs[0]) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devs[0], devs[k]) == hipSuccess && can) {
        (void)hipSetDevice(devs[0]);
        (void)hipDeviceEnablePeerAccess(devs[k], 0);
        (void)hipGetLastError();  // "already enabled" is fine
      }
    }
  CK(hipSetDevice(devs[0]));
  CK(hipStreamCreateWithFlags(&g->cstream, hipStreamNonBlocking));
  CK(hipEventCreateWithFlags(&g->done, hipEventDisableTiming));
  g->peer.resize(n - 1);
  for (int k = 1; k < n; k++) {
    GroupGather::Peer& P = g->peer[k - 1];
    pt_ctx* m = ctx->peers[k - 1];
    P.dev = devs[k];
    P.count = (size_t)packParams(m, k, n).count;
    CK(hipSetDevice(devs[0]));
    if (P.count) CK(hipMalloc(&P.recv, P.count * PACK_F * sizeof(float)));
    // copy mode: the transfer (and its completion event) runs on rank 0's device
    for (int i = 0; i < 2; i++)
      if (g->mode == PT_GATHER_COPY) CK(hipEventCreateWithFlags(&P.sent[i], hipEventDisableTiming));
    CK(hipSetDevice(P.dev));
    for (int i = 0; i < 2; i++) {
      if (P.count) CK(hipMalloc(&P.send[i], P.count * PACK_F * sizeof(float)));
      CK(hipEventCreateWithFlags(&P.packed[i], hipEventDisableTiming));
      if (g->mode == PT_GATHER_RCCL) CK(hipEventCreateWithFlags(&P.sent[i], hipEventDisableTiming));
    }
    if (g->mode == PT_GATHER_RCCL) CK(hipStreamCreateWithFlags(&P.mstream, hipStreamNonBlocking));
  }
  if (g->mode == PT_GATHER_RCCL) {
    ncclResult_t e = R.commInitAll(g->comms, n, devs.data());
    if (e != ncclSuccess) return fail(ctx, PT_E_HIP, std::string("ncclCommInitAll: ") + R.errorString(e));
    g->commsReady = true;
  }
  CK(hipSetDevice(devs[0]));
  return PT_OK;
}

int groupGather(pt_ctx* ctx) {
  GroupGather& g = *ctx->gather;
  const int i = (int)(g.frame++ & 1u);
  const int n = g.n;
  const int dev0 = ctx->cfg.device_id;
  // each rank's tiles of this frame, packed on its render stream behind the frame
  for (int k = 1; k < n; k++) {
    GroupGather::Peer& P = g.peer[k - 1];
    pt_ctx* m = ctx->peers[k - 1];
    if (!P.count) continue;
    if (int rc = joinPipe(m)) return fromPeer(ctx, m, rc);
    CK(hipSetDevice(P.dev));
    if (P.sentValid[i]) CK(hipStreamWaitEvent(m->stream, P.sent[i], 0));
    CK(launchPack(packParams(m, k, n), m->d_accum, P.send[i], m->stream));
    CK(hipEventRecord(P.packed[i], m->stream));
  }
  if (g.mode == PT_GATHER_RCCL) {
    const Rccl& R = rccl();
    for (auto& P : g.peer)
      if (P.count) {
        CK(hipSetDevice(P.dev));
        CK(hipStreamWaitEvent(P.mstream, P.packed[i], 0));
      }
    ncclResult_t e = R.groupStart();
    for (int k = 1; k < n && e == ncclSuccess; k++) {
      GroupGather::Peer& P = g.peer[k - 1];
      if (!P.count) continue;
      e = R.send(P.send[i], P.count * PACK_F, ncclFloat32, 0, g.comms[k], P.mstream);
      if (e == ncclSuccess) e = R.recv(P.recv, P.count * PACK_F, ncclFloat32, k, g.comms[0], g.cstream);
    }
    ncclResult_t e2 = R.groupEnd();
    if (e == ncclSuccess) e = e2;
    if (e != ncclSuccess) return fail(ctx, PT_E_HIP, std::string("RCCL gather: ") + R.errorString(e));
    for (auto& P : g.peer)
      if (P.count) {
        CK(hipSetDevice(P.dev));
        CK(hipEventRecord(P.sent[i], P.mstream));
      }
  } else {
    CK(hipSetDevice(dev0));
    for (auto& P : g.peer) {
      if (!P.count) continue;
      CK(hipStreamWaitEvent(g.cstream, P.packed[i], 0));
      CK(hipMemcpyPeerAsync(P.recv, dev0, P.send[i], P.dev, P.count * PACK_F * sizeof(float), g.cstream));
      CK(hipEventRecord(P.sent[i], g.cstream));
    }
  }
  CK(hipSetDevice(dev0));
  for (int k = 1; k < n; k++) {
    GroupGather::Peer& P = g.peer[k - 1];
    if (P.count) CK(launchUnpack(packParams(ctx, k, n), ctx->d_accum, P.recv, g.cstream));
    P.sentValid[i] = P.count > 0;
  }
  CK(hipEventRecord(g.done, g.cstream));
  g.pending = true;
  return PT_OK;
}

// a device group's rank-0 stream waits for the last gather (the whole image is in its accumulation)
int joinGather(pt_ctx* ctx) {
  GroupGather* g = ctx->gather;
  if (!g || !g->pending) return PT_OK;
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(hipStreamWaitEvent(ctx->stream, g->done, 0));
  return PT_OK;
}

// a group: every device's render stream, the gather's streams, then rank 0's stream
int syncGroup(pt_ctx* ctx) {
  for (pt_ctx* p : ctx->peers)
    if (int rc = syncStreams(p)) return fromPeer(ctx, p, rc);
  if (GroupGather* g = ctx->gather) {
    for (auto& P : g->peer)
      if (P.mstream) {
        CK(hipSetDevice(P.dev));
        CK(hipStreamSynchronize(P.mstream));
      }
    CK(hipSetDevice(ctx->cfg.device_id));
    CK(hipStreamSynchronize(g->cstream));
    g->pending = false;
  }
  return syncStreams(ctx);
}

void destroyGroup(pt_ctx* ctx) {
  GroupGather* g = ctx->gather;
  if (g) {
    if (g->cstream) {
      (void)hipSetDevice(ctx->cfg.device_id);
      (void)hipStreamSynchronize(g->cstream);
    }
    for (auto& P : g->peer) {
      (void)hipSetDevice(P.dev);
      if (P.mstream) (void)hipStreamSynchronize(P.mstream);
    }
    if (g->commsReady)
      for (int k = 0; k < g->n; k++)
        if (g->comms[k]) (void)rccl().commDestroy(g->comms[k]);
    for (auto& P : g->peer) {
      (void)hipSetDevice(P.dev);
      for (int i = 0; i < 2; i++) {
        dfree(P.send[i]);
        if (P.packed[i]) (void)hipEventDestroy(P.packed[i]);
        if (g->mode == PT_GATHER_RCCL && P.sent[i]) (void)hipEventDestroy(P.sent[i]);
      }
      if (P.mstream) (void)hipStreamDestroy(P.mstream);
      (void)hipSetDevice(ctx->cfg.device_id);
      dfree(P.recv);
      for (int i = 0; i < 2; i++)
        if (g->mode == PT_GATHER_COPY && P.sent[i]) (void)hipEventDestroy(P.sent[i]);
    }
    (void)hipSetDevice(ctx->cfg.device_id);
    if (g->done) (void)hipEventDestroy(g->done);
    if (g->cstream) (void)hipStreamDestroy(g->cstream);
    delete g;
    ctx->gather = nullptr;
  }
  for (pt_ctx* p : ctx->peers) pt_destroy(p);
  ctx->peers.clear();
}
