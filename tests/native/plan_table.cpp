// plan_table.cpp -- the frame path's launch policy (opengl_ray_tracing_amd/csrc/pt_plan.h) on
// contexts filled by hand: host-only, no HIP library, no device. One line per case;
// tests/test_frame_plan.py holds the expected values.
#include <cstdio>

#include "pt_plan.h"

static const size_t LARGE = ((size_t)PT_WIDE_SCENE_MB << 20) + 1, SMALL = 1u << 20;

// a context as pt_create and the uploads leave it: 1920 x 1080, tile_world 1, a small scene with both
// runtime trees, env 1024 x 512, the regen default
static pt_ctx make(int integrator, int maxBounce = -1, unsigned flags = 0, int tileWorld = 1) {
  pt_ctx x;
  pt_config& c = x.cfg;
  c.width = 1920;
  c.height = 1080;
  c.integrator = integrator;
  c.max_bounce = maxBounce;
  c.flags = flags;
  c.tile_world = tileWorld;
  const Share share = makeShare(c.width, c.height, x.shardSize, c.tile_rank, c.tile_world);
  x.shardsX = share.shardsX;
  x.shardsY = shardsY(share);
  x.numItems = waveTiles(share);
  x.perQueue = (x.numItems + NUM_QUEUES - 1) / NUM_QUEUES;
  x.pipe = pipelines(c);
  x.regenWide = -1;
  x.fastReady = x.fast4Ready = true;
  x.sceneBytes = SMALL;
  x.hdrW = 1024;
  x.hdrH = 512;
  return x;
}

static void plan(int n, const pt_ctx& x, bool solo, int want) {
  const FramePlan f = planFrame(&x, solo, want);
  std::printf("plan %d count=%d cull=%d wideScene=%d regenAll=%d oneCall=%d regen=%d wide=%d walk4=%d pass=%d bins=%d "
              "rowTable=%d envNt=%d ordered=%d piped=%d\n",
              n, f.count, f.cull, f.wideScene, f.regenAll, f.oneCall, f.regen, f.wide, f.walk4, f.pass, f.bins, f.rowTable,
              f.envNt, f.ordered, f.piped);
}

// the batch of a context at pipe depths 3 and 4, with the large-scene argument uploadScene passes
static void batch(const char* name, pt_ctx x) {
  const bool large = x.cfg.integrator != 0 && largeScene(&x);
  x.pipeDepth = 3;
  const int few = batchFor(&x, large);
  x.pipeDepth = 4;
  std::printf("batch %s %d %d\n", name, few, batchFor(&x, large));
}

int main() {
  const int L = PT_LAMBERT_O, D = PT_DISNEY_UNIFORM_D, M = PT_DISNEY_MIS_SOBOL_IS;
  // a row that names neither `want` nor solo: 4 frames wanted while others are in flight
  const bool solo = true, busy = false;
  pt_ctx x;
  plan(1, make(L), solo, 12);
  plan(2, make(L), solo, 1);
  plan(3, make(L), busy, 1);
  plan(4, make(L, -1, PT_FLAG_REGEN), solo, 1);
  plan(5, make(D), busy, 16);
  plan(6, make(D, -1, PT_FLAG_REGEN), busy, 4);
  plan(7, make(D, -1, PT_FLAG_REGEN | PT_FLAG_PRIMARY_PASS), busy, 4);
  plan(8, make(M), busy, 16);
  x = make(M, 8);
  x.hdrW = 2048, x.hdrH = 1024;
  plan(9, x, busy, 4);
  plan(90, make(M, 8), busy, 4);  // row 9 with env 1024 x 512
  x = make(M);
  x.sceneBytes = LARGE;
  plan(10, x, solo, 1);
  x.cfg.flags = PT_FLAG_MEGAKERNEL;
  plan(11, x, solo, 1);
  x.cfg.flags = PT_FLAG_REFERENCE_TREE;
  plan(12, x, solo, 1);
  x = make(L);
  x.sceneBytes = LARGE;
  plan(13, x, solo, 1);
  plan(14, make(L, -1, PT_FLAG_COUNT_FETCHES | PT_FLAG_REGEN), busy, 4);
  plan(15, make(L, -1, PT_FLAG_NO_CULL), busy, 4);
  x = make(D);
  x.regenWide = 1;
  plan(16, x, solo, 1);
  x = make(L);
  x.regenWide = 0;
  plan(17, x, busy, 4);
  plan(18, make(L, -1, PT_FLAG_SERIAL_FRAMES), busy, 4);
  plan(19, make(L, -1, PT_FLAG_NO_BINS), busy, 12);
  x = make(M, 8);
  x.fastReady = x.fast4Ready = false;
  plan(20, x, busy, 4);

  batch("lambert", make(L));
  batch("mis2", make(M, 2));
  batch("mis8", make(M, 8));
  batch("disney", make(D));
  x = make(D);
  x.sceneBytes = LARGE;
  batch("large_disney", x);
  x = make(M);
  x.sceneBytes = LARGE;
  batch("large_mis", x);
  batch("lambert_world8", make(L, -1, 0, 8));
  batch("mis8_world2", make(M, 8, 0, 2));
  x = make(L);
  x.cfg.frame_batch = 5;
  batch("frame_batch5", x);

  std::printf("depth lambert 12 %d\n", pipeDepthFor(make(L).cfg, -1, 12));
  std::printf("depth lambert 4 %d\n", pipeDepthFor(make(L).cfg, -1, 4));
  std::printf("depth mis 12 %d\n", pipeDepthFor(make(M).cfg, -1, 12));
  std::printf("depth lambert_world8 12 %d\n", pipeDepthFor(make(L, -1, 0, 8).cfg, -1, 12));
  std::printf("depth lambert_regenwide0 12 %d\n", pipeDepthFor(make(L).cfg, 0, 12));
  return 0;
}
