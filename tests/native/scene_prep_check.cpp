// scene_prep_check.cpp -- test infrastructure (tests/test_scene_prep.py): the host-only scene
// preparation of pt_upload_scene (csrc/pt_scene_prep.cpp) run on a scene read from a file, and
// everything it prepared written out. No device and no HIP library: the HIP headers for the vector
// types only.
//
//   scene_prep_check <in> <out>
//   in : int32 nTri, nNodes, hostBuild; nTri x 36 f32 (Triangle_encoded); nNodes x 12 f32 (BVHNode_encoded)
//   out: per array one text line "<name> <f4|i4|u1> <count>\n" followed by the count values' bytes
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_scene_prep.h"

using namespace pt;

static FILE* g_out;

static void dump(const char* name, const char* type, const void* p, size_t count, size_t size) {
  std::fprintf(g_out, "%s %s %zu\n", name, type, count);
  if (count) std::fwrite(p, size, count, g_out);
}
static void dumpF4(const char* name, const std::vector<float4>& v) { dump(name, "f4", v.data(), v.size() * 4, 4); }
static void dumpI(const char* name, const std::vector<int>& v) { dump(name, "i4", v.data(), v.size(), 4); }
static void dumpI2(const char* name, const std::vector<int2>& v) { dump(name, "i4", v.data(), v.size() * 2, 4); }
static void dumpInts(const char* name, std::vector<int> v) { dumpI(name, v); }

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: scene_prep_check <in> <out>\n");
    return 2;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[3];
  if (std::fread(head, sizeof(int32_t), 3, in) != 3 || head[0] < 1 || head[1] < 2) return 2;
  const int nTri = head[0], nNodes = head[1];
  std::vector<float> tris((size_t)nTri * 36), nodes((size_t)nNodes * 12);
  if (std::fread(tris.data(), sizeof(float), tris.size(), in) != tris.size() ||
      std::fread(nodes.data(), sizeof(float), nodes.size(), in) != nodes.size())
    return 2;
  std::fclose(in);
  g_out = std::fopen(argv[2], "wb");
  if (!g_out) return 2;

  SceneHost h;
  const std::string bad = prepareScene(tris.data(), nTri, nodes.data(), nNodes, h, head[2] != 0);
  dump("error", "u1", bad.data(), bad.size(), 1);
  if (bad.empty()) {
    dumpF4("geo", h.geo);
    dumpF4("pairs", h.pairs);
    dumpF4("hit", h.hit);
    dumpF4("mats", h.mats);
    dumpF4("ref.bvh", h.ref.bvh);
    dumpI("ref.ids", h.ref.ids);
    dumpInts("ref.shape", {h.ref.rootRef, h.ref.nDev, h.ref.depth});
    dumpI2("topo", h.topo);
    dumpF4("refBox", h.refBox);
    dumpInts("fast", {h.fast ? 1 : 0, h.deviceBuild ? 1 : 0, h.accelNodes});
    dumpF4("leafBox", h.leafBox);
    dumpI("leafOf", h.leafOf);
    dumpI("parent", h.parent);
    const RefitHost r = refitTables(h.topo, h.ref.ids);
    dumpI("refit.byHeight", r.byHeight);
    dumpI("refit.heightStart", r.heightStart);
    dumpI2("refit.devKids", r.devKids);
    dumpInts("refit.shape", {r.heights, r.tailFrom});
    // the host build (hostBuild, fast): the runtime's own tree, its pair records and their order
    dumpI("order", h.order);
    dumpF4("fastTree.bvh", h.fastTree.bvh);
    dumpI("fastTree.ids", h.fastTree.ids);
    dumpInts("fastTree.shape", {h.fastTree.rootRef, h.fastTree.nDev, h.fastTree.depth});
    dumpF4("fpairs", h.fpairs);
    // ... and the scale its boxes were widened by, which the origin domain is a multiple of (tests/test_accel_domain.py)
    dump("sceneScale", "f4", &h.sceneScale, 1, 4);
    // ... and its nodes before the widening, in the reference encoding (12 floats per node, root 1)
    dump("accelRef", "f4", h.accelRef.data(), h.accelRef.size(), 4);
  }
  return std::fclose(g_out) == 0 ? 0 : 2;
}
