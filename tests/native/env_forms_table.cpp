// env_forms_table.cpp -- the view of the environment's store that the kernels get
// (opengl_ray_tracing_amd/csrc/pt_envupdate.h envForms, compactLevel) for stores filled by hand:
// host-only, no HIP library, no device. The pointers are small distinct integers (never followed), printed
// as those integers; one line per case; tests/test_env_forms.py holds the expected values.
#include <cstdint>
#include <cstdio>

#include "pt_envupdate.h"

using namespace pt;

template <class T>
static T* at(uintptr_t k) { return reinterpret_cast<T*>(k); }
static unsigned of(const void* p) { return (unsigned)reinterpret_cast<uintptr_t>(p); }

// every buffer of a 37 x 19 store: hdr 1, cache 2, hdr8 3, cache4 4, cacheRow 5, cacheY 6, trig 7, light 8;
// the buffers no view shows (rowTmp, flags, the update's scratch and staging) 9 ..
static EnvStore full() {
  EnvStore s;
  s.w = 37;
  s.h = 19;
  s.complete = true;
  s.hdr = at<float4>(1);
  s.cache = at<float2>(2);
  s.hdr8 = at<uint2>(3);
  s.cache4 = at<uint32_t>(4);
  s.cacheRow = at<uint32_t>(5);
  s.cacheY = at<unsigned short>(6);
  s.trig = at<float2>(7);
  s.light = at<uint2>(8);
  s.rowTmp = at<int>(9);
  s.flags = at<int>(10);
  s.full = at<float4>(11);
  s.scratch = at<float>(12);
  s.quant = at<float>(13);
  s.stageHdr = at<float>(14);
  s.stageCache = at<float>(15);
  return s;
}

static void show(const char* name, const EnvStore& s, bool compactExact, bool rowsExact) {
  const EnvForms v = envForms(s, compactExact, rowsExact);
  std::printf("%s hdr=%u cache=%u hdr8=%u cache4=%u cacheRow=%u cacheY=%u trig=%u light=%u w=%d h=%d level=%d\n", name,
              of(v.hdr), of(v.cache), of(v.hdr8), of(v.cache4), of(v.cacheRow), of(v.cacheY), of(v.trig), of(v.light), v.w, v.h,
              compactLevel(v));
}

int main() {
  EnvStore s = full();
  s.hdr8 = nullptr;  // the compact forms could not be allocated, or PT_ENV_COMPACT=0: makeStore stops there
  s.cache4 = nullptr;
  s.cacheRow = nullptr;
  s.cacheY = nullptr;
  s.trig = nullptr;
  s.light = nullptr;
  show("no_compact", s, true, true);
  s.trig = at<float2>(7);  // ... and whatever else the store holds does not show without them
  s.light = at<uint2>(8);
  s.cacheRow = at<uint32_t>(5);
  s.cacheY = at<unsigned short>(6);
  show("no_compact_rest_allocated", s, true, true);
  show("compact_bad", full(), false, true);
  show("compact_bad_rows_bad", full(), false, false);
  show("rows_bad", full(), true, false);
  show("exact", full(), true, true);
  s = full();
  s.trig = nullptr;
  show("no_trig", s, true, true);
  s = full();
  s.light = nullptr;
  show("no_light", s, true, true);
  s = full();
  s.cacheRow = nullptr;
  show("no_cache_row", s, true, true);
  s = full();
  s.complete = false;  // an upload's store: only what serves, the same view
  s.rowTmp = s.flags = nullptr;
  show("upload_exact", s, true, true);
  show("empty", EnvStore{}, true, true);
  show("empty_flags_bad", EnvStore{}, false, false);
  return 0;
}
