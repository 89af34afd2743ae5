// pt_envupdate.h -- the environment updated in place (pt_envupdate.hip; pt_abi.h pt_update_env): the
// buffers one (w, h) keeps from update to update and the device steps between the caller's w*h*3
// floats and the Env the frame kernels read. Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"

namespace pt {

// The environment's device buffers, whichever call made them: the store owns them all (pt_env.cpp freeStore
// is the one place they are freed) and the context's EnvForms is a view of it. Two states beside empty:
// pt_update_env's store is complete -- every form allocated, so a later map of the same size allocates
// nothing --, pt_upload_env's holds only the forms that serve its map.
struct EnvStore {
  int w = 0, h = 0;                 // 0: no environment
  bool complete = false;            // every form allocated (makeStore's; an upload's store is not)
  float4* hdr = nullptr;            // w*h (r, g, b, pdf)
  float2* cache = nullptr;          // w*h (x, y)
  uint2* hdr8 = nullptr;            // the compact forms: both or neither (w, h <= 65535)
  uint32_t* cache4 = nullptr;
  uint32_t* cacheRow = nullptr;     // h; with hdr8
  unsigned short* cacheY = nullptr; // w*h: room for every row distinct
  int* rowTmp = nullptr;            // 65536 first rows by x, then h leader ids
  float2* trig = nullptr;           // w + h + 2; null: could not be allocated, computed in the kernels
  bool trigReady = false;           // ... and filled: it depends on (w, h) only
  uint2* light = nullptr;           // (w + 1)(h + 1); null likewise
  int* flags = nullptr;             // ENV_FLAGS ints, read back once per update
  // made at the first update that needs them
  float4* full = nullptr;           // the library's table as launchHdrCache writes it (w*h float4)
  float* scratch = nullptr;         // ... and its scratch (2*w*h + 2*w + 1 floats)
  float* quant = nullptr;           // w*h*3: the quantised texels launchHdrCache reads (PT_ENV_RGBE, no caller's table)
  float* stageHdr = nullptr;        // the host form's staging: w*h*3 texels
  float* stageCache = nullptr;      // ... and w*h*3 table entries
};

// The forms that serve the current map: what envView copies from. Null where a form does not serve.
struct EnvForms {
  float4* hdr = nullptr;
  float2* cache = nullptr;            // sample table (x, y); the pdf lives in hdr[k].w
  uint2* hdr8 = nullptr;              // the same texels compacted (pt_kernels.h Env), null = not exact
  uint32_t* cache4 = nullptr;
  uint32_t* cacheRow = nullptr;       // the sample table by rows (Env::cacheRow)
  unsigned short* cacheY = nullptr;
  float2* trig = nullptr;             // SampleHdr's sines and cosines (Env::trig)
  uint2* light = nullptr;             // each sample-table entry's light-sample color and pdf (Env::light)
  int w = 0, h = 0;
};

// The hand-over, the one place a view is made: the forms of store k that serve its map, given what was read
// back about it -- the compact forms decode to the float bits (compactExact), every entry equals its row
// form (rowsExact). The empty store gives the empty view.
inline EnvForms envForms(const EnvStore& k, bool compactExact, bool rowsExact) {
  EnvForms v;
  if (!k.hdr) return v;
  const bool compact = k.hdr8 && compactExact, rows = compact && k.cacheRow && rowsExact;
  v.hdr = k.hdr;
  v.cache = k.cache;
  v.hdr8 = compact ? k.hdr8 : nullptr;
  v.cache4 = compact ? k.cache4 : nullptr;
  v.trig = compact ? k.trig : nullptr;
  v.light = compact && k.trig ? k.light : nullptr;
  v.cacheRow = rows ? k.cacheRow : nullptr;
  v.cacheY = rows ? k.cacheY : nullptr;
  v.w = k.w;
  v.h = k.h;
  return v;
}

inline int compactLevel(const EnvForms& v) { return v.hdr8 ? (v.cacheRow ? 2 : 1) : 0; }  // pt_frame_stats.env_compact

constexpr int ENV_FLAGS = 4;        // flags[]: texels or table not compact, rows not in row form, distinct rows
constexpr int ENV_BAD = 0, ENV_ROWS_BAD = 1, ENV_ROW_IDS = 2;
constexpr int ENV_X_SLOTS = 65536;  // a compact table's x is a 16-bit integer

// hdr[k] = (src3[3k..3k+2] -- through pt_rgbe_quantise if rgbe --, cache3 ? cache3[3k+2] : 0), and with
// cache3 samp[k] = cache3[3k], cache3[3k+1]; quant3 (nullable) takes the three colour floats as written
hipError_t launchEnvTexels(const float* src3, const float* cache3, int rgbe, float4* hdr, float2* samp, float* quant3,
                           int n, hipStream_t s);
// The sample table by rows from the compact table cache4 (pt_kernels.h Env::cacheRow / cacheY): st.cacheRow,
// st.cacheY, and in st.flags ENV_ROWS_BAD (some entry differs from its row form) and ENV_ROW_IDS (distinct
// rows, numbered by first appearance in row order). Any cache4 contents are in bounds. h <= 65535.
hipError_t launchEnvRows(const EnvStore& st, hipStream_t s);
// diagnostic (pt_download_env forms 1 and 2): the texels and table decoded by the frame kernels' decoders
// from the compact forms (form 1) or the table alone through the row form (form 2); outputs nullable
hipError_t launchEnvDecode(const Env& e, int form, float4* texels, float2* table, hipStream_t s);

}  // namespace pt
