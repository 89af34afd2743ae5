// pt_envupdate.h -- the environment updated in place (pt_envupdate.hip; pt_abi.h pt_update_env): the
// buffers one (w, h) keeps from update to update and the device steps between the caller's w*h*3
// floats and the Env the frame kernels read. Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"

namespace pt {

// What pt_update_env keeps on the device for maps of one size. The context's env pointers (pt_runtime.h
// d_hdr .. d_light) are views of these buffers, or null where a form does not serve the current map.
struct EnvStore {
  int w = 0, h = 0;                 // 0: no store (the env, if any, is pt_upload_env's own)
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
