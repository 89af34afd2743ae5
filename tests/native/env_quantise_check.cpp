// Test infrastructure: include/pt_rgbe.h pt_rgbe_quantise -- the function pt_envupdate.hip's kernel calls under
// PT_ENV_RGBE -- on texels read from a file. Host-only.
//
//   env_quantise_check in.bin n out.bin   n texels of 3 f32 in, the same quantised out
//   env_quantise_check                    self check on edge texels (the sanitizer build's run): exit 0 / 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pt_rgbe.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static int selfCheck() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float below = std::nextafterf(PT_RGBE_MIN, 0.0f);
  struct Case {
    float in[3], out[3];
  } cases[] = {
      {{-1.0f, 0.5f, 0.25f}, {0.0f, 0.5f, 0.25f}},
      {{-0.0f, -0.0f, -0.0f}, {0.0f, 0.0f, 0.0f}},
      {{nan, 1.0f, nan}, {0.0f, 1.0f, 0.0f}},
      {{inf, 0.0f, 0.0f}, {PT_RGBE_MAX, 0.0f, 0.0f}},
      {{1e-45f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}},
      {{below, below, 0.0f}, {0.0f, 0.0f, 0.0f}},
      {{PT_RGBE_MAX, 0.0f, 0.0f}, {PT_RGBE_MAX, 0.0f, 0.0f}},
      {{3.0e38f, 1.0f, 0.0f}, {PT_RGBE_MAX, 0.0f, 0.0f}},
      {{0.75f, 0.5f, 0.2501f}, {0.75f, 0.5f, 0.25f}},
  };
  int bad = 0;
  for (const Case& c : cases) {
    float v[3] = {c.in[0], c.in[1], c.in[2]};
    pt_rgbe_quantise(&v[0], &v[1], &v[2]);
    float again[3] = {v[0], v[1], v[2]};
    pt_rgbe_quantise(&again[0], &again[1], &again[2]);
    for (int k = 0; k < 3; k++)
      if (bits(v[k]) != bits(c.out[k]) || bits(again[k]) != bits(v[k])) {
        std::fprintf(stderr, "(%g %g %g)[%d]: %g, expected %g, twice %g\n", c.in[0], c.in[1], c.in[2], k, v[k], c.out[k], again[k]);
        bad = 1;
      }
  }
  // 1e-32f would be stored as 207 * 2^-114, below it: black; 208 * 2^-114 is the smallest texel kept
  float t[3] = {PT_RGBE_MIN, 0.0f, 0.0f}, u[3] = {std::ldexp(208.0f, -114), 0.0f, 0.0f};
  pt_rgbe_quantise(&t[0], &t[1], &t[2]);
  pt_rgbe_quantise(&u[0], &u[1], &u[2]);
  if (t[0] != 0.0f || u[0] != std::ldexp(208.0f, -114)) bad = 1;
  return bad;
}

int main(int argc, char** argv) {
  if (argc == 1) return selfCheck();
  if (argc != 4) {
    std::fprintf(stderr, "usage: env_quantise_check in.bin n out.bin\n");
    return 2;
  }
  const long n = std::atol(argv[2]);
  if (n < 1) return 2;
  std::vector<float> v((size_t)n * 3);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) {
    std::fprintf(stderr, "cannot read %ld texels from %s\n", n, argv[1]);
    return 2;
  }
  std::fclose(f);
  for (long k = 0; k < n; k++) pt_rgbe_quantise(&v[3 * k], &v[3 * k + 1], &v[3 * k + 2]);
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) return 2;
  std::fclose(f);
  return 0;
}
