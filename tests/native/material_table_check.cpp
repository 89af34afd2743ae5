// material_table_check.cpp -- TEST INFRASTRUCTURE: the library's material-table function
// (csrc/pt_scene_prep.cpp materialTable, which prepareScene numbers an upload's materials by and
// pt_update_materials reproduces on the GPU) on records read from a file. Host-only, like scene_prep_check.
//
//   material_table_check FILE N STRIDE    FILE: N records of STRIDE f32 (18: the material floats alone;
//                                          36: whole Triangle_encoded records, materials at floats 18..35)
// prints three lines: the number of distinct keys, every record's id, each id's first record.
// With no arguments it runs a built-in self check (the build under -fsanitize=address,undefined runs that).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_scene_prep.h"

static int selfCheck() {
  // seven records of stride 19 (one float of padding each): keys A B A C(-0 for A's +0) NaN NaN NaN'
  const int n = 7, stride = 19;
  std::vector<float> rec((size_t)n * stride, 0.25f);
  auto word = [&](int i, int k) { return reinterpret_cast<uint32_t*>(&rec[(size_t)i * stride + k]); };
  *word(1, 17) ^= 1u;
  *word(3, 12) = 0x80000000u;
  *word(0, 12) = *word(2, 12) = 0u;
  *word(1, 12) = 0u;
  for (int i = 4; i < 7; i++) *word(i, 16) = i < 6 ? 0x7fc00001u : 0x7fc00002u;
  std::vector<int> ids, first;
  const int m = pt::materialTable(rec.data(), n, stride, ids, first);
  const int wantIds[7] = {0, 1, 0, 2, 3, 3, 4}, wantFirst[5] = {0, 1, 3, 4, 6};
  if (m != 5 || (int)first.size() != 5 || (int)ids.size() != n) return 1;
  for (int i = 0; i < n; i++)
    if (ids[i] != wantIds[i]) return 2;
  for (int k = 0; k < 5; k++)
    if (first[k] != wantFirst[k]) return 3;
  if (pt::materialTable(rec.data(), 0, stride, ids, first) != 0 || !ids.empty() || !first.empty()) return 4;
  std::puts("ok");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return selfCheck();
  if (argc != 4) return 2;
  const int n = std::atoi(argv[2]), stride = std::atoi(argv[3]);
  if (n < 0 || stride < 18) return 2;
  std::vector<float> rec((size_t)n * stride);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  const size_t got = std::fread(rec.data(), sizeof(float), rec.size(), f);
  std::fclose(f);
  if (got != rec.size()) return 3;
  std::vector<int> ids, first;
  const int m = pt::materialTable(rec.data() + (stride >= 36 ? 18 : 0), n, stride, ids, first);
  std::printf("%d\n", m);
  for (int id : ids) std::printf("%d ", id);
  std::printf("\n");
  for (int i : first) std::printf("%d ", i);
  std::printf("\n");
  return 0;
}
