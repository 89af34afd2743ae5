// share_table.cpp -- the screen-tile share's arithmetic (opengl_ray_tracing_amd/csrc/pt_frame.h, the
// host half of what every frame kernel calls) as tables: host-only, no HIP library, no device.
// tests/test_share.py holds what the tables must equal.
//
// Output: int32 words on stdout. Per case (size x tile_size x world x rank):
//   width height tile world rank ownedShards slots waveTiles
//   slots x {px, py, inImage, slotOf(px, py)}     pixelOfSlot of slot k = 0 .. slots - 1
//   waveTiles x {x0, y0}                          tileOrigin of wave tile t = 0 .. waveTiles - 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pt_frame.h"

int main() {
  using namespace pt;
  const int sizes[][2] = {{1, 1}, {8, 8}, {33, 31}, {70, 45}, {160, 90}};
  const int tiles[] = {8, 16, 32}, worlds[] = {1, 2, 3, 8};
  std::vector<int32_t> out;
  for (const auto& wh : sizes)
    for (int tile : tiles)
      for (int world : worlds)
        for (int rank = 0; rank < world; rank++) {  // ranks past the last shard tile own nothing
          const Share s = makeShare(wh[0], wh[1], tile, rank, world);
          const long n = slots(s);
          const int nt = waveTiles(s);
          for (int v : {s.width, s.height, s.shardSize, s.world, s.rank, ownedShards(s), (int)n, nt}) out.push_back(v);
          for (long k = 0; k < n; k++) {
            int px, py;
            const bool in = pixelOfSlot(s, k, px, py);
            for (int v : {px, py, (int)in, (int)slotOf(s, px, py)}) out.push_back(v);
          }
          for (int t = 0; t < nt; t++) {
            const int2 o = tileOrigin(s, t);
            out.push_back(o.x);
            out.push_back(o.y);
          }
        }
  return std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
