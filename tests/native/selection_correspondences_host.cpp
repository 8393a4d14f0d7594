// Host build of the device-free layout of an export over a SELECTION of kept sets (so_icp_batch_correspondences,
// so_icp_sequence_correspondences), for the CPU suite (tests/test_selection_correspondences_host.py drives it through ctypes; built on
// demand by the test, g++ -O2 -ffp-contract=off like the library):
//   reg_plan.h    selection_tile_table: the prefix table of the entries' tile counts, from their point counts
//                 selection_ticket: which (entry, tile) a workgroup works on, from the ticket it drew and that table
// With -DSELECTION_HOST_MAIN the file is a program of its own that walks the same cases and checks every ticket against a plain scan
// of the table -- the form for a sanitizer build of the layout functions:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DSELECTION_HOST_MAIN
//       -I superodom_amd/csrc tests/native/selection_correspondences_host.cpp -o selection_table_check && ./selection_table_check
#include "reg_plan.h"

using namespace soicp::host;

extern "C" {

// n_points: n_sel point counts (0: an entry without a set); tile_first: n_sel + 1 -> the tiles of the selection
uint32_t sel_tile_table(const uint32_t* n_points, uint32_t n_sel, uint32_t tile, uint32_t* tile_first) {
  return selection_tile_table(n_points, n_sel, tile, tile_first);
}
void sel_ticket(uint32_t t, const uint32_t* tile_first, uint32_t n_sel, uint32_t out[2]) {
  const BatchTicket b = selection_ticket(t, tile_first, n_sel, tile_first[n_sel]);
  out[0] = b.entry; out[1] = b.tile;
}

}  // extern "C"

#ifdef SELECTION_HOST_MAIN
#include <cstdio>
#include <vector>

namespace {

constexpr uint32_t kTile = 1024;  // corr_kernels.h kCorrTile

// -> 0: every ticket of the selection is the (entry, tile) a plain scan of the table names, each worked once, after its predecessors
int check(const std::vector<uint32_t>& n_points) {
  const uint32_t n_sel = (uint32_t)n_points.size();
  std::vector<uint32_t> first(n_sel + 1, 0xDEADBEEFu);
  const uint32_t tiles = selection_tile_table(n_points.data(), n_sel, kTile, first.data());
  uint32_t want = 0;
  for (uint32_t k = 0; k < n_sel; ++k) {
    if (first[k] != want) return 1;
    want += (n_points[k] + kTile - 1) / kTile;
  }
  if (first[n_sel] != want || tiles != want) return 2;
  uint32_t e = 0, tile = 0;  // the plain scan: entry-major, tile after tile
  for (uint32_t t = 0; t < tiles; ++t) {
    while (first[e + 1] <= t) { ++e; tile = 0; }
    const BatchTicket b = selection_ticket(t, first.data(), n_sel, tiles);
    if (b.entry != e || b.tile != tile || first[e] + tile != t) return 3;
    ++tile;
  }
  return 0;
}

}  // namespace

int main() {
  const std::vector<std::vector<uint32_t>> cases = {
      {4096, 4096, 4096, 4096, 4096},     // all entries equal
      {0, 2049, 1025},                    // an entry of 0 points first,
      {2049, 0, 1025},                    // in the middle
      {2049, 1025, 0},                    // and last
      {0, 0, 0, 0},                       // all zero
      {1}, {1024}, {1025},                // at the tile edge
      {1, 1024, 1025, 0, 1025, 1024, 1},
      {},                                 // n_sel = 0
      std::vector<uint32_t>(1024, 1),     // the largest selection of a run
  };
  int bad = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const int rc = check(cases[i]);
    if (rc) { std::printf("case %zu: check %d failed\n", i, rc); ++bad; }
  }
  std::printf("%zu cases, %d failed\n", cases.size(), bad);
  return bad ? 1 : 0;
}
#endif
