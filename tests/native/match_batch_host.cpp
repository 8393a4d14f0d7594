// Host build of what so_icp_match_batch adds to the device-free headers, for the CPU suite (tests/test_match_batch_host.py drives it through
// ctypes; built on demand by the test, g++ -O2 -ffp-contract=off like the library):
//   reg_plan.h    match_batch_slot: which (hypothesis of the launch's list, virtual workgroup) workgroup b of match_batch_kernel serves
//                 match_batch_partial_word, match_batch_ticket_word: where a hypothesis keeps the records of that launch and counts them
//                 refused_prior: the entry takes no prior, so whatever kind is pending refuses it
// Also a program of its own (main below walks the same grids and returns the number of violations): built without -shared it can be
// run directly, under -fsanitize=address,undefined for instance.
#include <cstdio>
#include <vector>

#include "reg_plan.h"

using namespace soicp::host;

extern "C" {

void mb_slot(uint32_t b, uint32_t V, uint32_t out[2]) {
  const MatchBatchSlot s = match_batch_slot(b, V);
  out[0] = s.entry; out[1] = s.vb;
}
unsigned long long mb_partial_word(unsigned long long h, uint32_t partial_stride, uint32_t a, uint32_t vb, uint32_t max_grid) {
  return (unsigned long long)match_batch_partial_word((size_t)h, partial_stride, a, vb, max_grid);
}
unsigned long long mb_ticket_word(unsigned long long h, uint32_t sync_stride) { return (unsigned long long)match_batch_ticket_word((size_t)h, sync_stride); }
// pending: kPriorSingle, kPriorsRun, kPriorsBatch or kPriorsNone -> what refuses an entry that takes no prior (kPriorsNone: nothing)
int mb_refused_by(int pending) { return refused_prior((PriorKind)pending, kPriorsNone); }

// every workgroup of the launch for n_act hypotheses on a virtual grid of V: -> 0, or the number of violations
//   every (entry, virtual workgroup) is served exactly once, in entry-major order;
//   the record words (n_values per workgroup) of different hypotheses are disjoint, even (value halves of 16-byte chunks) and inside the
//   hypothesis' share of the table; the ticket words are distinct and inside the hand-off block's share
int mb_check_grid(uint32_t V, uint32_t n_act, uint32_t n_values, uint32_t partial_stride, uint32_t sync_stride, uint32_t max_grid) {
  int bad = 0;
  std::vector<uint8_t> served((size_t)V * n_act, 0), word((size_t)partial_stride * n_act, 0), tick((size_t)sync_stride * n_act, 0);
  for (uint32_t b = 0; b < V * n_act; ++b) {
    const MatchBatchSlot s = match_batch_slot(b, V);
    if (s.entry >= n_act || s.vb >= V || s.entry * V + s.vb != b) { ++bad; continue; }
    if (served[(size_t)s.entry * V + s.vb]++) ++bad;
    const size_t h = s.entry;  // (the identity list of a group)
    for (uint32_t a = 0; a < n_values; ++a) {
      const size_t w = match_batch_partial_word(h, partial_stride, a, s.vb, max_grid);
      if (w < h * partial_stride || w >= (h + 1) * partial_stride || (w - h * partial_stride) % 2 != 0) { ++bad; continue; }
      if (word[w]++) ++bad;
    }
  }
  for (uint8_t v : served) bad += v != 1;
  for (uint32_t h = 0; h < n_act; ++h) {
    const size_t t = match_batch_ticket_word(h, sync_stride);
    if (t < (size_t)h * sync_stride || t >= (size_t)(h + 1) * sync_stride) { ++bad; continue; }
    if (tick[t]++) ++bad;
  }
  return bad;
}

}  // extern "C"

int main() {
  // the batch's reservations (kernels.h): 256 x 40 chunks of two doubles per hypothesis, 544 words of hand-off block, 29 sums, grids up to 256
  int bad = 0;
  for (uint32_t V : {1u, 2u, 16u, 256u})
    for (uint32_t n_act : {1u, 5u, 64u}) bad += mb_check_grid(V, n_act, 29, 256 * 40 * 2, 544, 256);
  for (int pending = 1; pending <= 3; ++pending) bad += mb_refused_by(pending) != pending;
  bad += mb_refused_by(kPriorsNone) != kPriorsNone;
  std::printf("match_batch_host: %d violations\n", bad);
  return bad ? 1 : 0;
}
