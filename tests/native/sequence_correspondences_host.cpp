// Host build of what so_icp_sequence_correspondences adds to the device-free headers, for the CPU suite
// (tests/test_sequence_correspondences_host.py drives it through ctypes; built on demand by the test, g++ -O2 -ffp-contract=off like the
// library):
//   reg_plan.h    selection_ticket: which (entry, tile) a workgroup of the export works on, from the ticket it drew and the prefix table
//                 of the entries' tile counts; sequence_status_ranges: where every entry's status row starts
//                 batch_selection_first_bad, batch_record_ranges: the check and the record ranges the export shares with the batch's
#include "reg_plan.h"

using namespace soicp::host;

extern "C" {

void sc_ticket(uint32_t t, const uint32_t* tile_first, uint32_t n_sel, uint32_t out[2]) {
  const BatchTicket b = selection_ticket(t, tile_first, n_sel, tile_first[n_sel]);
  out[0] = b.entry; out[1] = b.tile;
}
uint64_t sc_status_ranges(const size_t* n_points, const int32_t* frames, int n_sel, uint64_t* first_status) {
  return sequence_status_ranges(n_points, frames, n_sel, first_status);
}
int sc_selection_first_bad(const int32_t* frames, int n_sel, int n_frames) { return batch_selection_first_bad(frames, n_sel, n_frames); }
uint64_t sc_record_ranges(const uint32_t* accepted, const uint8_t* valid, const int32_t* frames, int n_sel, uint64_t* first_record) {
  return batch_record_ranges(accepted, valid, frames, n_sel, first_record);
}

}  // extern "C"
