// Host build of what so_icp_batch_correspondences adds to the device-free headers, for the CPU suite
// (tests/test_batch_correspondences_host.py drives it through ctypes; built on demand by the test, g++ -O2 -ffp-contract=off like the
// library):
//   reg_plan.h    batch_selection_first_bad, batch_record_ranges: the selection's check and its record ranges
//                 selection_ticket: which (entry, tile) a workgroup of the export works on, from the ticket it drew -- for a batch
//                 over the uniform prefix table tile_first[k] = k * nblk
#include "reg_plan.h"

using namespace soicp::host;

extern "C" {

// hyp: n_sel indices or NULL (0 .. n_sel - 1) -> the first entry outside [0, n_hyp), -1: none
int bc_selection_first_bad(const int32_t* hyp, int n_sel, int n_hyp) { return batch_selection_first_bad(hyp, n_sel, n_hyp); }
// accepted, valid: per hypothesis of the batch; first_record: n_sel + 1 -> the records of the whole selection
uint64_t bc_record_ranges(const uint32_t* accepted, const uint8_t* valid, const int32_t* hyp, int n_sel, uint64_t* first_record) {
  return batch_record_ranges(accepted, valid, hyp, n_sel, first_record);
}
void bc_ticket(uint32_t t, const uint32_t* tile_first, uint32_t n_sel, uint32_t out[2]) {
  const BatchTicket b = selection_ticket(t, tile_first, n_sel, tile_first[n_sel]);
  out[0] = b.entry; out[1] = b.tile;
}

}  // extern "C"
