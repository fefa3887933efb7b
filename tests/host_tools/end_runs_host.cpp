// Hooks into the host-only rule of the end runs of the gap symbol (layout_choice.h) for the CPU unit tests.
#include <stdint.h>

#include "../../lapis-silo_amd/csrc/layout_choice.h"

extern "C" {

int end_run_covers(uint32_t layout, uint32_t derived_symbol, uint32_t gap_symbol, uint64_t residual, uint64_t row_bytes, uint64_t key_cost) {
   return silo_gpu_layout::endRunCovers(static_cast<uint8_t>(layout), static_cast<uint8_t>(derived_symbol), gap_symbol, residual, row_bytes, key_cost) ? 1 : 0;
}

uint64_t end_run_residual(uint64_t row_bits, uint64_t sequences, uint64_t ends_before, uint64_t trails_from) {
   return silo_gpu_layout::endRunResidual(row_bits, sequences, ends_before, trails_from);
}

int end_runs_pay(uint64_t covered_rows, uint64_t row_bytes, uint64_t end_events, uint64_t residual_keys, uint64_t key_cost) {
   return silo_gpu_layout::endRunsPay(covered_rows, row_bytes, end_events, residual_keys, key_cost) ? 1 : 0;
}

uint32_t end_run_key_cost(void) {
   return silo_gpu_layout::KEY_COST_BYTES;
}

}  // extern "C"
