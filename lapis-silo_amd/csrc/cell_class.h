// cell_class.h — the class of a cell against the store's own reference: K18's rule on symbol indices, written once
// for the whole-sequence cell counts of K22 (silo_gpu_cell_counts.hip) and the region values of K23 (silo_gpu_region_counts.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace silo_gpu_cell_class {

/// The class of a cell in K18's `stats` order; SAME counts nowhere.
enum CellClass : uint32_t { SUBSTITUTION = 0, DELETION = 1, MISSING = 2, AMBIGUOUS = 3, SAME = 4 };
constexpr uint32_t GAP_SYMBOL = 0;  // '-' in both alphabets

/// Bit s for every symbol index s that is a valid mutation symbol: -ACGT of "-ACGTRYSWKMBDHVN", and all of
/// "-ACDEFGHIKLMNPQRSTVWYBZ*X" but B, Z and X (fillCharTable, store_internal.h).
constexpr uint32_t VALID_NUCLEOTIDES = 0x1Fu;
constexpr uint32_t VALID_AMINO_ACIDS = 0x1FFFFFu | (1u << 23);

/// The class of the symbol index `symbol` (31, a cell that nothing stored claims: ambiguous) where the reference holds `reference`:
/// K18's rule on indices.  A reference symbol that is not valid equals no valid symbol.
__host__ __device__ __forceinline__ uint32_t classOf(uint32_t symbol, uint32_t reference, uint32_t missing, uint32_t valid) {
   if (symbol == missing) {
      return MISSING;
   }
   if (symbol >= 32u || ((valid >> symbol) & 1u) == 0) {
      return AMBIGUOUS;
   }
   if (symbol == reference) {
      return SAME;
   }
   return symbol == GAP_SYMBOL ? DELETION : SUBSTITUTION;
}

}  // namespace silo_gpu_cell_class
