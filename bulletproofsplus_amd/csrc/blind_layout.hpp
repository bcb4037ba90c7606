// blind_layout.hpp -- the blinding scalars of one proof, as the prover lays them out (prover_batch.hpp) and as whoever reads
// proofs back finds them (recover_terms.hpp): [alpha, r, s, delta, eta, d_L[0..k), d_R[0..k)], k = log2(n m).  Plain C++.
#pragma once
#include <stdint.h>

#include "field.hpp"

namespace bpp {

BPP_HD uint32_t pb_blind_elems(uint32_t k) { return 5 + 2 * k; }
enum { PB_BL_ALPHA = 0, PB_BL_R = 1, PB_BL_S = 2, PB_BL_DELTA = 3, PB_BL_ETA = 4, PB_BL_DL = 5 };

}  // namespace bpp
