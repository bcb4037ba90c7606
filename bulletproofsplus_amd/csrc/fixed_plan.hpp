// fixed_plan.hpp -- the launch geometry of k_fixed_msm (kernels.hpp): how many blocks a proof's fixed generators are cut
// into, which proofs of a large batch get ONE long block instead, and the map from a block of the grid back to
// (proof, part).  No device types: a host compiler builds this header as it is (tests/host/fixed_plan_host_test.cpp), the
// kernel and the host side (impl_verify.hpp) include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "field.hpp"

namespace bpp {

constexpr unsigned FIXED_BLOCK = 128;

// Blocks of k_fixed_msm the chip holds at a time: 256 CUs x 4 SIMDs x 2 waves of the 13-limb kernel, two waves a block.
// blocks_per_proof's "rounds", the lone form (impl_verify.hpp) and the short zone of fixed_plan all count in it.
//
// The short zone: the LAST FIXED_RESIDENT proofs of a planned launch keep `per` short blocks each, which is `per` rounds
// of blocks 1 / per as long as a long one -- one long block's duration.  Workgroups start in grid order, so every long
// block has started by the time the first short one does, and is over before the short zone is: no long block is ever the
// tail of the launch, the tail is made of the same short blocks as without the plan.
constexpr size_t FIXED_RESIDENT = 1024;
#ifndef BPP_FIXED_SHORT_PROOFS   // tuning builds only (A/B of the plan on one box): proofs of the short zone; huge = plan off
#define BPP_FIXED_SHORT_PROOFS FIXED_RESIDENT
#endif

// Blocks per proof of a launch over `count` proofs of NF fixed generators.  This is the geometry of EVERY block of the
// launch unless fixed_plan makes the leading proofs long, and of the short zone if it does.
inline unsigned blocks_per_proof(uint32_t NF, size_t count) {
    const unsigned maxb = (NF + FIXED_BLOCK - 1) / FIXED_BLOCK;
    // small batches: aim at ~2^18 resident threads; at least one block, at most one generator per thread
    size_t tpp = ((size_t)1 << 18) / (count ? count : 1);
    tpp = std::max<size_t>(FIXED_BLOCK, std::min<size_t>(tpp, NF));
    const unsigned b_lat = (unsigned)((tpp + FIXED_BLOCK - 1) / FIXED_BLOCK);
    // large batches: the chip holds FIXED_RESIDENT blocks at a time, and a launch of only a few such rounds ends with a
    // long, mostly idle tail (8 rounds of 5 ms blocks: the last 3.5 ms ran 64 blocks).  Aim at >= 32 rounds,
    // but keep at least four generators per lane so that a block's prologue stays amortised.  Short blocks are needed
    // at the END of the launch only: fixed_plan below gives the proofs before the last FIXED_RESIDENT one block each.
    const unsigned b_thr = std::min<unsigned>((unsigned)((32 * FIXED_RESIDENT + (count ? count : 1) - 1) / (count ? count : 1)),
                                              std::max<unsigned>(1, NF / (FIXED_BLOCK * 4)));
#ifdef BPP_FORCE_PER   // tuning builds only (A/B of the launch geometry on one box)
    if (count >= FIXED_RESIDENT) return std::max(1u, std::min<unsigned>(BPP_FORCE_PER, maxb));
#endif
    return std::max(1u, std::min(std::max(b_lat, b_thr), maxb));
}

// proofs [0, long_count): ONE block each (part 0 of 1); the rest: `per` blocks each
struct FixedPlan {
    unsigned per;
    size_t long_count;
};

// The plan of a launch over `count` proofs in Horner form horner_form (0..3, as k_fixed_msm takes it).  per is always
// blocks_per_proof.  Long blocks exist only where they cannot be the tail and have something to save:
//   * the one-lane-per-proof Horner form (0), the form of the large batches -- the others wait for latency;
//   * more proofs than the short zone holds;
//   * a `per` that the throughput bound set, NF / (4 FIXED_BLOCK) >= 2, and that is >= 2: a long lane then has at least
//     8 whole generators, and there is a per-block cost to fold away (beyond 16384 proofs per is 1 already).
// A long block spares its proof per - 1 sets of FIXED_BLOCK per-thread partials (each a conversion and a store in the
// kernel, a general addition in k_partials_fold), per - 1 prologues and epilogues per lane, and most of the left-over
// step: NF = 2050 over 512 lanes is 57 steps for 56.05 additions a lane, over 128 lanes 225 for 224.2.  Measured at
// (64, 16) x 8192, the partials are what pays: the folds fall from 1.10 to 0.52 ms a pass, the kernel stays within its
// run-to-run spread (DESIGN 6a').
inline FixedPlan fixed_plan(uint32_t NF, size_t count, uint32_t horner_form) {
    FixedPlan p{blocks_per_proof(NF, count), 0};
    const size_t short_proofs = (size_t)(BPP_FIXED_SHORT_PROOFS);
    if (horner_form == 0 && count > FIXED_RESIDENT && count > short_proofs && NF / (FIXED_BLOCK * 4) >= 2 && p.per >= 2)
        p.long_count = count - short_proofs;
    return p;
}

// partial blocks of a planned launch (the grid behind the Horner blocks); never more than count * per
inline size_t fixed_plan_blocks(const FixedPlan& p, size_t count) { return p.long_count + (count - p.long_count) * p.per; }

// block bid of that grid -> its proof, its part among the per_here blocks that share the proof's generators
BPP_HD void fixed_block_of(uint32_t bid, uint32_t per, uint32_t long_count, uint32_t& proof, uint32_t& part,
                           uint32_t& per_here) {
    if (bid < long_count) {
        proof = bid;
        part = 0;
        per_here = 1;
    } else {
        const uint32_t r = bid - long_count;
        proof = long_count + r / per;
        part = r % per;
        per_here = per;
    }
}

}  // namespace bpp
