// Host-side checks of the launch plan of k_fixed_msm (csrc/fixed_plan.hpp: blocks_per_proof, fixed_plan, fixed_block_of),
// compiled with g++; the kernel and the verifier's host side run the same code.  tests/test_fixed_plan_cpu.py drives it.
//   sweep                       NF in {10, 66, 130, 258, 514, 1026, 2050, 8194} x count in {1..4200, 8192, 16384, 40000} x
//                               every Horner form: per against a literal copy of the formula the plan was added to, the
//                               rule for long_count, the block map as a bijection, the number of partial blocks, the size
//                               of the short zone.  Prints "ok sweep <launches> <planned>"; the first violation goes to
//                               stderr and the exit status is 1.
//   plan <NF>:<count>:<form>..  per case one line "per long_count blocks"
//   map <per> <long_count> <bid>..   per block one line "proof part per_here"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/fixed_plan.hpp"
using namespace bpp;

// the yardstick: blocks_per_proof as it stood before there was a plan (impl_verify.hpp, FIXED_BLOCK = 128), kept literally
static unsigned old_cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }
static unsigned old_blocks_per_proof(uint32_t NF, size_t count) {
    const unsigned maxb = old_cdiv(NF, 128);
    size_t tpp = ((size_t)1 << 18) / (count ? count : 1);
    tpp = std::max<size_t>(128, std::min<size_t>(tpp, NF));
    const unsigned b_lat = old_cdiv(tpp, 128);
    const unsigned b_thr = std::min<unsigned>(old_cdiv((size_t)32768, count ? count : 1), std::max<unsigned>(1, NF / (128 * 4)));
    return std::max(1u, std::min(std::max(b_lat, b_thr), maxb));
}

#define REQUIRE(cond)                                                                                            \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            fprintf(stderr, "sweep NF=%u count=%zu form=%u: %s (line %d)\n", NF, count, form, #cond, __LINE__);  \
            return false;                                                                                        \
        }                                                                                                        \
    } while (0)

static bool sweep_one(uint32_t NF, size_t count, uint32_t form, std::vector<uint8_t>& seen, size_t& planned) {
    const FixedPlan p = fixed_plan(NF, count, form);
    REQUIRE(p.per == old_blocks_per_proof(NF, count));
    REQUIRE(p.per == blocks_per_proof(NF, count) && p.per >= 1);
    // the rule, restated: the large-batch form, more proofs than are resident, a throughput-bound per of at least 2
    const bool want = form == 0 && count > 1024 && NF / 512 >= 2 && p.per >= 2;
    REQUIRE(p.long_count == (want ? count - 1024 : 0));
    REQUIRE(p.long_count < count);
    const size_t shorts = count - p.long_count;
    REQUIRE(shorts == (p.long_count ? (size_t)1024 : count) && (count > 1024 || shorts == count));   // min(count, RES) under a plan
    if (p.long_count) {
        REQUIRE(NF / (FIXED_BLOCK * p.per) >= 4);   // a short lane keeps its four whole generators,
        REQUIRE(NF / FIXED_BLOCK >= 8);             // a long lane has at least eight
        planned++;
    }
    const size_t blocks = fixed_plan_blocks(p, count);
    REQUIRE(blocks == p.long_count + shorts * p.per && blocks <= count * p.per && blocks < ((size_t)1 << 31));
    // every block lands on its own (proof, part), and every (proof, part) of the plan has a block
    seen.assign(count * p.per, 0);
    for (size_t bid = 0; bid < blocks; bid++) {
        uint32_t proof, part, per_here;
        fixed_block_of((uint32_t)bid, p.per, (uint32_t)p.long_count, proof, part, per_here);
        REQUIRE(proof < count && part < per_here);
        REQUIRE(per_here == (proof < p.long_count ? 1u : p.per));
        REQUIRE((bid < p.long_count) == (proof < p.long_count));
        uint8_t& cell = seen[(size_t)proof * p.per + part];
        REQUIRE(cell == 0);
        cell = 1;
    }
    size_t hit = 0;
    for (size_t proof = 0; proof < count; proof++)
        for (uint32_t part = 0; part < p.per; part++) {
            const bool exists = part < (proof < p.long_count ? 1u : p.per);
            REQUIRE((seen[proof * p.per + part] != 0) == exists);
            hit += exists;
        }
    REQUIRE(hit == blocks);
    return true;
}

static int sweep() {
    static const uint32_t NFS[] = {10, 66, 130, 258, 514, 1026, 2050, 8194};
    std::vector<size_t> counts;
    for (size_t c = 1; c <= 4200; c++) counts.push_back(c);
    for (size_t c : {(size_t)8192, (size_t)16384, (size_t)40000}) counts.push_back(c);
    std::vector<uint8_t> seen;
    size_t launches = 0, planned = 0;
    for (uint32_t NF : NFS)
        for (size_t count : counts)
            for (uint32_t form = 0; form < 4; form++) {
                if (!sweep_one(NF, count, form, seen, planned)) return 1;
                launches++;
            }
    printf("ok sweep %zu %zu\n", launches, planned);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "sweep")) return sweep();
    if (!strcmp(mode, "plan")) {
        for (int a = 2; a < argc; a++) {
            unsigned NF, form;
            unsigned long long count;
            if (sscanf(argv[a], "%u:%llu:%u", &NF, &count, &form) != 3) return 2;
            const FixedPlan p = fixed_plan(NF, (size_t)count, form);
            printf("%u %zu %zu\n", p.per, p.long_count, fixed_plan_blocks(p, (size_t)count));
        }
        return 0;
    }
    if (!strcmp(mode, "map")) {
        if (argc < 4) return 2;
        const uint32_t per = (uint32_t)strtoul(argv[2], nullptr, 10), lc = (uint32_t)strtoul(argv[3], nullptr, 10);
        if (per == 0) return 2;
        for (int a = 4; a < argc; a++) {
            uint32_t proof, part, per_here;
            fixed_block_of((uint32_t)strtoul(argv[a], nullptr, 10), per, lc, proof, part, per_here);
            printf("%u %u %u\n", proof, part, per_here);
        }
        return 0;
    }
    return 2;
}
