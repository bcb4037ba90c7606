// explicit instantiation: ProveImpl and ProveBatchImpl of Bls12381 (their kernels are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "impl_prove.hpp"
#include "impl_prove_batch.hpp"
namespace bpp {
template struct ProveImpl<Bls12381>;
template struct ProveBatchImpl<Bls12381>;
}
