// explicit instantiation: ProveImpl and ProveBatchImpl of Secp256k1 (their kernels are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "impl_prove.hpp"
#include "impl_prove_batch.hpp"
namespace bpp {
template struct ProveImpl<Secp256k1>;
template struct ProveBatchImpl<Secp256k1>;
}
