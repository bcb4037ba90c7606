// explicit instantiation: ProveImpl and ProveBatchImpl of Ed25519 (their kernels are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "impl_prove.hpp"
#include "impl_prove_batch.hpp"
namespace bpp {
template struct ProveImpl<Ed25519>;
template struct ProveBatchImpl<Ed25519>;
}
