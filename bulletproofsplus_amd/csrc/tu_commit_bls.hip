// explicit instantiation: CommitImpl<Bls12381> (k_commit_batch is compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "commit.hpp"
namespace bpp {
template struct CommitImpl<Bls12381>;
}
