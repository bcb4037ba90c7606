// explicit instantiation: CommitImpl<Ed25519> (k_commit_batch is compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "commit.hpp"
namespace bpp {
template struct CommitImpl<Ed25519>;
}
