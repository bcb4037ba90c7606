// explicit instantiation: RecoverImpl<Ed25519> (k_recover_masks, k_recover_confirm are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "recover.hpp"
namespace bpp {
template struct RecoverImpl<Ed25519>;
}
