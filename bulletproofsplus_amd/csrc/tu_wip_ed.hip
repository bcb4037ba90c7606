// explicit instantiation: WipImpl<Ed25519> (the kernels of the WIP seam are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "impl_wip.hpp"
namespace bpp {
template struct WipImpl<Ed25519>;
}
