// explicit instantiation: WipImpl<Secp256k1> (the kernels of the WIP seam are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "impl_wip.hpp"
namespace bpp {
template struct WipImpl<Secp256k1>;
}
