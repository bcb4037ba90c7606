// explicit instantiation: RecoverKeysImpl<Ed25519> (k_recover_coeffs, k_scan_keys, k_scan_keys_confirm are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "recover_keys.hpp"
namespace bpp {
template struct RecoverKeysImpl<Ed25519>;
}
