// explicit instantiation: FindImpl<Secp256k1> (k_amounts_seal, k_view_tags, k_find_confirm, k_find_count, k_find_offsets, k_find_emit, k_find_tags, k_find_list, k_find_scan_list, k_find_confirm_list are compiled in this translation unit only)
#define BPP_IMPL_DEFINITIONS 1
#include "find.hpp"
namespace bpp {
template struct FindImpl<Secp256k1>;
}
