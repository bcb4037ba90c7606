// explicit instantiation: FindImpl<Bls12381> (k_amounts_seal, k_find_confirm, k_find_count, k_find_offsets, k_find_emit are compiled in this translation unit only)
// and FindTagsImpl<Bls12381> (k_view_tags, k_find_tags, k_find_list, k_find_scan_list, k_find_confirm_list) beside it: the tagged call
// launches find.hpp's compaction kernels, which live here
#define BPP_IMPL_DEFINITIONS 1
#include "find_tags.hpp"
namespace bpp {
template struct FindImpl<Bls12381>;
template struct FindTagsImpl<Bls12381>;
}
