// explicit instantiation: OutputsImpl<Secp256k1> (k_outputs_make, k_out_tags, k_out_confirm are compiled in this translation unit only; k_find_offsets, k_find_list, k_find_count, k_find_emit here as well as in tu_find_*.hip)
#define BPP_IMPL_DEFINITIONS 1
#include "outputs.hpp"
namespace bpp {
template struct OutputsImpl<Secp256k1>;
}
