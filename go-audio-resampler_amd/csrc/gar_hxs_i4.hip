// gar_hxs_i4.hip -- explicit instantiations of the streaming kernels with the dithered PCM quantizer (parallel build unit 4)
#include "gar_hxs.hpp"

namespace gar {
GAR_HXS_FOR_DITHER(GAR_HXS_INST_DITHER)
}  // namespace gar
