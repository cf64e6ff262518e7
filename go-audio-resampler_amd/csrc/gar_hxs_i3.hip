// gar_hxs_i3.hip -- explicit hxs_kernel instantiations (parallel build unit 3): the f16 / bf16
// stereo frame-pair store layout (VST 5)
#include "gar_hxs.hpp"

namespace gar {
GAR_HXS_FOR_HALF(GAR_HXS_INST)
}  // namespace gar
