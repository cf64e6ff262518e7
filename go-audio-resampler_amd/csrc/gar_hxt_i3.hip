// gar_hxt_i3.hip -- explicit hxt_kernel instantiations with the lean loaders (parallel build unit 3)
#include "gar_hxt.hpp"

namespace gar {
GAR_HXT_FOR_LEAN(GAR_HXT_INST_LEAN)
}  // namespace gar
