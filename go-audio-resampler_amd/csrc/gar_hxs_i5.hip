// gar_hxs_i5.hip -- explicit instantiations of the streaming kernels with the clip / peak meter, NS 1 .. 5 (parallel build unit 5)
#define GAR_HXS_METER_BUILD 1
#include "gar_hxs.hpp"

namespace gar {
GAR_HXS_FOR_METER_LO(GAR_HXS_INST_METER)
}  // namespace gar
