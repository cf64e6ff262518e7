// gar_hxs_i6.hip -- explicit instantiations of the streaming kernels with the clip / peak meter, NS 6 .. 10 (parallel build unit 6)
#define GAR_HXS_METER_BUILD 1
#include "gar_hxs.hpp"

namespace gar {
GAR_HXS_FOR_METER_HI(GAR_HXS_INST_METER)
}  // namespace gar
