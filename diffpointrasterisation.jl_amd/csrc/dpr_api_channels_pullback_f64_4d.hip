// Channel pullback launches, fp64: n_out = 4, the largest kernels  (see dpr_api_channels_pullback.h)
#include "dpr_api_channels_pullback.h"

namespace dpr {
DPR_CHANNELS_PULLBACK_OUT(double, 4)
}  // namespace dpr
