// Channel pullback launches, fp64: n_out <= 3  (see dpr_api_channels_pullback.h)
#include "dpr_api_channels_pullback.h"

namespace dpr {
DPR_CHANNELS_PULLBACK_OUT(double, 1)
DPR_CHANNELS_PULLBACK_OUT(double, 2)
DPR_CHANNELS_PULLBACK_OUT(double, 3)
}  // namespace dpr
