// Channel pullback launches, fp32: every (n_in, n_out)  (see dpr_api_channels_pullback.h)
#include "dpr_api_channels_pullback.h"

namespace dpr {
DPR_CHANNELS_PULLBACK_OUT(float, 1)
DPR_CHANNELS_PULLBACK_OUT(float, 2)
DPR_CHANNELS_PULLBACK_OUT(float, 3)
DPR_CHANNELS_PULLBACK_OUT(float, 4)
}  // namespace dpr
