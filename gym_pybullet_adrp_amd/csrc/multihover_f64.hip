// multihover_f64.hip — MultiHoverAviary kernels and launchers for Real = double (own translation unit so
// the kernel instantiations compile in parallel)
#include "multihover_launch.h"

template int multihover_step<double>(adrp_t*, const float*, float*, float*, uint8_t*, uint8_t*, float*, hipStream_t);
template int multihover_reset<double>(adrp_t*, const uint8_t*, float*, hipStream_t);
