// multihover_f32.hip — MultiHoverAviary kernels and launchers for Real = float (own translation unit so
// the kernel instantiations compile in parallel)
#include "multihover_launch.h"

template int multihover_step<float>(adrp_t*, const float*, float*, float*, uint8_t*, uint8_t*, float*, hipStream_t);
template int multihover_reset<float>(adrp_t*, const uint8_t*, float*, hipStream_t);
