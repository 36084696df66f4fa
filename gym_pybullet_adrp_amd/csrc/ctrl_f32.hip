// ctrl_f32.hip — CtrlAviary / VelocityAviary kernels and launchers for Real = float (own translation
// unit so the kernel instantiations compile in parallel)
#include "ctrl_launch.h"

template int ctrl_step<float>(adrp_t*, const float*, const void*, float*, float*, uint8_t*, uint8_t*, hipStream_t);
template int ctrl_reset<float>(adrp_t*, const uint8_t*, float*, hipStream_t);
