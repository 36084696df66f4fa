// ctrl_f64.hip — CtrlAviary / VelocityAviary kernels and launchers for Real = double (own translation
// unit so the kernel instantiations compile in parallel)
#include "ctrl_launch.h"

template int ctrl_step<double>(adrp_t*, const float*, const void*, float*, float*, uint8_t*, uint8_t*, hipStream_t);
template int ctrl_reset<double>(adrp_t*, const uint8_t*, float*, hipStream_t);
